"""lirec_eval_clip_topk without a GPU: the export and its struct, every LIREC_EINVAL of the contract before any device call,
the library's host-side dry run, and the rank rule the kernel implements (tests/topk_cases.py) held to the host Precision on
the reference's own fixtures and to ``np.argsort(-x, kind='stable')`` on rows with ties, +-0, NaN and +-inf."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import topk_cases as TC
from golden_util import GOLDEN
from lirec_amd import _lib, ops
from lirec_amd.metrics import Precision

DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
X, Y, SOFT, CTR, CONF = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000     # fake, aligned, never dereferenced
FX = dict(np.load(os.path.join(GOLDEN, 'metrics.npz')))
SOFT_FX = dict(np.load(os.path.join(GOLDEN, 'metrics_soft.npz')))


def _args(**kw):
    a = _lib.EvalTopkArgs()
    a.logits, a.ld_logits, a.y, a.y_stride, a.counters, a.B, a.C = X, 101, Y, 1, CTR, 8, 101
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_export_and_struct_size():
    L = _lib.lib()
    assert 'lirec_eval_clip_topk' in _lib.EXPORTS and hasattr(L, 'lirec_eval_clip_topk')
    assert L.lirec_abi_sizeof(13) == C.sizeof(_lib.EvalTopkArgs) == 80
    assert L.lirec_abi_sizeof(14) == -1 and L.lirec_abi_sizeof(99) == -1
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert ops.EVAL_TOPK_COUNTERS == TC.COUNTERS


BAD = {
    'null logits': dict(logits=None), 'null y': dict(y=None), 'null counters': dict(counters=None),
    'B < 0': dict(B=-1), 'C < 1': dict(C=0), 'C < 0': dict(C=-3), 'ld_logits < C': dict(ld_logits=100),
    'y_stride < 0': dict(y_stride=-1),
    'soft without n_soft': dict(soft=SOFT, n_soft=0, ld_soft=4), 'soft with n_soft < 0': dict(soft=SOFT, n_soft=-2, ld_soft=4),
    'ld_soft < n_soft': dict(soft=SOFT, n_soft=5, ld_soft=4),
    'logits misaligned': dict(logits=X + 2), 'y misaligned (int32)': dict(y=Y + 2), 'y misaligned (int64)': dict(y=Y + 4, loader_types=1),
    'soft misaligned (fp32)': dict(soft=SOFT + 1, n_soft=4, ld_soft=4),
    'soft misaligned (float64)': dict(soft=SOFT + 4, n_soft=4, ld_soft=4, loader_types=1),
    'counters misaligned': dict(counters=CTR + 4), 'conf misaligned': dict(conf=CONF + 4),
    'C over the limit': dict(C=_lib.EVAL_TOPK_MAX_C + 1, ld_logits=_lib.EVAL_TOPK_MAX_C + 1),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_invalid_arguments_are_refused_before_any_device_call(what):
    """not in the dry mode: a call that got past the checks would reach the HIP runtime, which has no device here"""
    L = _lib.lib()
    assert L.lirec_eval_clip_topk(C.byref(_args(**BAD[what])), None) == EINVAL, what


def test_null_struct_and_empty_batch():
    L = _lib.lib()
    assert L.lirec_eval_clip_topk(None, None) == EINVAL
    assert L.lirec_eval_clip_topk(C.byref(_args(B=0)), None) == 0                       # no launch
    assert L.lirec_eval_clip_topk(C.byref(_args(B=0, C=0)), None) == EINVAL             # (the checks come first)


def test_valid_calls_in_the_dry_mode():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_eval_clip_topk(C.byref(_args()), None) == 0
        assert L.lirec_eval_clip_topk(C.byref(_args(conf=CONF, soft=SOFT, n_soft=101, ld_soft=101, loader_types=1)), None) == 0
        assert L.lirec_eval_clip_topk(C.byref(_args(y=Y + 4, soft=SOFT + 4, n_soft=3, ld_soft=8)), None) == 0      # 4-byte types
        assert L.lirec_eval_clip_topk(C.byref(_args(y_stride=0, ld_logits=3 * 101)), None) == 0
        big = _lib.EVAL_TOPK_MAX_C
        assert L.lirec_eval_clip_topk(C.byref(_args(C=big, ld_logits=big)), None) == 0
        assert L.lirec_eval_clip_topk(C.byref(_args(C=1, ld_logits=1, B=1)), None) == 0
        # recorded into a command list like every other launch
        assert L.lirec_record_begin() == 0
        assert L.lirec_eval_clip_topk(C.byref(_args()), None) == 0
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0 and L.lirec_cmdlist_size(h) == 1
        assert L.lirec_cmdlist_destroy(h) == 0
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def test_binding_refuses_host_tensors():
    with pytest.raises((_lib.LirecError, AssertionError)):
        ops.eval_clip_topk(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32), torch.zeros(8, dtype=torch.int64))


# ---- the rank rule --------------------------------------------------------------------------------------------------------
def test_rank_rule_reproduces_the_reference_counters_on_metrics_npz():
    x, y = FX['up_probs'], FX['up_gt']
    Cn = x.shape[1]
    conf = np.zeros((Cn, Cn))
    got = TC.rank_counters(x, y, conf=conf)
    p = Precision()
    cm = p.update_probs(torch.from_numpy(x.copy()), torch.from_numpy(y), conf_mat=np.zeros((Cn, Cn)))
    assert got[:4] == [p.total, p._top1, p._top3, p._top5] == [int(FX[k]) for k in ('up_total', 'up_top1', 'up_top3', 'up_top5')]
    assert np.array_equal(conf, cm) and np.array_equal(conf, FX['up_conf'])
    # the float32 cast the device path evaluates leaves the fixture tie-free, so its counters apply to the kernel unchanged
    assert TC.tie_free(x.astype(np.float32))


def test_rank_rule_reproduces_the_reference_counters_on_metrics_soft_npz():
    Cn = SOFT_FX['logits0'].shape[1]
    conf, total = np.zeros((Cn, Cn)), np.zeros(6, dtype=np.int64)
    p, cm = Precision(soft_gt=True), np.zeros((Cn, Cn))
    for it in range(3):
        x, y, s = SOFT_FX['logits%d' % it], SOFT_FX['gt%d' % it], SOFT_FX['soft%d' % it]
        assert TC.tie_free(x.astype(np.float32))
        total += TC.rank_counters(x, y, soft=s, conf=conf)
        cm = p.update_probs(torch.from_numpy(x.copy()), torch.from_numpy(y), soft_labels=torch.from_numpy(s), conf_mat=cm)
    assert total.tolist() == [int(getattr(p, k)) for k in TC.COUNTERS]
    assert total.tolist() == [int(SOFT_FX[k]) for k in ('total', 'top1', 'top3', 'top5', 'top1_sf', 'top5_sf')]
    assert np.array_equal(conf, cm) and np.array_equal(conf, SOFT_FX['conf'])


@pytest.mark.parametrize('Cn', [8, 11, 40])
def test_rank_rule_is_the_stable_descending_argsort_on_adversarial_rows(Cn):
    x, y, soft = TC.adversarial(Cn)
    assert not TC.tie_free(x)
    r = TC.ranks(x)
    order = TC.stable_order(x)
    assert np.array_equal(np.argsort(r, axis=1), order)                     # rank is a permutation: its inverse is the order
    assert np.array_equal(np.take_along_axis(r, order, 1), np.tile(np.arange(Cn), (len(x), 1)))
    conf_r, conf_h = np.zeros((Cn, Cn)), np.zeros((Cn, Cn))
    assert TC.rank_counters(x, y, soft=soft, conf=conf_r) == TC.host_counters(x, y, soft=soft, conf=conf_h)
    assert np.array_equal(conf_r, conf_h) and conf_r.sum() == ((y >= 0) & (y < Cn)).sum()
    assert TC.rank_counters(x, y)[:4] == TC.host_counters(x, y)[:4]


def test_rank_rule_on_random_rows_with_forced_ties():
    rng = np.random.default_rng(5)
    x = rng.integers(-3, 4, size=(200, 17)).astype(np.float32)               # heavy ties
    x[rng.random(x.shape) < 0.05] = np.nan
    x[rng.random(x.shape) < 0.05] = -0.0
    x[rng.random(x.shape) < 0.03] = np.inf
    x[rng.random(x.shape) < 0.03] = -np.inf
    y = rng.integers(-1, 18, size=200)
    soft = rng.integers(-1, 18, size=(200, 3)).astype(np.float64)
    assert np.array_equal(np.argsort(TC.ranks(x), axis=1), TC.stable_order(x))
    a, b = np.zeros((17, 17)), np.zeros((17, 17))
    assert TC.rank_counters(x, y, soft=soft, conf=a) == TC.host_counters(x, y, soft=soft, conf=b)
    assert np.array_equal(a, b)


def test_add_device_topk_counters_round_trips():
    p = Precision(soft_gt=True)
    p.add_device_topk_counters(torch.tensor([23, 5, 9, 14, 6, 15, 77, 88]))
    assert [getattr(p, k) for k in TC.COUNTERS] == [23, 5, 9, 14, 6, 15]
    assert (p.total_cl, p.total_rels, p._trks_top1, p._cls_top1, p._rels_top1) == (0, 0, 0, 0, 0)
    p.add_device_topk_counters(np.array([1, 1, 1, 1, 0, 1, 0, 0]))
    assert [getattr(p, k) for k in TC.COUNTERS] == [24, 6, 10, 15, 6, 16]
    assert p.top1() == 6 / 24 and p.top5_sf() == 16 / 24
    q = Precision(soft_gt=True)                                             # the fold of a fold: the counters() dict is the sum
    q.add_device_topk_counters(torch.tensor([p.counters()[k] for k in TC.COUNTERS] + [0, 0]))
    assert q.counters() == p.counters()
    # add_device_counters keeps its own order
    r = Precision()
    r.add_device_counters(torch.arange(1, 9))
    assert (r.total, r.total_cl, r.total_rels, r._top1, r._trks_top1, r._cls_top1, r._rels_top1) == (1, 2, 3, 4, 5, 6, 7)
