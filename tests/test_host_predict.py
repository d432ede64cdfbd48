"""lirec_predict_clips without a GPU: the export and its struct, every LIREC_EINVAL of the contract before any device call, the
library's host-side dry run, and the host restatement the kernel is held to (lirec_amd.metrics.joint_predictions / top_lists,
lirec_amd.predict.pair_scores): against a brute-force loop, against the reference's own counters through the refactored
Precision, and the facts about the test inputs that tests/test_gpu_predict.py relies on."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import predict_cases as PC
import topk_cases as TC
from golden_util import GOLDEN
from lirec_amd import _lib, ops
from lirec_amd.metrics import Precision, RelationshipsAcc, joint_predictions, top_lists
from test_metrics import COUNTERS, TIE_CASES, TIES, tie_inputs

DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
# fake, aligned, never dereferenced
INTS, RELS, MEM, OUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000
OUTPUTS = ('trk', 'cls', 'rel', 'score', 'trk_score', 'top_cls', 'top_cls_p', 'top_rel', 'top_rel_p', 'flags')
CASES = PC.named_cases()


def _args(**kw):
    a = _lib.PredictArgs()
    a.ints, a.ld_ints, a.rels, a.ld_rels, a.mem = INTS, 101, RELS, 15, MEM
    for i, k in enumerate(OUTPUTS):
        setattr(a, k, OUT + 0x100000 * i)
    a.B, a.T, a.C, a.NR, a.K = 8, 16, 101, 15, 5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_export_binding_and_struct_size():
    L = _lib.lib()
    assert 'lirec_predict_clips' in _lib.EXPORTS and hasattr(L, 'lirec_predict_clips')
    assert L.lirec_abi_sizeof(15) == C.sizeof(_lib.PredictArgs) == 144
    assert L.lirec_abi_sizeof(14) == -1 and L.lirec_abi_sizeof(16) == -1
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert _lib.PREDICT_MAX_K == 16 and ops.PREDICT_FIELDS == OUTPUTS
    import lirec_amd
    from lirec_amd.predict import Predictions, predict
    assert lirec_amd.predict is predict and callable(predict) and Predictions.fields == OUTPUTS


def lds_bytes(T, Cn, NR):
    """the header's formula"""
    return 4 * (T * Cn + (T * (NR + 1) if NR else 0) + Cn + NR) + 8 * T + 144


BAD = {
    'null ints': dict(ints=None), 'null trk': dict(trk=None),
    'every output null': {k: None for k in OUTPUTS},
    'B < 0': dict(B=-1), 'T < 1': dict(T=0), 'T < 0': dict(T=-4), 'C < 1': dict(C=0), 'K < 1': dict(K=0), 'K < 0': dict(K=-1),
    'K over the limit': dict(K=_lib.PREDICT_MAX_K + 1),
    'ld_ints < C': dict(ld_ints=100), 'ld_rels < NR': dict(ld_rels=14), 'rels with NR < 1': dict(NR=0), 'rels with NR < 0': dict(NR=-2),
    'ints misaligned': dict(ints=INTS + 2), 'rels misaligned': dict(rels=RELS + 1), 'mem misaligned (fp32)': dict(mem=MEM + 2),
    'mem misaligned (float64)': dict(mem=MEM + 4, loader_types=1),
    'score misaligned': dict(score=OUT + 4), 'trk_score misaligned': dict(trk_score=OUT + 12),
    'LDS over the limit (rels)': dict(T=343), 'LDS over the limit (no rels)': dict(T=397, rels=None),
    'LDS far over the limit': dict(T=1 << 30, C=1 << 30, ld_ints=1 << 30),
}
BAD.update({'%s misaligned' % k: {k: OUT + 2} for k in OUTPUTS if k not in ('score', 'trk_score')})


@pytest.mark.parametrize('what', sorted(BAD))
def test_invalid_arguments_are_refused_before_any_device_call(what):
    """not in the dry mode: a call that got past the checks would reach the HIP runtime, which has no device here"""
    L = _lib.lib()
    assert L.lirec_predict_clips(C.byref(_args(**BAD[what])), None) == EINVAL, what


def test_the_lds_limit_is_the_published_formula():
    assert lds_bytes(342, 101, 15) <= 160 * 1024 < lds_bytes(343, 101, 15)
    assert lds_bytes(396, 101, 0) <= 160 * 1024 < lds_bytes(397, 101, 0)


def test_null_struct_and_empty_batch():
    L = _lib.lib()
    assert L.lirec_predict_clips(None, None) == EINVAL
    assert L.lirec_predict_clips(C.byref(_args(B=0)), None) == 0                         # no launch
    assert L.lirec_predict_clips(C.byref(_args(B=0, C=0)), None) == EINVAL               # (the checks come first)


def test_valid_calls_in_the_dry_mode():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_predict_clips(C.byref(_args()), None) == 0
        assert L.lirec_predict_clips(C.byref(_args(T=342)), None) == 0                   # the LDS limit itself
        assert L.lirec_predict_clips(C.byref(_args(T=396, rels=None, NR=0)), None) == 0
        assert L.lirec_predict_clips(C.byref(_args(mem=MEM + 8, loader_types=1)), None) == 0
        assert L.lirec_predict_clips(C.byref(_args(mem=MEM + 4)), None) == 0             # 4-byte mask
        assert L.lirec_predict_clips(C.byref(_args(T=1, mem=None, rels=None, K=16)), None) == 0      # the clip-level form
        assert L.lirec_predict_clips(C.byref(_args(rels=None, NR=-7, ld_rels=0)), None) == 0         # NR is not read without rels
        only_trk = {k: None for k in OUTPUTS if k != 'trk'}
        assert L.lirec_predict_clips(C.byref(_args(**only_trk)), None) == 0
        assert L.lirec_predict_clips(C.byref(_args(ld_ints=104, ld_rels=16, B=1, T=1, C=1, NR=1, K=1)), None) == 0
        # recorded into a command list like every other launch
        assert L.lirec_record_begin() == 0
        assert L.lirec_predict_clips(C.byref(_args()), None) == 0
        assert L.lirec_predict_clips(C.byref(_args(B=0)), None) == 0                     # (no launch: nothing recorded)
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0 and L.lirec_cmdlist_size(h) == 1
        assert L.lirec_cmdlist_replay(h, 0, -1) == 0
        assert L.lirec_cmdlist_destroy(h) == 0
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def test_binding_refuses_host_tensors():
    with pytest.raises((_lib.LirecError, AssertionError)):
        ops.predict_clips(torch.zeros(4, 5), None, None, B=2, T=2)


# ---- the host restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(n for n in CASES if not n.startswith('k')))
def test_joint_predictions_match_a_brute_force_loop(name):
    case = CASES[name]
    got = joint_predictions(case['ints'].copy(), case['rels'].copy() if case['rels'] is not None else None, case['mem'])
    want = PC.brute_force(case['ints'], case['rels'], case['mem'])
    for g, w, what in zip(got, want, ('trk', 'cls', 'rel', 'score', 'trk_score')):
        assert np.array_equal(np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)), (name, what)


def test_joint_predictions_mask_in_place_and_append_the_probabilities():
    case = CASES['c']
    ints, rels = case['ints'].copy(), case['rels'].copy()
    res = joint_predictions(ints, rels, case['mem'], with_probs=True)
    pad = case['mem'] == 0
    assert pad.any() and np.isinf(ints[pad]).all() and np.isinf(rels[pad]).all()
    pc, pr = res[5], res[6]
    assert pc.dtype == np.float32 and pr.dtype == np.float64 and pr.shape[2] == rels.shape[2] + 1 and (pr[:, :, -1] == 0).all()
    assert joint_predictions(ints, None, None, with_probs=True)[6] is None
    assert (joint_predictions(ints, None, None)[2] == -1).all()


@pytest.mark.parametrize('name', TIE_CASES)
def test_precision_through_the_refactored_methods_keeps_the_fixture_counters(name):
    """tests/test_metrics.py does this too (unchanged); here next to the function the two methods now call, and with the
    per-clip predictions checked against the sigmoid implementations the device test relies on"""
    p0, p1 = Precision(), Precision()
    for it in range(2):
        ints, rels, mem, y, r, gt, jz = tie_inputs(name, it)
        t = torch.from_numpy
        NR = rels.shape[2]
        p0.update_probs_max_tracks(t(ints.copy()), t(gt), t(y), mask=t(mem), just_zeros=t(jz))
        p1.update_probs_max_tracks_rels(t(ints.copy()), t(rels.copy()), t(y), t(r), gt_tracks=t(gt), just_zeros=t(jz), mask=t(mem),
                                        rels_mask=torch.nonzero(t(r[:, 0]) - (NR + 1) + 1))
    assert [int(getattr(p0, k)) for k in COUNTERS] == TIES[name + '/mt'].tolist()
    assert [int(getattr(p1, k)) for k in COUNTERS] == TIES[name + '/mr'].tolist()


def fixture_disagreements(name, with_rels):
    """(clips, clips on which the three host sigmoids do not all give the same joint prediction) over the fixture's batches"""
    n = bad = 0
    for it in range(2):
        ints, rels, mem = tie_inputs(name, it)[:3]
        same = PC.sigmoids_agree(ints, rels if with_rels else None, mem)
        n, bad = n + len(ints), bad + int((~same).sum())
    return n, bad


@pytest.mark.parametrize('name', TIE_CASES)
def test_fixture_predictions_under_three_sigmoid_implementations(name):
    """what tests/test_gpu_predict.py may assume: exact equality is owed on six fixtures, and on `saturated` wherever the host
    sigmoids agree among themselves"""
    for with_rels, bad_saturated in ((False, 11), (True, 20)):
        n, bad = fixture_disagreements(name, with_rels)
        assert (n, bad) == ((48, bad_saturated) if name == 'saturated' else (n, 0)), (name, with_rels, n, bad)
        # joint_predictions IS the first of the three
        for it in range(2):
            ints, rels, mem = tie_inputs(name, it)[:3]
            rr = rels.copy() if with_rels else None
            got = joint_predictions(ints.copy(), rr, mem)[:3]
            want = PC.joint_under(PC.SIGMOIDS['expit_f32'], ints, rr, mem)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_exact_tie_values_are_separated_under_three_sigmoid_implementations():
    """sums of distinct value multisets -- {a, b}, {a} beside the None column's 0, and the 0 + 0 of a padded track -- differ by at
    least 1.06e-2; single probabilities (no rels) by far more"""
    for name, s in PC.SIGMOIDS.items():
        p = s(PC.TIE_VALUES).astype(np.float64)
        assert s(np.array([-np.inf], dtype=np.float32))[0] == 0
        sums = sorted([0.0] + list(p) + [p[i] + p[j] for i in range(4) for j in range(i, 4)])
        assert min(b - a for a, b in zip(sums, sums[1:])) >= 1.06e-2, name
        # the sum of one multiset is one double whichever way round it is added
        assert all(p[i] + p[j] == p[j] + p[i] for i in range(4) for j in range(4))


def test_generators_keep_their_promises():
    for name, case in CASES.items():
        assert case['ints'].dtype == np.float32 and (case['rels'] is None or case['rels'].dtype == np.float32)
        if case['exact']:
            assert np.isin(case['ints'], PC.TIE_VALUES).all()
            continue
        flags = PC.flags_of(case['ints'], case['rels'], case['mem'])
        ok = flags == 0
        with np.errstate(invalid='ignore'):
            assert (PC.joint_margin(case['ints'], case['rels'], case['mem'])[ok] > PC.MARGIN).all(), name
        ints, rels = PC.masked(case['ints'], case['rels'], case['mem'])
        trk = joint_predictions(ints.copy(), rels.copy() if rels is not None else None, None)[0]
        assert TC.tie_free(ints[ok, trk[ok]]) and (rels is None or rels.shape[2] < 2 or TC.tie_free(rels[ok, trk[ok]])), name
    assert CASES['j']['mem'][2].sum() == 0 and PC.flags_of(**{k: CASES['j'][k] for k in ('ints', 'rels', 'mem')}).tolist() == [0, 0, 2, 0]
    assert PC.flags_of(**{k: CASES['k'][k] for k in ('ints', 'rels', 'mem')}).tolist() == [0, 1, 0, 0]
    assert PC.flags_of(**{k: CASES['k_clip_level'][k] for k in ('ints', 'rels', 'mem')}).tolist() == [1, 0, 0, 1]


@pytest.mark.parametrize('K', [1, 5, 16])
def test_top_lists_are_the_stable_descending_order(K):
    for Cn in (8, 11):
        x, _, _ = TC.adversarial(Cn)
        idx, p = top_lists(x, K)
        k = min(K, Cn)
        assert idx.dtype == np.int32 and p.dtype == np.float32 and idx.shape == p.shape == (len(x), K)
        assert np.array_equal(idx[:, :k], TC.stable_order(x)[:, :k]) and (idx[:, k:] == -1).all() and (p[:, k:] == 0).all()
        from scipy.special import expit
        assert np.array_equal(p[:, :k], np.take_along_axis(expit(x), idx[:, :k].astype(np.int64), 1), equal_nan=True)
    x, _, _ = TC.random_case(3, 20, 40)
    assert np.array_equal(top_lists(x, K)[0], TC.stable_order(x)[:, :K])


def test_pair_scores_are_the_sums_of_relationships_acc():
    from lirec_amd.predict import pair_scores
    fx = dict(np.load(os.path.join(GOLDEN, 'metrics.npz')))
    ra = RelationshipsAcc(n_rels=fx['ra_probs'].shape[1] + 1)
    ra.update(torch.from_numpy(fx['ra_probs'].copy()), torch.from_numpy(fx['ra_gt']), torch.from_numpy(fx['ra_hash']))
    pairs = pair_scores(fx['ra_probs'], fx['ra_hash'])
    assert list(pairs) == list(ra._scores) and len(pairs) > 1
    assert len(fx['ra_hash']) > len(pairs)                                     # (some pair does have several clips: sums are formed)
    for h, (order, s) in pairs.items():
        assert s.dtype == ra._scores[h].dtype and np.array_equal(s, ra._scores[h])
        assert np.array_equal(order, np.argsort(-s, kind='stable'))
    ra.top1()
    assert [int(pairs[h][0][0]) for h in ra._gt] == [int(p) for _, p in ra.preds]
    # clips without a pair (hash -1) take no part
    x, h = np.concatenate([fx['ra_probs'], fx['ra_probs'][:2]]), np.concatenate([fx['ra_hash'].reshape(-1), [-1, -1]])
    again = pair_scores(x, h)
    assert list(again) == list(pairs) and all(np.array_equal(again[k][1], pairs[k][1]) for k in pairs)
