"""Gradient clipping by global norm without a GPU: the argument checks of lirec_grad_sq_partials, lirec_clip_finalize and
lirec_set_adam_clip through the C ABI (LIREC_EINVAL before any device call) under the library's host-side dry run; the condition
under which tests/test_gpu_clip.py may hold the CLIPPED Adam launches to adam_cases' bounds -- the fp32 restatement with the scale
gs32 * coef32 stays inside them --; the recorded step's key; and the norm over the trainable ranges of a partly frozen layout."""
import ctypes as C
import math
import subprocess
import sys
import os

import numpy as np
import pytest

import adam_cases as AC
import clip_cases as CC
from lirec_amd import _lib
from lirec_amd.graph import RecordedTrainStep
from lirec_amd.optim import FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
G, PART, SQ, OUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000     # fake, aligned, never dereferenced device addresses


@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_set_adam_clip(None) == 0
        assert L.lirec_debug_set(0, -1) == 0


def _ranges(*rs):
    arr = (_lib.AdamRange * max(len(rs), 1))()
    for a, (o, k) in zip(arr, rs):
        a.offset, a.length, a.lag = o, k, 7          # (the lag is ignored)
    return arr


def test_grad_sq_partials_argument_checks(dry):
    L = dry
    one = _ranges((0, 1000))
    assert L.lirec_grad_sq_partials(G, one, 1, PART, None) == 0
    assert L.lirec_grad_sq_partials(G, _ranges((0, 0)), 1, PART, None) == 0                 # nothing to sum: the partials are zeros
    assert L.lirec_grad_sq_partials(G, _ranges(*[(8 * i, 5) for i in range(64)]), 64, PART, None) == 0
    assert L.lirec_grad_sq_partials(G + 16, one, 1, PART + 8, None) == 0
    for bad in ((None, one, 1, PART), (G, None, 1, PART), (G, one, 1, None),               # a null pointer
                (G, one, 0, PART), (G, one, -1, PART), (G, _ranges(*[(8 * i, 5) for i in range(65)]), 65, PART),   # n_ranges outside 1..64
                (G, _ranges((0, -1)), 1, PART),                                             # a negative length
                (G, _ranges((0, 8), (10, 8)), 2, PART), (G, _ranges((-4, 8)), 1, PART),     # an offset that is no multiple of 4 / negative
                (G + 4, one, 1, PART), (G + 8, one, 1, PART),                               # g not 16-byte aligned
                (G, one, 1, PART + 4)):                                                     # partials not 8-byte aligned
        assert L.lirec_grad_sq_partials(*bad, None) == EINVAL, bad


def test_clip_finalize_argument_checks(dry):
    L = dry
    for mode in (0, 1, 2):
        assert L.lirec_clip_finalize(PART, SQ, mode, 1.0, 1.0, OUT, None) == 0
    assert L.lirec_clip_finalize(None, SQ, 2, 0.5, 1e9, OUT + 4, None) == 0                 # mode 2 reads no partials
    for bad in ((None, SQ, 0, 1.0, 1.0, OUT), (None, SQ, 1, 1.0, 1.0, OUT), (PART, None, 0, 1.0, 1.0, OUT), (PART, SQ, 0, 1.0, 1.0, None),
                (PART, SQ, 3, 1.0, 1.0, OUT), (PART, SQ, -1, 1.0, 1.0, OUT),
                (PART, SQ, 0, 1.0, 0.0, OUT), (PART, SQ, 0, 1.0, -1.0, OUT), (PART, SQ, 0, 1.0, float('nan'), OUT),
                (PART + 4, SQ, 0, 1.0, 1.0, OUT), (PART, SQ + 4, 0, 1.0, 1.0, OUT), (PART, SQ, 0, 1.0, 1.0, OUT + 2)):
        assert L.lirec_clip_finalize(*bad, None) == EINVAL, bad


def test_set_adam_clip_reaches_the_three_adam_calls(dry):
    L = dry
    p, g, m, v = (0x50000000 + 0x4000000 * i for i in range(4))
    hyper = (3e-5, .9, .999, 1e-8, 1e-5, 1.0)
    rs = (_lib.AdamRange * 1)()
    rs[0].offset, rs[0].length, rs[0].lag = 0, 100, 0

    def calls():
        return (L.lirec_adam_step(p, g, m, v, 100, 1, *hyper, None, None),
                L.lirec_adam_step_counted(p, g, m, v, 100, *hyper, SQ, OUT, 1, None),
                L.lirec_adam_step_ranges(p, g, m, v, rs, 1, 1, *hyper, None, None, None, 0, None))
    assert calls() == (0, 0, 0)
    assert L.lirec_set_adam_clip(OUT + 2) == EINVAL
    assert L.lirec_set_adam_clip(OUT) == 0
    assert calls() == (0, 0, 0)                                   # (recorded, the launches carry the pointer by value)
    assert L.lirec_record_begin() == 0
    assert calls() == (0, 0, 0)
    h = C.c_void_p()
    assert L.lirec_record_end(C.byref(h)) == 0
    kinds = []
    for i in range(L.lirec_cmdlist_size(h)):
        s, k = C.c_void_p(), C.c_int32()
        assert L.lirec_cmdlist_command(h, i, C.byref(s), C.byref(k)) == 0
        kinds.append(k.value)
    assert kinds.count(0) == 3                                    # one launch each (the rest: profiling brackets)
    assert L.lirec_set_adam_clip(None) == 0
    assert L.lirec_cmdlist_replay(h, 0, -1) == 0 and L.lirec_cmdlist_destroy(h) == 0
    assert calls() == (0, 0, 0)


def test_the_folded_first_layer_update_is_refused_while_a_coefficient_is_set(dry):
    """its launch finishes the very gradients the norm needs: it cannot be clipped, and is not silently left unclipped"""
    from lirec_amd import ops
    L = dry
    # a plain head on the persistent layer-1 kernels, the only path that takes the folded update (gemm mode 2, a split-K scratch)
    J, dims, rows = 256, [256, 512], 33
    n_flat = (J * sum(dims) + 2 * J + 63) // 64 * 64 + 64
    _addr = lambda i: 0x10000000 + 0x4000000 * i
    g_at = _addr(20)

    def _fused():
        return _lib.FusedAdamArgs(_addr(21), g_at, _addr(22), _addr(23), _addr(24), 0, n_flat, sum(J * d + J for d in dims), 3,
                                  1e-3, .9, .999, 1e-8, 1e-5, 1.0, None)

    def _bwd(L, adam):
        a = _lib.EmbedBwdArgs()
        a.X, a.ldx = _addr(0), sum(dims)
        a.H1, a.dZ2, a.lddz2 = _addr(1), _addr(2), 32
        for arr, vals in ((a.W2, [_addr(3), _addr(4)]), (a.dW2, [_addr(5), _addr(6)]), (a.db2, [_addr(7), _addr(8)]),
                          (a.dW1, [g_at, g_at + 4 * J * dims[0]]), (a.db1, [g_at + 4 * J * sum(dims), g_at + 4 * (J * sum(dims) + J)]),
                          (a.in_off, [0, dims[0]]), (a.in_dim, dims), (a.out_dim, [16, 16])):
            for i, x in enumerate(vals):
                arr[i] = x
        a.rows, a.nseg, a.J, a.parts = rows, 2, J, 4
        a.sel = _lib.RowSel(1, 2, 0)
        a.workspace, a.workspace_bytes = _addr(9), L.lirec_workspace_bytes(rows, 2, J)
        a.planes, a.planes_bytes = _addr(10), L.lirec_planes_bytes(rows, sum(dims), J, 0)
        if adam is not None:
            a.adam = C.cast(C.pointer(adam), C.c_void_p)
        return L.lirec_embed_bwd(C.byref(a), None)
    mode = L.lirec_get_gemm_mode()
    assert L.lirec_set_gemm_mode(2) == 0 and L.lirec_set_scratch(_addr(30), 256 << 20) == 0
    try:
        assert _bwd(L, _fused()) == 0
        assert L.lirec_set_adam_clip(OUT) == 0
        assert _bwd(L, _fused()) == EINVAL and _bwd(L, None) == 0
        assert L.lirec_set_adam_clip(None) == 0
        assert _bwd(L, _fused()) == 0
    finally:
        assert L.lirec_set_scratch(None, 0) == 0 and L.lirec_set_gemm_mode(mode) == 0
        ops._scratch.pop(ops._ctx_key(), None)


def test_the_whole_host_stack_with_clipping_in_the_dry_run():
    """every recipe's eager and recorded step with opt.clip_grad_norm set, through the real Python host stack (a process of its
    own: the dry run patches torch and switches the library process-wide)"""
    code = ('import host_dryrun as H, torch\n'
            'from lirec_amd import _lib, ops\n'
            'from lirec_amd.config import opt\n'
            'L = _lib.lib(); assert L.lirec_debug_set(H.DRY, -1) == 0; H.patch()\n'
            'small = dict(text_dim=24, visual_dim=32, track_dim=32, joint_dim=16)\n'
            'big = dict(text_dim=768, visual_dim=2048, track_dim=2048, joint_dim=512)\n'
            'ops.set_gemm_mode(2)\n'
            'for kind, a in (("int_rel_ch", (11, 5, 4, 6, 3)), ("int_rels", (11, 5, 5, 1, 3)), ("int_ch", (11, 5, 4, 6, 0))):\n'
            '    H.one_recipe(kind, small, *a, clip_grad_norm=0.5)\n'
            'H.one_recipe("int_rel_ch", big, 101, 15, 8, 16, 18, steps=1, features="q32", clip_grad_norm=0.5)\n'
            'opt.clip_grad_norm = 0.0\n'
            'print("clipped dry run ok")\n')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'clipped dry run ok' in r.stdout, r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds still hold with the coefficient
# ---------------------------------------------------------------------------------------------------------------------------
_worst = {}


@pytest.mark.parametrize('coef', CC.COEFS, ids=['c%g' % c for c in CC.COEFS])
def test_clipped_fp32_restatement_stays_inside_the_bounds(coef):
    """The clipped kernels round the scale gs * coef to fp32 once more than the unclipped ones round gs.  For every case of
    adam_cases.CASES the fp32 restatement with that scale stays inside adam_cases.bounds of the float64 definition with the exact
    product: the GPU test may hold the clipped launches to these bounds.  The largest use of a bound is printed.

    Coefficients 1, 0.37 and 1e-3.  2^-20 was tried and is DROPPED (clip_cases.DROPPED_COEFS): case h0-t2-g1 uses 2.12 of the bound
    on p' with it.  Not through the extra rounding -- the product 1 * 2^-20 is exact -- but because g * 2^-20 ~ 1e-6 then meets the
    weight-decay term wd * p ~ 1e-6 with the other sign: where the sum cancels and v = 0, the update's denominator sqrt((1 - b2)
    g'^2) follows |g'| itself, whose roundings are relative to its two terms; the bound on p' allows for that in the numerator
    (G) only.  A property of the bound at gradients as small as the weight decay, clipped or not; the bound is not widened."""
    worst = (0.0, None)
    for case in AC.CASES:
        h = AC.hyper32(case.hyper)
        s = AC.make_state(case, AC.N_HOST)
        got = CC.ref32(*s, case.step, h, coef)
        assert all(np.isfinite(x).all() for x in got)
        use = CC.use_of_bounds(got, *s, case.step, h, coef)
        worst = max(worst, (max(use), case.id))
        assert max(use) < 1.0, (case.id, coef, use)
    _worst[coef] = worst
    print('coef %g: largest use of a bound %.3f (case %s)' % (coef, worst[0], worst[1]))


def test_coefficient_one_is_the_unclipped_update():
    for case in AC.CASES[:8]:
        h = AC.hyper32(case.hyper)
        s = AC.make_state(case, 1001)
        for a, b in zip(CC.ref32(*s, case.step, h, 1.0), AC.ref32(*s, case.step, h)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# the recorded step's key
# ---------------------------------------------------------------------------------------------------------------------------
class _Opt:
    def __init__(self, **kw):
        self.param_groups = [dict(lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)]
        self.grad_scale = 1.0
        self.__dict__.update(kw)


def test_recording_key_carries_the_clip_bound():
    base = RecordedTrainStep.hyper_key(_Opt())                    # (a stand-in without the attribute: the key as it always was)
    assert RecordedTrainStep.hyper_key(_Opt(max_grad_norm=None)) == base
    assert RecordedTrainStep.hyper_key(_Opt(max_grad_norm=0)) == base
    assert RecordedTrainStep.hyper_key(_Opt(max_grad_norm=0.0)) == base
    k1, k2 = RecordedTrainStep.hyper_key(_Opt(max_grad_norm=1.0)), RecordedTrainStep.hyper_key(_Opt(max_grad_norm=2.0))
    assert k1 != base and k2 != base and k1 != k2
    assert RecordedTrainStep.hyper_key(_Opt(max_grad_norm=1.0)) == k1
    assert base == (3e-5, (0.9, 0.999), 1e-8, 1e-5, 1.0)


def test_max_grad_norm_values():
    class M:
        pass
    o = FusedAdam.__new__(FusedAdam)
    for off in (None, 0, 0.0):
        o.max_grad_norm = off
        assert o._clip_max() is None
    o.max_grad_norm = 2
    assert o._clip_max() == 2.0
    for bad in (-1.0, float('nan')):
        o.max_grad_norm = bad
        with pytest.raises(ValueError):
            o._clip_max()


# ---------------------------------------------------------------------------------------------------------------------------
# the norm over the trainable ranges
# ---------------------------------------------------------------------------------------------------------------------------
def test_norm_over_trainable_ranges_leaves_the_frozen_slice_out():
    """a layout with a frozen middle parameter (and alignment gaps, which hold zeros): the norm over FusedAdam.merged_ranges is the
    norm of the trainable parameters' elements, whatever the frozen slice holds"""
    offsets = {'a.weight': (0, 10), 'a.bias': (12, 3), 'b.weight': (16, 21), 'b.bias': (40, 5), 'c.weight': (48, 7)}
    extent = 56
    r = np.random.default_rng(3)
    g = np.zeros(extent, np.float32)
    for n, (o, k) in offsets.items():
        g[o:o + k] = r.standard_normal(k).astype(np.float32)
    trainable = {n: n != 'b.weight' for n in offsets}
    rs = FusedAdam.merged_ranges(offsets, trainable, {}, extent)
    assert rs == [(0, 15, 0), (40, 56, 0)]
    want = math.sqrt(math.fsum(float(x) ** 2 for n, (o, k) in offsets.items() if trainable[n] for x in g[o:o + k]))
    assert CC.norm_over(g, [(a, b) for a, b, _ in rs]) == want
    g2 = g.copy()
    g2[16:37] = 1e30                                             # whatever a shared launch left in the frozen slice
    assert CC.norm_over(g2, [(a, b) for a, b, _ in rs]) == want
    assert CC.norm_over(g2, [(0, extent)]) > 1e30                # ... which a norm over the whole buffer would count
    # nothing frozen: one range, the whole buffer
    assert FusedAdam.merged_ranges(offsets, {n: True for n in offsets}, {}, extent) == [(0, extent, 0)]
    # a lag splits ranges of the UPDATE; the norm takes offsets and lengths only
    rs = FusedAdam.merged_ranges(offsets, {n: True for n in offsets}, {'b.bias': 2}, extent)
    assert [(a, b) for a, b, _ in rs] == [(0, 37), (40, 45), (48, 56)]
    assert CC.norm_over(g, [(a, b) for a, b, _ in rs]) == CC.norm_over(g, [(0, extent)])       # (the gaps hold zeros; fsum is exact)


def test_the_norm_route_under_data_parallelism_is_refused_before_any_counter_is_attached(monkeypatch):
    """the refusal comes from FusedAdam.route() with the constructor's other argument checks: nothing of the optimiser or the
    model has been touched when it is raised"""
    from lirec_amd import config
    from lirec_amd import model as M
    from lirec_amd._lib import LirecError
    from lirec_amd.config import opt
    attached = []
    monkeypatch.setattr(RecordedTrainStep, '_attach_counters', lambda self: attached.append(self))
    try:
        config.recipe('int_rel_ch', joint_dim=16, rels_n_clips=3, text_dim=24, visual_dim=32, track_dim=32)
        opt.device = 'cpu'
        model, loss, optim = M.create_model(11, n_rels=5)
        model.train()
        model.grad_sync = type('Sync', (), dict(world=2))()
        for setting in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
            for k, v in setting.items():
                setattr(optim, k, v)
            assert optim.route().norm and optim.route().parallel
            with pytest.raises(LirecError, match='under data parallelism is not recorded'):
                RecordedTrainStep(model, loss, optim, {})
            assert optim._step_dev is None and model._seed_dev is None and not attached
            optim.max_grad_norm, optim.skip_nonfinite = None, False
        assert optim.route().refuse is None
    finally:
        config.reset()
