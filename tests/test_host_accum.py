"""Gradient accumulation without a GPU (FusedAdam(accumulate_steps=k); include/lirec_hip.h, "gradient accumulation"): the float64
restatement of a window and its bound (tests/accum_cases.py) with the fp32 restatement inside it; the phase arithmetic and the
per-parameter step with skipped windows; the argument checks of lirec_accum_begin and lirec_set_adam_hold under the library's
host-side dry run, the hold reaching the four Adam calls and lirec_ema_step without sticking, the folded update refused under it;
and, through the real host stack in the dry run (tests/accum_dryrun.py), what the eager loop and the recorded accumulating step
issue, and that accumulate_steps = 1 issues what an optimiser of this tree built without the argument does."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import accum_cases as XC
import adam_cases as AC
import test_host_guard as HG
from lirec_amd import _lib
from lirec_amd.graph import RecordedTrainStep
from lirec_amd.optim import FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304
EINVAL = _lib.LIREC_EINVAL
BUF, CTR, WIN = 0x20000000, 0x30000000, 0x40000000      # fake, aligned, never dereferenced device addresses


@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_set_adam_hold(None, 0) == 0
        assert L.lirec_set_adam_guard(None, None) == 0
        assert L.lirec_set_adam_clip(None) == 0
        assert L.lirec_debug_set(0, -1) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the window's restatement and its bound
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 3, 8])
def test_fp32_restatement_of_a_window_is_inside_the_widened_bounds(k):
    """ref32 on the sequential fp32 sum of k gradients with the scale gs / k, against ref64 on their float64 sum: inside
    adam_cases.bounds + the accumulation term for every case; k = 1 is adam_cases' own yardstick"""
    worst = [0.0, 0.0, 0.0]
    for c in AC.CASES:
        h = AC.hyper32(c.hyper)
        p, _, m, v = AC.make_state(c, AC.N_HOST)
        grads = XC.micro_grads(c, AC.N_HOST, k)
        got = AC.ref32(p, XC.sum32(grads), m, v, c.step, XC.window_hyper(h, k))
        use = XC.use_of_window_bounds(got, p, grads, m, v, c.step, h)
        worst = [max(a, b) for a, b in zip(worst, use)]
        assert max(use) <= 1.0, (c.id, k, use)
        if k == 1:
            assert use == AC.use_of_bounds(got, p, grads[0], m, v, c.step, h), c.id
    print('ACCUM-FIGURE host_bounds k=%d worst_use p=%.3f m=%.3f v=%.3f' % (k, *worst))


def test_the_widening_is_the_accumulation_term_and_nothing_else():
    """zero at k = 1; for k > 1 the bound on m' grows by exactly (1 - b1) gs_k (k - 1) u sum|g_i|"""
    c = AC.CASES[0]
    h = AC.hyper32(c.hyper)
    p, g, m, v = AC.make_state(c, 257)
    _, one = XC.ref64_window(p, [g], m, v, c.step, h)
    pn, mn, vn, G, A, V = AC.ref64(p, g, m, v, c.step, h)
    for a, b in zip(one, AC.bounds(p, m, G, A, V)):
        assert (a == b).all()
    grads = XC.micro_grads(c, 257, 3)
    hk = XC.window_hyper(h, 3)
    assert hk[5] == float(np.float32(h[5] / 3)) and hk[:5] == h[:5]
    _, (bp, bm, bv) = XC.ref64_window(p, grads, m, v, c.step, h)
    s = XC.sum64(grads)
    _, _, _, G, A, V = AC.ref64(p, s, m, v, c.step, hk)
    base = AC.bounds(p, m, G, A, V)
    S = sum(np.abs(np.asarray(x, np.float64)) for x in grads)
    assert np.allclose(bm - base[1], (1.0 - hk[1]) * hk[5] * 2 * AC.U * S, rtol=1e-12, atol=0)
    assert (bp >= base[0]).all() and (bv >= base[2]).all()


def test_accum_scale_is_the_float_of_the_double_quotient():
    from lirec_amd import ops
    for gs in (1.0, 0.5, 1.0 / 3.0, 0.125, 1e-3):
        for k in (1, 2, 3, 4, 7, 8):
            assert ops.accum_scale(gs, k) == XC.accum_scale(gs, k)
        assert ops.accum_scale(gs, 1) == float(np.float32(gs))
    assert ops.accum_scale(1.0, 2) == 0.5


# ---------------------------------------------------------------------------------------------------------------------------
# the phase and the per-parameter step
# ---------------------------------------------------------------------------------------------------------------------------
def test_window_after_is_the_restated_chain():
    for ks in ([1] * 5, [2] * 7, [3] * 7, [2, 2, 3, 3, 3, 1, 1, 4, 4, 4, 4, 2]):
        phase = 0
        for k, (found, zeroes, applies, _) in zip(ks, XC.chain(ks)):
            assert phase == found and (phase == 0) == zeroes
            phase, applied = FusedAdam.window_after(phase, k)
            assert applied == applies
    assert FusedAdam.window_after(0, 1) == (0, True) and FusedAdam.window_after(1, 3) == (2, False)
    # the head launch's restatement agrees with the host's
    for k in (2, 3):
        for phase0 in range(k):
            phase = phase0
            for zeroed, hold, after, ctr in XC.head_chain(k, 2 * k + 1, phase0):
                assert zeroed == (phase == 0)
                phase, applied = FusedAdam.window_after(phase, k)
                assert after == phase and hold == (0 if applied else 1)
            assert ctr[0] == 2 * k + 1 and ctr[1] == ctr[2] == (phase0 + 2 * k + 1) // k


def _fake(n=3):
    o = HG._fake(n)
    o._accum_k, o._accum_phase, o._win_dev, o.grad_scale = 1, 0, None, 1.0
    return o


def test_the_setter_and_the_phase_on_the_optimiser():
    o = _fake()
    assert o.accumulate_steps == 1 and o.accum_phase == 0
    o.accumulate_steps = 3
    assert [o._advance_window() for _ in range(7)] == [False, False, True, False, False, True, False]
    assert o.accum_phase == 1
    with pytest.raises(RuntimeError, match='middle of a window'):
        o.accumulate_steps = 2
    o.accumulate_steps = 3                       # (the same value: no change)
    o.drop_window()
    o.accumulate_steps = 2
    assert o.accum_phase == 0 and o._scale() == 0.5
    o._win_dev = object()
    with pytest.raises(RuntimeError, match='release'):
        o.accumulate_steps = 4
    with pytest.raises(RuntimeError, match='release'):
        o.drop_window()
    o._win_dev = None
    for bad in (0, -2, 1.5, True, None):
        with pytest.raises(ValueError, match='integer >= 1'):
            o.accumulate_steps = bad


def test_updates_received_with_skipped_windows():
    """step() calls in windows of k; a window with a NaN is ONE skipped step; a frozen parameter's lag grows per WINDOW"""
    import guard_cases as GC
    for k in (1, 2, 3):
        o, led = _fake(3), GC.Ledger(3)
        o.accumulate_steps = k
        P = o.model._plist
        script = [((), False), ((), True), ((1,), False), ((1,), True), ((1,), True), ((), False)]      # per window: (frozen, skipped)
        want = None
        for frozen, skipped in script:
            for i, p in enumerate(P):
                p.requires_grad = i not in frozen
            for call in range(k):
                applied = o.window_after(o.accum_phase, k)[1]
                if applied:
                    want = HG._call(o, led, skipped)          # (the apply step is the one guarded step() of the window)
                    o._advance_window()
                else:
                    before = (o._step, dict(o._lag), o._skipped_dev.s)
                    o._advance_window()                       # (a hold touches none of the books)
                    assert (o._step, dict(o._lag), o._skipped_dev.s) == before
                if want is not None:
                    assert HG._steps(o) == want, (k, frozen, skipped, call)
        assert o.accum_phase == 0 and led.count == [3, 2, 3] and o.skipped_total() == 3


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI in the dry run
# ---------------------------------------------------------------------------------------------------------------------------
def test_exports_and_the_abi_number():
    L = _lib.lib()
    assert 'lirec_accum_begin' in _lib.EXPORTS and 'lirec_set_adam_hold' in _lib.EXPORTS
    assert L.lirec_version() == _lib.ABI_VERSION


def test_accum_begin_argument_checks(dry):
    L = dry
    ev, ap = (C.c_int64 * 4)(1, 0, 0, 0), (C.c_int64 * 4)(0, 1, 1, 0)
    for k in (1, 2, 3, 1000):
        assert L.lirec_accum_begin(BUF, 4096 + 5, CTR, ev, ap, 3, WIN, k, None) == 0
    assert L.lirec_accum_begin(None, 0, CTR, ev, ap, 4, WIN, 2, None) == 0             # nothing to zero
    assert L.lirec_accum_begin(BUF, 16, None, None, None, 0, WIN + 16, 2, None) == 0   # no counters
    for bad in ((BUF, -1, CTR, ev, ap, 3, WIN, 2), (None, 16, CTR, ev, ap, 3, WIN, 2),                 # bytes < 0; p NULL with bytes
                (BUF + 4, 16, CTR, ev, ap, 3, WIN, 2), (BUF + 8, 16, CTR, ev, ap, 3, WIN, 2),          # p misaligned
                (BUF, 16, CTR, ev, ap, 5, WIN, 2), (BUF, 16, CTR, ev, ap, -1, WIN, 2),                 # n outside 0..4
                (BUF, 16, None, ev, ap, 1, WIN, 2), (BUF, 16, CTR, None, ap, 1, WIN, 2), (BUF, 16, CTR, ev, None, 1, WIN, 2),
                (BUF, 16, CTR + 4, ev, ap, 1, WIN, 2),                                                 # ctr misaligned
                (BUF, 16, CTR, ev, ap, 3, None, 2), (BUF, 16, CTR, ev, ap, 3, WIN + 8, 2), (BUF, 16, CTR, ev, ap, 3, WIN + 4, 2),
                (BUF, 16, CTR, ev, ap, 3, WIN, 0), (BUF, 16, CTR, ev, ap, 3, WIN, -3)):                # k < 1
        assert L.lirec_accum_begin(*bad, None) == EINVAL, bad


def test_set_adam_hold_argument_checks(dry):
    L = dry
    assert L.lirec_set_adam_hold(WIN + 8, 1) == 0 and L.lirec_set_adam_hold(WIN + 8, 7) == 0
    for bad in ((WIN + 8, 0), (WIN + 8, -1), (None, 2), (None, -1), (WIN + 4, 2), (WIN + 2, 2)):
        assert L.lirec_set_adam_hold(*bad) == EINVAL, bad
    assert L.lirec_set_adam_hold(None, 0) == 0


def test_hold_reaches_the_adam_and_ema_calls_and_does_not_stick(dry):
    L = dry
    p, g, m, v = (0x50000000 + 0x4000000 * i for i in range(4))
    table = 0x70000000
    hyper = (3e-5, .9, .999, 1e-8, 1e-5, 1.0)
    rs = (_lib.AdamRange * 1)()
    rs[0].offset, rs[0].length, rs[0].lag = 0, 100, 0
    gr = (_lib.AdamGroupRange * 1)()
    gr[0].offset, gr[0].length, gr[0].lag, gr[0].group = 0, 100, 0, 0

    def calls():
        return (L.lirec_adam_step(p, g, m, v, 100, 1, *hyper, None, None),
                L.lirec_adam_step_counted(p, g, m, v, 100, *hyper, CTR, CTR + 64, 1, None),
                L.lirec_adam_step_ranges(p, g, m, v, rs, 1, 1, *hyper, None, None, None, 0, None),
                L.lirec_adam_step_groups(p, g, m, v, gr, 1, table, 1, 1, 1.0, None, None, None, 0, None),
                L.lirec_ema_step(m, p, 100, 0.1, None, None))

    def launches():
        assert L.lirec_record_begin() == 0
        assert calls() == (0,) * 5
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0
        kinds = []
        for i in range(L.lirec_cmdlist_size(h)):
            s, k = C.c_void_p(), C.c_int32()
            assert L.lirec_cmdlist_command(h, i, C.byref(s), C.byref(k)) == 0
            kinds.append(k.value)
        assert L.lirec_cmdlist_replay(h, 0, -1) == 0 and L.lirec_cmdlist_destroy(h) == 0
        return kinds.count(0), len(kinds)
    plain = launches()
    assert plain[0] == 5
    assert L.lirec_set_adam_hold(WIN + 8, 3) == 0
    assert launches() == plain                                   # one launch each, gated or not
    assert L.lirec_set_adam_guard(0x48000000, 0x48000100) == 0   # with the guard ...
    assert launches() == plain
    assert L.lirec_set_adam_guard(None, None) == 0 and L.lirec_set_adam_clip(0x48000000) == 0      # ... and with a clip coefficient
    assert launches() == plain
    assert L.lirec_set_adam_clip(None) == 0 and L.lirec_set_adam_hold(None, 0) == 0
    assert launches() == plain


def test_the_folded_first_layer_update_is_refused_while_a_hold_is_set(dry):
    L = dry
    try:
        assert HG._bwd_fused(L) == 0
        assert L.lirec_set_adam_hold(WIN + 8, 2) == 0
        assert HG._bwd_fused(L) == EINVAL and HG._bwd_fused(L, fused=False) == 0
        assert L.lirec_set_adam_hold(None, 0) == 0
        assert HG._bwd_fused(L) == 0
    finally:
        HG._bwd_fused(L, done=True)


def test_ops_adam_hold_clears_the_setting_when_a_launch_raises(dry):
    import torch
    from lirec_amd import ops
    L = dry
    win = torch.zeros(4, dtype=torch.int64)
    keep = ops._p
    ops._p = lambda t: None if t is None else t.data_ptr()
    try:
        with pytest.raises(ZeroDivisionError):
            with ops.adam_hold(win[1:2], 2):
                assert HG._bwd_fused(L) == EINVAL
                1 / 0
        assert HG._bwd_fused(L) == 0
        with ops.adam_hold(None):
            assert HG._bwd_fused(L) == 0
    finally:
        ops._p = keep
        HG._bwd_fused(L, done=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the key, the keyword, the config entry
# ---------------------------------------------------------------------------------------------------------------------------
def test_recording_key_carries_k_only_when_on():
    base = RecordedTrainStep.hyper_key(HG._Opt())
    assert RecordedTrainStep.hyper_key(HG._Opt(accumulate_steps=1)) == base
    assert RecordedTrainStep.hyper_key(HG._Opt(accumulate_steps=3)) == base + (('accumulate_steps', 3),)
    assert RecordedTrainStep.hyper_key(HG._Opt(accumulate_steps=2, ema_decay=0.9)) == base + (('ema_decay', 0.9), ('accumulate_steps', 2))


def test_the_keyword_and_the_config_entry():
    from lirec_amd.config import opt
    assert inspect.signature(FusedAdam.__init__).parameters['accumulate_steps'].default == 1
    assert opt.accumulate_steps == 1


# ---------------------------------------------------------------------------------------------------------------------------
# the host stack in the dry run
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['eager_chain', 'recorded_sequences', 'refusals', 'off_is_off'])
def test_the_host_stack_in_the_dry_run(what):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'accum_dryrun.py'), what], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and what.replace('_', ' ') + ' ok' in r.stdout, r.stdout[-4000:]
