"""Skipping non-finite steps without a GPU: the argument checks of lirec_clip_finalize_guard and lirec_set_adam_guard through the C
ABI (LIREC_EINVAL before any device call) under the library's host-side dry run; the setting reaches the four Adam calls and does
not stick; the folded first-layer update is refused while a guard is set; the recorded step's key; the whole host stack with the
guard on; and the accounting -- FusedAdam's (step, lag, S) against a per-parameter count kept by hand."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import guard_cases as GC
from lirec_amd import _lib
from lirec_amd.graph import RecordedTrainStep
from lirec_amd.optim import FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
PART, SQ, OUT, SK = 0x20000000, 0x30000000, 0x40000000, 0x48000000     # fake, aligned, never dereferenced device addresses


@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_set_adam_guard(None, None) == 0
        assert L.lirec_set_adam_clip(None) == 0
        assert L.lirec_debug_set(0, -1) == 0


def test_clip_finalize_guard_argument_checks(dry):
    L = dry
    for mode in (0, 1, 2):
        for count in (0, 1):
            assert L.lirec_clip_finalize_guard(PART, SQ, mode, 1.0, 1.0, OUT, SK, count, None) == 0
    assert L.lirec_clip_finalize_guard(None, SQ, 2, 0.5, 0.0, OUT + 4, None, 0, None) == 0      # max_norm 0: no clipping; no counter
    assert L.lirec_clip_finalize_guard(PART, SQ, 0, 1.0, 1e9, OUT, SK + 8, 1, None) == 0
    for bad in ((None, SQ, 0, 1.0, 1.0, OUT, SK, 0), (None, SQ, 1, 1.0, 1.0, OUT, SK, 0),       # partials NULL with mode 0 / 1
                (PART, None, 0, 1.0, 1.0, OUT, SK, 0), (PART, SQ, 0, 1.0, 1.0, None, SK, 0),    # sq / out NULL
                (PART, SQ, 3, 1.0, 1.0, OUT, SK, 0), (PART, SQ, -1, 1.0, 1.0, OUT, SK, 0),      # a mode outside 0..2
                (PART, SQ, 0, 1.0, -1.0, OUT, SK, 0), (PART, SQ, 0, 1.0, float('nan'), OUT, SK, 0),     # max_norm negative / NaN
                (PART, SQ, 2, 1.0, 1.0, OUT, None, 1),                                          # count without a counter
                (PART + 4, SQ, 0, 1.0, 1.0, OUT, SK, 0), (PART, SQ + 4, 0, 1.0, 1.0, OUT, SK, 0),
                (PART, SQ, 0, 1.0, 1.0, OUT + 2, SK, 0), (PART, SQ, 0, 1.0, 1.0, OUT, SK + 4, 1)):      # misaligned
        assert L.lirec_clip_finalize_guard(*bad, None) == EINVAL, bad


def test_set_adam_guard_argument_checks(dry):
    L = dry
    assert L.lirec_set_adam_guard(OUT, SK) == 0 and L.lirec_set_adam_guard(OUT + 4, SK + 8) == 0
    for bad in ((OUT, None), (None, SK), (OUT + 2, SK), (OUT, SK + 4)):
        assert L.lirec_set_adam_guard(*bad) == EINVAL, bad
    assert L.lirec_set_adam_guard(None, None) == 0


def test_set_adam_guard_reaches_the_four_adam_calls_and_does_not_stick(dry):
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
                L.lirec_adam_step_counted(p, g, m, v, 100, *hyper, SQ, OUT + 64, 1, None),
                L.lirec_adam_step_ranges(p, g, m, v, rs, 1, 1, *hyper, None, None, None, 0, None),
                L.lirec_adam_step_groups(p, g, m, v, gr, 1, table, 1, 1, 1.0, None, None, None, 0, None))

    def launched_bytes():
        """the recorded launches of calls(): (number of launches, total commands)"""
        assert L.lirec_record_begin() == 0
        assert calls() == (0, 0, 0, 0)
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0
        kinds = []
        for i in range(L.lirec_cmdlist_size(h)):
            s, k = C.c_void_p(), C.c_int32()
            assert L.lirec_cmdlist_command(h, i, C.byref(s), C.byref(k)) == 0
            kinds.append(k.value)
        assert L.lirec_cmdlist_replay(h, 0, -1) == 0 and L.lirec_cmdlist_destroy(h) == 0
        return kinds.count(0), len(kinds)
    assert calls() == (0, 0, 0, 0)
    plain = launched_bytes()
    assert L.lirec_set_adam_guard(OUT, SK) == 0
    assert calls() == (0, 0, 0, 0)
    assert launched_bytes() == plain and plain[0] == 4           # one launch each, guarded or not
    assert L.lirec_set_adam_clip(OUT) == 0                       # (the guard takes precedence: still fine)
    assert calls() == (0, 0, 0, 0)
    assert L.lirec_set_adam_guard(None, None) == 0 and L.lirec_set_adam_clip(None) == 0
    assert calls() == (0, 0, 0, 0)


def test_ops_adam_guard_clears_the_setting_when_a_launch_raises(dry):
    """seen through the folded update's refusal: EINVAL inside the block, fine after it"""
    import torch
    from lirec_amd import ops
    L = dry
    out, skipped = torch.zeros(4), torch.zeros(1, dtype=torch.int64)
    keep = ops._p
    ops._p = lambda t: None if t is None else t.data_ptr()
    try:
        with pytest.raises(ZeroDivisionError):
            with ops.adam_guard(out, skipped):
                assert _bwd_fused(L) == EINVAL
                1 / 0
        assert _bwd_fused(L) == 0
        with ops.adam_guard(None):
            assert _bwd_fused(L) == 0
    finally:
        ops._p = keep
        _bwd_fused(L, done=True)


_J, _DIMS, _ROWS = 256, [256, 512], 33


def _addr(i):
    return 0x10000000 + 0x4000000 * i


def _bwd_fused(L, fused=True, done=False):
    """a plain head on the persistent layer-1 kernels, the only path that takes the folded update (gemm mode 2, a split-K scratch):
    lirec_embed_bwd with (or without) lirec_embed_bwd_args::adam, as tests/test_host_clip.py builds it"""
    from lirec_amd import ops
    st = _bwd_fused.__dict__
    if done:
        if 'mode' in st:
            assert L.lirec_set_scratch(None, 0) == 0 and L.lirec_set_gemm_mode(st.pop('mode')) == 0
            ops._scratch.pop(ops._ctx_key(), None)
        return None
    if 'mode' not in st:
        st['mode'] = L.lirec_get_gemm_mode()
        assert L.lirec_set_gemm_mode(2) == 0 and L.lirec_set_scratch(_addr(30), 256 << 20) == 0
    J, dims, rows = _J, _DIMS, _ROWS
    n_flat = (J * sum(dims) + 2 * J + 63) // 64 * 64 + 64
    g_at = _addr(20)
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
    adam = None
    if fused:
        adam = _lib.FusedAdamArgs(_addr(21), g_at, _addr(22), _addr(23), _addr(24), 0, n_flat, sum(J * d + J for d in dims), 3,
                                  1e-3, .9, .999, 1e-8, 1e-5, 1.0, None)
        a.adam = C.cast(C.pointer(adam), C.c_void_p)
    return L.lirec_embed_bwd(C.byref(a), None)


def test_the_folded_first_layer_update_is_refused_while_a_guard_is_set(dry):
    """its launch finishes the very gradients the decision needs: it cannot be guarded, and is not silently left unguarded"""
    L = dry
    try:
        assert _bwd_fused(L) == 0
        assert L.lirec_set_adam_guard(OUT, SK) == 0
        assert _bwd_fused(L) == EINVAL and _bwd_fused(L, fused=False) == 0
        assert L.lirec_set_adam_guard(None, None) == 0
        assert _bwd_fused(L) == 0
    finally:
        _bwd_fused(L, done=True)


def test_the_whole_host_stack_with_the_guard_in_the_dry_run():
    """every recipe's eager and recorded step with opt.skip_nonfinite set, alone and with clipping, through the real Python host
    stack (a process of its own: the dry run patches torch and switches the library process-wide)"""
    code = ('import host_dryrun as H, torch\n'
            'from lirec_amd import _lib, ops\n'
            'from lirec_amd.config import opt\n'
            'L = _lib.lib(); assert L.lirec_debug_set(H.DRY, -1) == 0; H.patch()\n'
            'small = dict(text_dim=24, visual_dim=32, track_dim=32, joint_dim=16)\n'
            'big = dict(text_dim=768, visual_dim=2048, track_dim=2048, joint_dim=512)\n'
            'ops.set_gemm_mode(2)\n'
            'for kind, a in (("int_rel_ch", (11, 5, 4, 6, 3)), ("int_rels", (11, 5, 5, 1, 3)), ("int_ch", (11, 5, 4, 6, 0))):\n'
            '    m = H.one_recipe(kind, small, *a, skip_nonfinite=True)\n'
            '    H.one_recipe(kind, small, *a, skip_nonfinite=True, clip_grad_norm=0.5)\n'
            'm = H.one_recipe("int_rel_ch", big, 101, 15, 8, 16, 18, steps=1, features="q32", skip_nonfinite=True)\n'
            'opt.clip_grad_norm = 0.0; opt.skip_nonfinite = False\n'
            'print("guarded dry run ok")\n')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'guarded dry run ok' in r.stdout, r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------
# the recorded step's key
# ---------------------------------------------------------------------------------------------------------------------------
class _Opt:
    def __init__(self, **kw):
        self.param_groups = [dict(lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)]
        self.grad_scale = 1.0
        self.__dict__.update(kw)


def test_recording_key_carries_the_flag_only_when_on():
    base = RecordedTrainStep.hyper_key(_Opt())                    # (a stand-in without the attribute: the key as it always was)
    assert base == (3e-5, (0.9, 0.999), 1e-8, 1e-5, 1.0)
    assert RecordedTrainStep.hyper_key(_Opt(skip_nonfinite=False)) == base
    on = RecordedTrainStep.hyper_key(_Opt(skip_nonfinite=True))
    assert on == base + (('skip_nonfinite', True),)
    both = RecordedTrainStep.hyper_key(_Opt(skip_nonfinite=True, max_grad_norm=2.0))
    assert both == base + (('max_grad_norm', 2.0), ('skip_nonfinite', True))
    assert RecordedTrainStep.hyper_key(_Opt(skip_nonfinite=False, max_grad_norm=2.0)) == base + (('max_grad_norm', 2.0),)


def test_the_keyword_and_the_config_entry():
    import inspect
    from lirec_amd.config import opt
    assert inspect.signature(FusedAdam.__init__).parameters['skip_nonfinite'].default is False
    assert opt.skip_nonfinite is False


# ---------------------------------------------------------------------------------------------------------------------------
# the accounting: (step, lag, S) against a count kept by hand
# ---------------------------------------------------------------------------------------------------------------------------
class _Counter:
    """stands in for the device int64: S, injected"""

    def __init__(self, s):
        self.s, self.reads = s, 0

    def item(self):
        self.reads += 1
        return self.s

    def zero_(self):
        self.s = 0


class _P:
    def __init__(self):
        self.requires_grad = True


def _fake(n=4):
    import torch
    o = FusedAdam.__new__(FusedAdam)
    o._names = ['p%d' % i for i in range(n)]
    o.model = type('M', (), {})()
    o.model._plist = [_P() for _ in range(n)]
    o.state = {p: {'step': torch.tensor(0.)} for p in o.model._plist}
    o._lag, o._step, o._step_dev, o._skipped_folded = {}, 0, None, 0
    o._guard_flags, o._skipped_dev, o._ranges_key = None, _Counter(0), None
    o.skip_nonfinite = True
    return o


def _call(o, led, skipped):
    """what one guarded step() does to the host's books (fold, count, flags of the interval, lags) and to S"""
    o.fold_if_due()
    o._step += 1
    flags = o._flags()
    if o.skip_nonfinite:
        o._guard_flags = flags
        o._skipped_dev.s += int(skipped and any(flags))           # (nothing trainable: no decision, no count)
    o._advance_lags()
    return led.call(flags, skipped and o.skip_nonfinite and any(flags))


def _steps(o):
    o._sync_state_steps()
    return [int(o.state[p]['step']) for p in o.model._plist]


def test_state_dict_steps_and_the_fold_against_a_count_kept_by_hand():
    o, led = _fake(), GC.Ledger(4)
    P = o.model._plist
    script = [  # (frozen parameters, skipped?)
        ((), False), ((), True), ((), False),              # everything trainable: one skipped of three
        ((1,), False), ((1,), True), ((1,), True),         # p1 frozen: two more skipped, which p1 did not "miss"
        ((1, 2), False),                                   # the frozen set changes: a fold is due here
        ((), True), ((), False),                           # ... and again
        ((0, 1, 2, 3), True),                              # nothing trainable: no decision, no count
        ((3,), False)]
    for frozen, skipped in script:
        for i, p in enumerate(P):
            p.requires_grad = i not in frozen
        want = _call(o, led, skipped)
        assert _steps(o) == want, (frozen, skipped, _steps(o), want, o._step, o._lag, o._skipped_dev.s)
        # state_dict leaves every counter alone
        before = (o._step, dict(o._lag), o._skipped_dev.s, o._guard_flags)
        _steps(o)
        assert (o._step, dict(o._lag), o._skipped_dev.s, o._guard_flags) == before
    assert o._step == len(script)  - o._skipped_folded and o.skipped_total() == o._skipped_folded + o._skipped_dev.s
    assert led.count == [6, 4, 5, 5] and o.skipped_total() == 4


def test_the_pure_accounting_functions():
    # 10 calls, 3 skipped; lags 0 / 4 (frozen now) / 2 (trainable, was frozen before the interval)
    flags, lags = (True, False, True), [0, 4, 2]
    assert FusedAdam.updates_received(10, lags, flags, 3) == [7, 6, 5]
    step, lags2 = FusedAdam.folded(10, lags, flags, 3)
    assert (step, lags2) == (7, [0, 1, 2])
    assert FusedAdam.updates_received(step, lags2, flags, 0) == [7, 6, 5]


def test_switching_the_guard_off_folds_and_a_fold_under_a_device_step_raises():
    o, led = _fake(2), GC.Ledger(2)
    for skipped in (False, True, True, False):
        _call(o, led, skipped)
    assert o._step == 4 and o._skipped_dev.s == 2 and _steps(o) == [2, 2]
    o.skip_nonfinite = False
    o._step_dev = object()                       # a recorded step holds the step on the device
    with pytest.raises(RuntimeError, match='release'):
        o.fold_if_due()
    o._step_dev = None
    o.fold_if_due()
    assert (o._step, o._lag, o._skipped_dev.s, o._guard_flags) == (2, {}, 0, None) and _steps(o) == [2, 2]
    reads = o._skipped_dev.reads
    o.fold_if_due()                              # nothing due: no read
    _steps(o)
    assert o._skipped_dev.reads == reads
