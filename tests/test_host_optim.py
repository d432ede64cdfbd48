"""The update side of the step without a GPU: the yardsticks of tests/test_gpu_optim.py checked on their own -- the fp32
restatement of the update (adam_cases.ref32) stays under half of every bound on |kernel - ref64| for every case the GPU file
runs, so the bounds admit a correct fp32 implementation --, FusedAdam._minus against a set difference, and the argument checks of
lirec_adam_step, lirec_adam_step_counted, lirec_zero_count, lirec_counter_add and lirec_fused_adam through the C ABI
(LIREC_EINVAL before any device call) under the library's host-side dry run, which hands nothing to the HIP runtime."""
import ctypes as C
import itertools

import numpy as np
import pytest

import adam_cases as AC
from lirec_amd import _lib
from lirec_amd.optim import FusedAdam

DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
A0 = 0x10000000                                # fake, aligned, never dereferenced device addresses


def _addr(i):
    return A0 + 0x4000000 * i


@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_debug_set(0, -1) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick on its own
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.CASES, ids=[c.id for c in AC.CASES])
def test_fp32_restatement_stays_under_half_of_every_bound(case):
    """ref32 is a correct fp32 implementation of the update by construction; it uses less than half of the bound on p', m' and v'
    at every size the GPU file runs the case at (and at N_HOST elements, which every case gets here)."""
    h = AC.hyper32(case.hyper)
    sizes = [n for n in AC.SIZES if n < AC.N_BIG] + [AC.N_HOST] + ([AC.N_BIG] if case in AC.BIG_CASES else [])
    for n in sizes:
        s = AC.make_state(case, n)
        got = AC.ref32(*s, case.step, h)
        assert all(np.isfinite(x).all() for x in got)
        use = AC.use_of_bounds(got, *s, case.step, h)
        assert max(use) < 0.5, (n, use)


def test_ref64_is_the_header_update_on_a_hand_computed_element():
    """one element by hand, in Python floats: torch.optim.Adam's rule with coupled weight decay (include/lirec_hip.h)"""
    lr, b1, b2, eps, wd, gs = h = AC.hyper32((1e-2, .5, .75, 1e-3, 1e-2, .5))
    p, g, m, v, t = 0.5, 2.0, 0.25, 0.0625, 2
    gg = g * gs + wd * p
    mn = b1 * m + (1 - b1) * gg
    vn = b2 * v + (1 - b2) * gg * gg
    pn = p - lr / (1 - b1 ** t) * mn / (vn ** 0.5 / (1 - b2 ** t) ** 0.5 + eps)
    got = AC.ref64(*(np.float32([x]) for x in (p, g, m, v)), t, h)
    for a, b in zip(got[:3], (pn, mn, vn)):
        assert abs(float(a[0]) - b) <= 1e-15 * abs(b)
    assert float(got[3][0]) == abs(g * gs) + abs(wd * p)


def test_case_list_covers_what_it_claims():
    assert 24 <= len(AC.CASES) <= 48 and len(set(AC.CASES)) == len(AC.CASES)
    assert {(c.hyper, c.step) for c in AC.CASES} >= set(itertools.product(range(4), AC.STEPS))
    assert {(c.hyper, c.mag) for c in AC.CASES} >= set(itertools.product(range(4), AC.MAGS))
    assert {c.hyper for c in AC.BIG_CASES} == {0, 1, 2, 3}
    assert AC.N_BIG == 2 * 2097152 + 3 * 1024 + 3 and AC.N_BIG % 4 == 3
    p, g, m, v = AC.make_state(AC.CASES[2], 5 * 7 * 11 * 13)
    for a, k in ((v, 5), (m, 7), (g, 11), (p, 13)):
        z = np.nonzero(a == 0)[0]
        assert np.array_equal(z, np.arange(k - 1, a.size, k))
    p, g, m, v = AC.make_state(AC.Case(0, 1, 1.0), 50)
    assert not m.any() and not v.any()


# ---------------------------------------------------------------------------------------------------------------------------
# FusedAdam._minus
# ---------------------------------------------------------------------------------------------------------------------------
MINUS = {
    'nothing_skipped': (0, 100, []),
    'one_inside': (0, 100, [(10, 20)]),
    'touching': (0, 100, [(10, 20), (20, 30)]),
    'overlapping': (0, 100, [(10, 25), (20, 30)]),
    'nested': (0, 100, [(10, 50), (20, 30)]),
    'nested_unsorted': (0, 100, [(20, 30), (10, 50), (60, 61)]),
    'unsorted': (0, 100, [(70, 80), (10, 20), (40, 50)]),
    'empty_skip': (0, 100, [(30, 30), (50, 40)]),
    'at_both_ends': (0, 100, [(0, 10), (90, 100)]),
    'everything': (0, 100, [(0, 100)]),
    'everything_in_two': (0, 100, [(0, 60), (60, 100)]),
    'out_of_range': (10, 90, [(0, 5), (95, 200), (-7, 10), (90, 91)]),
    'across_the_ends': (10, 90, [(0, 20), (80, 200)]),
    'wider_than_the_range': (10, 90, [(0, 200)]),
    'empty_range': (50, 50, [(10, 60)]),
    'empty_range_no_skip': (50, 50, []),
    'first_layer_bucket': (0, 64 * 37, [(64 * 21, 64 * 37)]),
    'first_layer_bucket_second_half': (64 * 21, 64 * 37, [(64 * 21, 64 * 37)]),
    'duplicates': (0, 100, [(10, 20), (10, 20)]),
}


@pytest.mark.parametrize('what', sorted(MINUS))
def test_minus_is_the_set_difference(what):
    lo, hi, skip = MINUS[what]
    got = FusedAdam._minus(lo, hi, skip)
    assert got == AC.minus_ref(lo, hi, skip)
    assert all(isinstance(r, tuple) and lo <= r[0] < r[1] <= hi for r in got)


def test_minus_against_the_set_difference_on_random_lists():
    r = np.random.default_rng(5)
    for _ in range(300):
        lo, hi = sorted(int(x) for x in r.integers(0, 60, 2))
        skip = [tuple(int(x) for x in r.integers(-5, 70, 2)) for _ in range(int(r.integers(0, 5)))]
        assert FusedAdam._minus(lo, hi, skip) == AC.minus_ref(lo, hi, skip), (lo, hi, skip)


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
HY = (3e-5, 0.9, 0.999, 1e-8, 1e-5, 1.0)


def _adam(L, **kw):
    v = dict(p=_addr(0), g=_addr(1), m=_addr(2), v=_addr(3), n=1023, step=3, hy=HY, step_dev=None)
    v.update(kw)
    return L.lirec_adam_step(v['p'], v['g'], v['m'], v['v'], v['n'], v['step'], *v['hy'], v['step_dev'], None)


def _counted(L, **kw):
    v = dict(p=_addr(0), g=_addr(1), m=_addr(2), v=_addr(3), n=1023, hy=HY, count=_addr(4), ticket=_addr(5), advance=1)
    v.update(kw)
    return L.lirec_adam_step_counted(v['p'], v['g'], v['m'], v['v'], v['n'], *v['hy'], v['count'], v['ticket'], v['advance'], None)


MISALIGNED = [{k: _addr(i) + off} for i, k in enumerate('pgmv') for off in (4, 8, 12)]


@pytest.mark.parametrize('kw', [dict(n=-1), dict(step=0), dict(step=-3), dict(p=None), dict(g=None), dict(m=None), dict(v=None)]
                         + MISALIGNED, ids=lambda kw: '-'.join('%s_%s' % (k, v if v is None or abs(v) < 99 else 'plus%d' % (v & 15))
                                                               for k, v in kw.items()))
def test_adam_step_argument_checks(dry, kw):
    """n < 0, a step below 1 without step_dev, a NULL buffer, and -- the kernel moves four floats at a time -- any of p, g, m, v
    off a 16-byte boundary: refused; the valid neighbours pass"""
    assert _adam(dry, **kw) == _lib.LIREC_EINVAL
    assert _adam(dry) == 0 and _adam(dry, n=0) == 0 and _adam(dry, n=1) == 0
    assert _adam(dry, step=0, step_dev=_addr(6)) == 0                       # (the step is read on the device)
    assert _adam(dry, p=_addr(0) + 16, g=_addr(1) + 48, m=_addr(2) + 16, v=_addr(3) + 32) == 0
    if set(kw) & set('pgmv') and None not in kw.values():
        assert _adam(dry, n=0, **kw) == _lib.LIREC_EINVAL                  # (checked before the n = 0 shortcut)


@pytest.mark.parametrize('kw', [dict(n=0), dict(n=-1), dict(count=None), dict(ticket=None), dict(p=None), dict(g=None),
                                dict(m=None), dict(v=None)] + MISALIGNED,
                         ids=lambda kw: '-'.join('%s_%s' % (k, v if v is None or abs(v) < 99 else 'plus%d' % (v & 15))
                                                 for k, v in kw.items()))
def test_adam_step_counted_argument_checks(dry, kw):
    assert _counted(dry, **kw) == _lib.LIREC_EINVAL
    assert _counted(dry) == 0 and _counted(dry, n=1, advance=0) == 0
    assert _counted(dry, p=_addr(0) + 16, g=_addr(1) + 48, m=_addr(2) + 16, v=_addr(3) + 32) == 0


def test_sizes_are_refused_without_the_dry_run_too():
    """the refusal comes before any device call: no dry run, no GPU"""
    L = _lib.lib()
    assert _adam(L, n=-1) == _lib.LIREC_EINVAL and _counted(L, n=0) == _lib.LIREC_EINVAL


def _incs(*v):
    return (C.c_int64 * max(len(v), 1))(*v)


def test_zero_count_argument_checks(dry):
    L = dry
    ok = lambda **kw: L.lirec_zero_count(kw.get('p', _addr(0)), kw.get('bytes', 4096 + 5), kw.get('ctr', _addr(1)),
                                         kw.get('inc', _incs(1, 2)), kw.get('n', 2), None)
    assert ok() == 0 and ok(n=0, ctr=None, inc=None) == 0 and ok(n=4, inc=_incs(1, 2, 3, 4)) == 0 and ok(bytes=0) == 0
    assert ok(p=None, bytes=0) == 0
    for off in (1, 4, 8, 15):
        assert ok(p=_addr(0) + off) == _lib.LIREC_EINVAL                    # p not 16-byte aligned
    assert ok(p=_addr(0) + 16) == 0
    assert ok(n=5, inc=_incs(1, 2, 3, 4, 5)) == _lib.LIREC_EINVAL
    assert ok(n=-1) == _lib.LIREC_EINVAL
    assert ok(n=1, ctr=None) == _lib.LIREC_EINVAL                           # counters to advance, and none given
    assert ok(n=1, inc=None) == _lib.LIREC_EINVAL
    assert ok(bytes=-1) == _lib.LIREC_EINVAL and ok(p=None) == _lib.LIREC_EINVAL


def test_counter_add_argument_checks(dry):
    L = dry
    assert L.lirec_counter_add(_addr(0), _incs(1), 0, None) == _lib.LIREC_EINVAL
    assert L.lirec_counter_add(_addr(0), _incs(1, 2, 3, 4, 5), 5, None) == _lib.LIREC_EINVAL
    assert L.lirec_counter_add(None, _incs(1), 1, None) == _lib.LIREC_EINVAL
    assert L.lirec_counter_add(_addr(0), None, 1, None) == _lib.LIREC_EINVAL
    for n in (1, 2, 3, 4):
        assert L.lirec_counter_add(_addr(0), _incs(*range(n)), n, None) == 0


def test_memset_zero_argument_checks(dry):
    assert dry.lirec_memset_zero(_addr(0), -1, None) == _lib.LIREC_EINVAL
    assert dry.lirec_memset_zero(None, 16, None) == _lib.LIREC_EINVAL
    assert dry.lirec_memset_zero(None, 0, None) == 0 and dry.lirec_memset_zero(_addr(0) + 3, 17, None) == 0


# -- lirec_fused_adam, reached through lirec_embed_bwd: a plain head on the persistent layer-1 kernels (the only path that takes it)
J, DIMS, ROWS = 256, [256, 512], 33
OFFS = [0, J * DIMS[0]]
BOFFS = [J * sum(DIMS), J * sum(DIMS) + J]
N_FLAT = (J * sum(DIMS) + 2 * J + 63) // 64 * 64 + 64
N_PARAMS = sum(J * d + J for d in DIMS)
G_AT, P_AT, M_AT, V_AT, WQ_AT = _addr(20), _addr(21), _addr(22), _addr(23), _addr(24)


def _fill(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = v


def _head(L, J=J):
    a = _lib.EmbedBwdArgs()
    a.X, a.ldx = _addr(0), sum(DIMS)
    a.H1, a.dZ2, a.lddz2 = _addr(1), _addr(2), 32
    _fill(a.W2, [_addr(3), _addr(4)])
    _fill(a.dW2, [_addr(5), _addr(6)]); _fill(a.db2, [_addr(7), _addr(8)])
    _fill(a.dW1, [G_AT, G_AT + 4 * J * DIMS[0]]); _fill(a.db1, [G_AT + 4 * J * sum(DIMS), G_AT + 4 * (J * sum(DIMS) + J)])
    _fill(a.in_off, [0, DIMS[0]]); _fill(a.in_dim, DIMS); _fill(a.out_dim, [16, 16])
    a.rows, a.nseg, a.J, a.parts = ROWS, 2, J, 4                # (parts 4: the first-layer weight gradient alone)
    a.sel = _lib.RowSel(1, 2, 0)
    a.workspace, a.workspace_bytes = _addr(9), L.lirec_workspace_bytes(ROWS, 2, J)
    a.planes, a.planes_bytes = _addr(10), L.lirec_planes_bytes(ROWS, sum(DIMS), J, 0)
    return a


def _fused(**kw):
    v = dict(p=P_AT, g=G_AT, m=M_AT, v=V_AT, wq=WQ_AT, wq_first=0, n=N_FLAT, n_params=N_PARAMS, step=3, lr=1e-3, beta1=.9,
             beta2=.999, eps=1e-8, weight_decay=1e-5, grad_scale=1.0, step_dev=None)
    v.update(kw)
    return _lib.FusedAdamArgs(*v.values())


def _bwd(L, adam, edit=None, J=J):
    a = _head(L, J)
    if edit:
        edit(a)
    if adam is not None:
        a.adam = C.cast(C.pointer(adam), C.c_void_p)
    return L.lirec_embed_bwd(C.byref(a), None)


@pytest.fixture
def planes_path(dry):
    """gemm mode 2 with a (fake) split-K scratch registered: what the persistent weight-gradient launch asks for"""
    from lirec_amd import ops
    L = dry
    mode = L.lirec_get_gemm_mode()
    assert L.lirec_set_gemm_mode(2) == 0 and L.lirec_set_scratch(_addr(30), 256 << 20) == 0
    try:
        yield L
    finally:
        assert L.lirec_set_scratch(None, 0) == 0 and L.lirec_set_gemm_mode(mode) == 0
        ops._scratch.pop(ops._ctx_key(), None)


def _dw1(i, at):
    def f(a):
        a.dW1[i] = at
    return f


def _db1(i, at):
    def f(a):
        a.db1[i] = at
    return f


FUSED_BREAKS = {
    'p_not_16_byte_aligned': (dict(p=P_AT + 4), None),
    'g_not_16_byte_aligned': (dict(g=G_AT + 8), None),
    'm_not_16_byte_aligned': (dict(m=M_AT + 12), None),
    'v_not_16_byte_aligned': (dict(v=V_AT + 4), None),
    'dW1_below_g': (dict(), _dw1(0, G_AT - 4 * J * DIMS[0])),
    'dW1_behind_g_plus_n': (dict(), _dw1(1, G_AT + 4 * N_FLAT)),
    'dW1_ends_behind_g_plus_n': (dict(n=OFFS[1] + J * DIMS[1] - 4), None),
    'dW1_not_a_multiple_of_4_elements_into_g': (dict(), _dw1(1, G_AT + 4 * (OFFS[1] + 2))),
    'db1_behind_g_plus_n': (dict(), _db1(1, G_AT + 4 * (N_FLAT - J + 1))),
    'n_params_one_more': (dict(n_params=N_PARAMS + 1), None),
    'n_params_one_less': (dict(n_params=N_PARAMS - 1), None),
    'wq_not_256_byte_aligned': (dict(wq=WQ_AT + 16), None),
    'wq_first_behind_a_W1': (dict(wq_first=64), None),
    'W1_shadow_not_256_byte_aligned': (dict(), _dw1(1, G_AT + 4 * (OFFS[1] + 4))),
    'no_step': (dict(step=0), None),
    'n_0': (dict(n=0), None),
    'no_m': (dict(m=None), None),
}
FUSED_OK = {
    'as_is': (dict(), None),
    'without_shadow': (dict(wq=None), None),
    'without_shadow_W1_anywhere_4_aligned': (dict(wq=None, n=N_FLAT + 64), _dw1(1, G_AT + 4 * (OFFS[1] + 4))),
    'step_on_the_device': (dict(step=0, step_dev=_addr(31)), None),
    'buffers_16_byte_aligned': (dict(p=P_AT + 16, m=M_AT + 48, v=V_AT + 32), None),
    'n_exact': (dict(n=BOFFS[1] + J), None),
}


@pytest.mark.parametrize('what', sorted(FUSED_BREAKS))
def test_fused_adam_argument_checks(planes_path, what):
    kw, edit = FUSED_BREAKS[what]
    assert _bwd(planes_path, _fused(**kw), edit) == _lib.LIREC_EINVAL
    assert _bwd(planes_path, None, edit) == 0                    # (the head itself is fine: the update is what is refused)


@pytest.mark.parametrize('what', sorted(FUSED_OK))
def test_fused_adam_arguments_accepted(planes_path, what):
    """the valid neighbours of every break pass, so each break is refused for its own reason"""
    kw, edit = FUSED_OK[what]
    assert _bwd(planes_path, _fused(**kw), edit) == 0


def test_fused_adam_is_refused_on_heads_the_persistent_kernels_decline(planes_path):
    """The fused update exists on the persistent kernels only, which want J and in_dim in multiples of 256: a head with another J is
    refused with the update, with or without a shadow, and runs without it (on the on-the-fly core).  So fused_adam_fill's own
    check that a shadowed W1 has rows and columns in multiples of 32 cannot be reached through lirec_embed_bwd, and nothing here
    would notice its removal."""
    L = planes_path
    for j in (48, 272):
        assert _bwd(L, _fused(n=2 * N_FLAT, n_params=sum(j * d + j for d in DIMS)), J=j) == _lib.LIREC_EINVAL
        assert _bwd(L, _fused(n=2 * N_FLAT, n_params=sum(j * d + j for d in DIMS), wq=None), J=j) == _lib.LIREC_EINVAL
        assert _bwd(L, None, J=j) == 0
    # ... and the fused update off the persistent path (mode 0) or on a head that is not its own launch is refused as well
    assert L.lirec_set_gemm_mode(0) == 0
    assert _bwd(L, _fused()) == _lib.LIREC_EINVAL and _bwd(L, None) == 0
    assert L.lirec_set_gemm_mode(2) == 0
