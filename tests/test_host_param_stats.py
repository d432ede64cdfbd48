"""Per-parameter statistics without a GPU (lirec_param_stats, FusedAdam.param_stats(); include/lirec_hip.h, "per-range gradient,
weight and update statistics"): the exports, the struct and the ABI number; every refusal of the C call under the library's
host-side dry run; the float64 yardstick (tests/param_stats_cases.py) on hand-made inputs; and, through the real host stack in the
dry run (tests/param_stats_dryrun.py), what ``training()`` issues under ``opt.param_stats_every`` and what the optimiser refuses."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import param_stats_cases as PC
from lirec_amd import _lib
from lirec_amd.optim import FusedAdam, ParamStat, ParamStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304
EINVAL = _lib.LIREC_EINVAL
P, G, M, V, OUT, WS = (0x20000000 + 0x4000000 * i for i in range(6))      # fake, aligned, never dereferenced device addresses


@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def _entries(rows):
    arr = (_lib.ParamStatEntry * max(len(rows), 1))()
    for a, r in zip(arr, rows):
        a.offset, a.length, a.flags, a.inv_bc1, a.inv_sqrt_bc2, a.eps = r
    return arr


GOOD = (3, 1000, 7, 1.5, 2.5, 1e-8)


def _call(L, rows=(GOOD,), n=None, p=P, g=G, m=M, v=V, out=OUT, ws=WS, ws_bytes=None):
    n = len(rows) if n is None else n
    if ws_bytes is None:
        ws_bytes = max(L.lirec_param_stats_ws_bytes(min(max(n, 1), 64)), 0)
    return L.lirec_param_stats(p, g, m, v, _entries(rows), n, out, ws, ws_bytes, None)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_exports_struct_and_abi_number():
    L = _lib.lib()
    assert 'lirec_param_stats' in _lib.EXPORTS and 'lirec_param_stats_ws_bytes' in _lib.EXPORTS
    assert hasattr(L, 'lirec_param_stats') and hasattr(L, 'lirec_param_stats_ws_bytes')
    assert L.lirec_abi_sizeof(43) == C.sizeof(_lib.ParamStatEntry) == 32
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert _lib.PARAM_STATS_COLS == PC.COLS == 9 and _lib.PARAM_STATS_MAX_RANGES == 64
    assert (_lib.STAT_GRAD, _lib.STAT_PARAM, _lib.STAT_UPDATE) == (PC.GRAD, PC.PARAM, PC.UPDATE) == (1, 2, 4)
    # the workspace: a whole number of doubles per range, growing with the table; no answer outside 1..64
    sizes = [L.lirec_param_stats_ws_bytes(n) for n in range(1, 65)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[1] == 2 * sizes[0]
    assert L.lirec_param_stats_ws_bytes(0) == -1 and L.lirec_param_stats_ws_bytes(65) == -1 and L.lirec_param_stats_ws_bytes(-3) == -1
    assert 'param_stats' in {L.lirec_profile_site_name(s).decode() for s in range(L.lirec_profile_sites())}


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the refusals, in the dry run
# ---------------------------------------------------------------------------------------------------------------------------
def test_well_formed_calls_are_accepted(dry):
    L = dry
    assert _call(L) == 0
    assert _call(L, [GOOD] * 64) == 0 and _call(L, [GOOD] * 63) == 0
    assert _call(L, [(0, 0, 7, 1.0, 1.0, 0.0)]) == 0                        # a length of 0 is legal
    assert _call(L, [(5, 10, 0, 1.0, 1.0, 0.0)], p=None, g=None, m=None, v=None) == 0      # nothing asked for: no buffer needed
    assert _call(L, [(5, 10, 1, 1.0, 1.0, 0.0)], p=None, m=None, v=None) == 0             # only the buffers of the flags
    assert _call(L, [(5, 10, 2, 1.0, 1.0, 0.0)], g=None, m=None, v=None) == 0
    assert _call(L, [(5, 10, 4, 1.0, 1.0, 0.0)], p=None, g=None) == 0
    assert _call(L, [(5, 10, 7, -1.0, 0.0, 0.0)]) == 0                      # the factors: any finite value
    assert _call(L, [(2 ** 40, 2 ** 40, 7, 1.0, 1.0, 1e-8)]) == 0           # offsets are 64-bit
    # buffers off a 16-byte boundary, by the same amount or not: accepted (the scalar loads)
    assert _call(L, p=P + 4, g=G + 4, m=M + 4, v=V + 4) == 0
    assert _call(L, p=P + 4, g=G + 8, m=M, v=V + 12) == 0
    assert _call(L, ws_bytes=L.lirec_param_stats_ws_bytes(1) + 8) == 0


def test_every_refusal(dry):
    L = dry
    need = L.lirec_param_stats_ws_bytes(1)
    nan, inf = math.nan, math.inf
    bad_calls = {
        'n_ranges 0': dict(n=0), 'n_ranges -1': dict(n=-1), 'n_ranges 65': dict(rows=[GOOD] * 65, ws_bytes=1 << 30),
        'negative offset': dict(rows=[(-1, 10, 7, 1.0, 1.0, 0.0)]), 'negative length': dict(rows=[(0, -1, 7, 1.0, 1.0, 0.0)]),
        'an end that wraps': dict(rows=[(2 ** 62, 2 ** 62 + 2 ** 61, 2, 1.0, 1.0, 0.0), (2 ** 62, 2 ** 62, 2, 1.0, 1.0, 0.0)]),
        'out NULL': dict(out=None), 'out misaligned': dict(out=OUT + 4), 'ws NULL': dict(ws=None), 'ws misaligned': dict(ws=WS + 4),
        'ws too small': dict(ws_bytes=need - 1), 'ws of no bytes': dict(ws_bytes=0), 'ws sized for fewer ranges': dict(rows=[GOOD] * 2, ws_bytes=need),
        'gradient flag without g': dict(g=None), 'parameter flag without p': dict(p=None), 'update flag without m': dict(m=None),
        'update flag without v': dict(v=None), 'flags 8': dict(rows=[(0, 10, 8, 1.0, 1.0, 0.0)]), 'flags -1': dict(rows=[(0, 10, -1, 1.0, 1.0, 0.0)]),
        'eps NaN': dict(rows=[(0, 10, 7, 1.0, 1.0, nan)]), 'eps Inf': dict(rows=[(0, 10, 7, 1.0, 1.0, inf)]),
        'eps negative': dict(rows=[(0, 10, 7, 1.0, 1.0, -1e-8)]), 'inv_bc1 NaN': dict(rows=[(0, 10, 7, nan, 1.0, 0.0)]),
        'inv_bc1 Inf': dict(rows=[(0, 10, 7, inf, 1.0, 0.0)]), 'inv_sqrt_bc2 NaN': dict(rows=[(0, 10, 7, 1.0, nan, 0.0)]),
        'inv_sqrt_bc2 -Inf': dict(rows=[(0, 10, 7, 1.0, -inf, 0.0)]),
        'the second entry bad': dict(rows=[GOOD, (0, 10, 9, 1.0, 1.0, 0.0)]),
        'a pointer off 4 bytes': dict(g=G + 2),
    }
    for what, kw in bad_calls.items():
        assert _call(L, **kw) == EINVAL, what
    assert L.lirec_param_stats(P, G, M, V, None, 1, OUT, WS, need, None) == EINVAL      # entries NULL
    # the checks come before anything is issued: a refused call records nothing, an accepted one its two launches
    assert L.lirec_record_begin() == 0
    try:
        assert _call(L, out=None) == EINVAL and L.lirec_record_mark() == 0
        assert _call(L) == 0
        mid = L.lirec_record_mark()
        assert _call(L, [(7, 0, 7, 1.0, 1.0, 0.0)]) == 0                 # nothing but empty ranges: the launch that writes the zeros
    finally:
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0
    kinds = []
    for i in range(L.lirec_cmdlist_size(h)):
        s, k = C.c_void_p(), C.c_int32()
        assert L.lirec_cmdlist_command(h, i, C.byref(s), C.byref(k)) == 0
        kinds.append(k.value)
    assert kinds[:mid].count(0) == 2 and kinds[mid:].count(0) == 1 and kinds.count(2) == 4      # (launches; the profile site's brackets)
    assert L.lirec_cmdlist_replay(h, 0, -1) == 0 and L.lirec_cmdlist_destroy(h) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the yardstick on hand-made inputs
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_on_special_values():
    """a NaN, +Inf, -Inf, -0, a denormal and FLT_MAX in one range: three are counted and stay out of the sum and the maximum; FLT_MAX
    squared is finite in float64 and IS summed; -0 and the denormal are ordinary values"""
    x = np.array([np.nan, np.inf, -np.inf, -0.0, PC.DENORMAL, PC.FLT_MAX], np.float32)
    z = np.zeros(6, np.float32)
    got = PC.row(x, x, z, z, (0, 6, 3))
    want_sum = PC.FLT_MAX ** 2 + PC.DENORMAL ** 2          # (rounds to FLT_MAX^2: the denormal's square is 2^-282 of it)
    assert math.isfinite(want_sum) and want_sum == PC.FLT_MAX ** 2
    assert got == [want_sum, PC.FLT_MAX, 3.0, want_sum, PC.FLT_MAX, 3.0, 0.0, 0.0, 0.0]
    assert PC.row(x, x, z, z, (3, 2, 1))[:3] == [PC.DENORMAL ** 2, PC.DENORMAL, 0.0] and PC.DENORMAL ** 2 > 0.0
    assert PC.row(x, x, z, z, (0, 3, 2))[3:6] == [0.0, 0.0, 3.0]                       # nothing finite: sum and maximum 0
    assert PC.row(x, x, z, z, (2, 0, 7)) == [0.0] * 9                                 # an empty range
    # fsum is exact where a running float64 sum is not
    y = np.array([2.0 ** 27] + [1.0] * 4, np.float32)
    assert PC.row(y, y, z, z, (0, 5, 1))[0] == 2.0 ** 54 + 4.0
    run = 0.0
    for t in [2.0 ** 54] + [1.0] * 4:
        run += t
    assert run == 2.0 ** 54                                                          # (what the bound n u allows for)


def test_restatement_of_the_update_columns():
    m = np.array([3.0, -4.0, 0.0, np.nan, 1.0, 1.0, np.inf, 2.0], np.float32)
    v = np.array([4.0, 16.0, 0.0, 1.0, -1.0, np.nan, 1.0, np.inf], np.float32)
    # u = (m 2) / (sqrt(v) 0.5 + 0.5): 6 / 1.5, -8 / 2.5, 0 / 0.5, NaN, NaN (negative v), NaN, Inf, 4 / Inf = 0
    got = PC.row(m, m, m, v, (0, 8, 4, 2.0, 0.5, 0.5))
    assert got[:6] == [0.0] * 6
    assert got[6] == pytest.approx(16.0 + 10.24, rel=1e-15) and got[7] == 4.0 and got[8] == 4.0
    assert PC.row(m, m, m, v, (2, 1, 4, 1.0, 1.0, 0.0))[6:] == [0.0, 0.0, 1.0]         # 0 / 0 with eps = 0: counted
    # the float64 and the long double evaluation agree to float64's precision, and the hi + lo split is exact
    p, g, mm, vv = PC.buffers(4097, 11)
    u64 = PC.update_direction(mm, vv, *PC.FACTORS)
    ul = PC.update_direction(mm, vv, *PC.FACTORS, dtype=PC.LD)
    assert np.isfinite(u64).all() and (np.abs(u64 - ul.astype(np.float64)) <= 5 * PC.U * np.abs(u64)).all()
    r = PC.row(p, g, mm, vv, (0, 4097, 7) + PC.FACTORS)
    assert abs(r[6] - float(np.sum(u64 * u64))) <= (4097 + 16) * PC.U * r[6]
    # FusedAdam's factors are the fp32 roundings of the double expressions
    f = FusedAdam.stat_factors(3, 0.9, 0.999)
    assert f == (float(np.float32(PC.FACTORS[0])), float(np.float32(PC.FACTORS[1])))
    assert FusedAdam.stat_factors(0, 0.9, 0.999) == FusedAdam.stat_factors(1, 0.9, 0.999)


def test_the_check_itself_catches_what_it_should():
    p, g, m, v = PC.buffers(1025, 5)
    ent = [(3, 1000, 7) + PC.FACTORS, (1003, 22, 2) + PC.FACTORS]
    want = PC.reference(p, g, m, v, ent)
    assert PC.check(want.copy(), want, ent) == 0.0
    for r, c, delta in ((0, 0, 1e-12), (0, 1, 1e-30), (0, 2, 1.0), (0, 6, 1e-12), (1, 0, 1e-300), (1, 6, 1.0)):
        bad = want.copy()
        bad[r, c] = np.nextafter(bad[r, c], np.inf) if c % 3 == 1 else bad[r, c] * (1 + delta) + (delta if bad[r, c] == 0 else 0)
        with pytest.raises(AssertionError):
            PC.check(bad, want, ent)
    near = want.copy()
    near[0, 0] *= 1 + 500 * PC.U                 # inside n u = 1000 u
    assert 0.4 < PC.check(near, want, ent) <= 1.0


def test_crossed_entries_cover_the_lengths_and_offsets():
    ent, extent = PC.crossed_entries()
    assert len(ent) == 48 and {e[1] for e in ent} == set(PC.LENGTHS)
    assert {(e[1], e[0] % 4) for e in ent} == {(n, r) for n in PC.LENGTHS for r in range(4)}
    ends = [e[0] + e[1] for e in ent]
    gaps = [b[0] - a for a, b in zip(ends, ent[1:])]
    assert min(gaps) == 0 and max(gaps) > 0 and all(x >= 0 for x in gaps) and extent == ends[-1] <= 300000


def test_host_of_a_table():
    """ParamStats.host(): roots, scales, None for what was not asked for, the ratio"""
    import torch
    t = torch.tensor([[4.0, 1.5, 2.0, 9.0, 2.0, 0.0, 16.0, 3.0, 1.0], [0.0] * 3 + [0.0, 0.0, 0.0] + [0.0] * 3,
                      [1.0, 1.0, 0.0, 25.0, 4.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    h = ParamStats(['a', 'b', 'c'], t, [7, 2, 3], 0.5, [0.1, 0.1, 0.2]).host()
    assert list(h) == ['a', 'b', 'c'] and isinstance(h['a'], ParamStat)
    assert h['a'] == ParamStat(1.0, 0.75, 2, 3.0, 2.0, 0, pytest.approx(0.4), pytest.approx(0.3), 1, pytest.approx(0.4 / 3.0))
    assert h['b'] == ParamStat(None, None, None, 0.0, 0.0, 0, None, None, None, None)
    assert h['c'] == ParamStat(0.5, 0.5, 0, 5.0, 4.0, 0, None, None, None, None)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. / 5. training() and the optimiser's refusals, through the host stack in the dry run
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['wiring', 'refusals'])
def test_the_host_stack_in_the_dry_run(what):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'param_stats_dryrun.py'), what], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and what + ' ok' in r.stdout, r.stdout[-4000:]
