"""lirec_adam_step_ranges alone, on guarded buffers: one launch over a table of ranges (offset, length, lag) of the flat buffers,
range r updated with step t - lag[r] -- t by value, from `step_dev`, or from the count_dev / ticket / advance triple of
lirec_adam_step_counted.

Yardsticks (tests/adam_cases.py): every updated element equals ref32 -- the update operation by operation in fp32 -- with the
range's OWN step, bit for bit, and lies within the bounds of ref64; everything between and around the ranges keeps its bits, the
moments included; a one-range, zero-lag table gives the bits of lirec_adam_step.  Range lengths 1, 3, 4, 5 (the float4 body and the
scalar tail on their own), 1023, 1024, 1025 (around one block of 1024 elements) and adam_cases.N_BIG (4 197 379 elements: 4100
blocks dealt to 2048 workgroups -- the loop over blocks goes round a third time -- and a tail of three); tables of 1, 2 and 64
ranges; lags 0 and 2.  The global step is 3 (ranges at steps 3 and 1, the moments zero or not) and, by value, 1000."""
import numpy as np
import pytest
import torch

import adam_cases as AC
from lirec_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _layout(lengths, lags, gap=8):
    """ranges [(offset, length, lag)] behind a guard, each start a multiple of 4, `gap` (+ padding) elements nobody owns between two"""
    rs, at = [], GUARD
    for n, lag in zip(lengths, lags):
        rs.append((at, n, lag))
        at = (at + n + gap + 3) // 4 * 4
    return rs, at + GUARD


TABLES = {
    'one_1': ([1], [0]), 'one_3_lag': ([3], [2]), 'one_4': ([4], [0]), 'one_5_lag': ([5], [2]), 'one_1023': ([1023], [0]),
    'one_1024_lag': ([1024], [2]), 'one_1025': ([1025], [0]),
    'two': ([1025, 3], [2, 0]),
    'seven': (LENGTHS, [0, 2, 0, 2, 2, 0, 2]),
    'sixty_four': ([LENGTHS[i % 7] for i in range(64)], [2 * ((i // 3) % 2) for i in range(64)]),
    'one_big_lag': ([AC.N_BIG], [2]),
    'two_big': ([AC.N_BIG, 1025], [0, 2]),
}


class State:
    def __init__(self, case, total):
        self.np = AC.make_state(case, total)
        # (a state as after a few steps everywhere -- also where this step is a range's first: its moments then simply are not zero)
        self.p, self.g, self.m, self.v = (torch.from_numpy(a).to(DEV) for a in self.np)
        self.p0, self.g0, self.m0, self.v0 = (t.clone() for t in (self.p, self.g, self.m, self.v))

    def check(self, rs, t, hyper, what, bitwise=True):
        torch.cuda.synchronize()
        inside = torch.zeros(self.p.numel(), dtype=torch.bool, device=DEV)
        worst = [0.0, 0.0, 0.0]
        for a, n, lag in rs:
            inside[a:a + n] = True
            got = [x[a:a + n] for x in (self.p, self.m, self.v)]
            use = AC.use_of_bounds(got, *(x[a:a + n] for x in (self.p0, self.g0, self.m0, self.v0)), t - lag, hyper)
            worst = [max(x, y) for x, y in zip(worst, use)]
            assert max(use) <= 1.0, (what, (a, n, lag), use)
            want = AC.ref32(*(x[a:a + n] for x in self.np), t - lag, hyper)
            d = [int((_bits(x) != w.view(np.uint32)).sum()) for x, w in zip(got, want)]
            if bitwise:
                assert d == [0, 0, 0], (what, (a, n, lag), 'elements whose bits differ from ref32 at step %d (p, m, v)' % (t - lag), d)
        print('FROZEN-ADAM-FIGURE %s ranges=%d use_of_bounds p=%.3f m=%.3f v=%.3f' % (what, len(rs), *worst))
        for x, x0, nm in zip((self.p, self.m, self.v), (self.p0, self.m0, self.v0), 'pmv'):
            assert torch.equal(x[~inside], x0[~inside]), '%s: %s written outside the ranges' % (what, nm)
            assert bool((x[inside] != x0[inside]).any())
        assert torch.equal(self.g, self.g0), 'the gradient was written'


@pytest.mark.parametrize('table,t', [(k, 3) for k in sorted(TABLES)] + [('seven', 1000), ('two_big', 1000)])
def test_ranges_by_value_are_the_fp32_restatement_at_each_ranges_own_step(table, t):
    c = AC.Case(0, 3, 1.0) if t == 3 else AC.Case(2, 1000, 1e-12)
    h = AC.hyper32(c.hyper)
    rs, total = _layout(*TABLES[table])
    s = State(c, total)
    ops.adam_step_ranges(s.p, s.g, s.m, s.v, rs, t, *h)
    s.check(rs, t, h, 'value-%s-t%d' % (table, t))


@pytest.mark.parametrize('form', ['step_dev', 'counted'])
@pytest.mark.parametrize('table', ['one_5_lag', 'two', 'seven', 'sixty_four', 'two_big'])
def test_ranges_with_the_step_on_the_device(table, form):
    """the step from `step_dev` (the by-value one is then ignored), and from a counter of completed steps (+ 1): the same checks,
    the two bias corrections now computed by the kernel, per range, in double"""
    c = AC.Case(0, 3, 1.0)
    h = AC.hyper32(c.hyper)
    t = 3
    rs, total = _layout(*TABLES[table])
    s = State(c, total)
    if form == 'step_dev':
        sd = torch.tensor([t], dtype=torch.int64, device=DEV)
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, rs, 77, *h, step_dev=sd)
        s.check(rs, t, h, 'step_dev-' + table)
        assert int(sd) == t
    else:
        count = torch.tensor([t - 1], dtype=torch.int64, device=DEV)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, rs, 0, *h, count_dev=count, ticket=ticket, advance=True)
        s.check(rs, t, h, 'counted-' + table)
        assert int(count) == t and int(ticket) == 0


def test_counted_chain_advances_once_and_leaves_the_ticket_at_zero():
    """As tests/test_gpu_optim.py pins lirec_adam_step_counted: a chain of calls over disjoint tables, `advance` on the last one
    only -- all take step k + 1, the counter reads k until the last call has run and k + 1 after it, the ticket is 0 after every
    call; the next chain takes k + 2; with advance = 0 throughout the counter stays.  Mixed with the plain counted call."""
    c = AC.Case(0, 3, 1.0)
    h = AC.hyper32(c.hyper)
    k = 2
    rs, total = _layout(*TABLES['seven'])
    got, want = State(c, total), State(c, total)
    count = torch.tensor([k], dtype=torch.int64, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    parts = [rs[:3], rs[3:6]]
    last = rs[6]

    def chain(advance_last, step):
        for i, part in enumerate(parts):
            ops.adam_step_ranges(got.p, got.g, got.m, got.v, part, 0, *h, count_dev=count, ticket=ticket, advance=False)
            torch.cuda.synchronize()
            assert int(ticket) == 0 and int(count) == step - 1, (i, int(ticket), int(count))
        a, n, lag = last                              # the plain counted call closes the chain (its range has step k + 1 itself)
        ops.adam_step_ranges(got.p, got.g, got.m, got.v, [(a, n, 0)], 0, *h, count_dev=count, ticket=ticket, advance=advance_last)
        torch.cuda.synchronize()
        assert int(ticket) == 0 and int(count) == step - 1 + (1 if advance_last else 0)
        sd = torch.tensor([step], dtype=torch.int64, device=DEV)
        ops.adam_step_ranges(want.p, want.g, want.m, want.v, rs[:6] + [(a, n, 0)], 0, *h, step_dev=sd)
        torch.cuda.synchronize()
        for x, y, nm in zip((got.p, got.m, got.v), (want.p, want.m, want.v), 'pmv'):
            assert torch.equal(x, y), (nm, 'the counted chain differs from step_dev = %d' % step)

    chain(True, k + 1)
    chain(True, k + 2)
    chain(False, k + 3)
    assert int(count) == k + 2 and int(ticket) == 0
    # ... and the plain counted call reads the same counter
    a, n, _ = rs[4]
    x = State(c, total)
    ops.adam_step_counted(x.p[a:a + n], x.g[a:a + n], x.m[a:a + n], x.v[a:a + n], *h, count, ticket, advance=True)
    y = State(c, total)
    ops.adam_step_ranges(y.p, y.g, y.m, y.v, [(a, n, 0)], 0, *h, step_dev=torch.tensor([k + 3], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert int(count) == k + 3 and all(torch.equal(p, q) for p, q in zip((x.p, x.m, x.v), (y.p, y.m, y.v)))


@pytest.mark.parametrize('n', LENGTHS + [AC.N_BIG])
def test_one_zero_lag_range_gives_the_bits_of_adam_step(n):
    c = AC.Case(0, 3, 1.0) if n < AC.N_BIG else AC.Case(3, 100000, 1e3)
    h = AC.hyper32(c.hyper)
    rs, total = _layout([n], [0])
    a = rs[0][0]
    x, y = State(c, total), State(c, total)
    ops.adam_step_ranges(x.p, x.g, x.m, x.v, rs, c.step, *h)
    ops.adam_step(y.p[a:a + n], y.g[a:a + n], y.m[a:a + n], y.v[a:a + n], c.step, *h)
    torch.cuda.synchronize()
    for p, q, nm in zip((x.p, x.m, x.v), (y.p, y.m, y.v), 'pmv'):
        assert torch.equal(p, q), nm
    x.check(rs, c.step, h, 'one-range-%d' % n)
    # the same from a sub-view whose base is another multiple of 16 bytes: offsets count from the pointers given
    z = State(c, total)
    ops.adam_step_ranges(z.p[4:], z.g[4:], z.m[4:], z.v[4:], [(a - 4, n, 0)], c.step, *h)
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip((x.p, x.m, x.v), (z.p, z.m, z.v)))


def test_an_empty_table_and_empty_ranges_launch_nothing():
    c = AC.Case(0, 3, 1.0)
    h = AC.hyper32(c.hyper)
    s = State(c, 4096)
    count = torch.tensor([5], dtype=torch.int64, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.profile_enable(True)
    try:
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, [], 3, *h)
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, [(64, 0, 0), (128, 0, 1)], 3, *h)
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, [], 0, *h, count_dev=count, ticket=ticket, advance=True)
        torch.cuda.synchronize()
        assert 'adam' not in ops.profile_read()
    finally:
        ops.profile_enable(False)
    assert int(count) == 5 and all(torch.equal(a, b) for a, b in zip((s.p, s.m, s.v), (s.p0, s.m0, s.v0)))
