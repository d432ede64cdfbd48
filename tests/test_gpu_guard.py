"""Skipping non-finite steps on the device (include/lirec_hip.h, "skipping non-finite steps"; lirec_amd/optim.py): the guard
finalize against lirec_clip_finalize and against the values themselves, the guarded Adam launches against the clipped ones bit
for bit, and FusedAdam(skip_nonfinite=True) on its eager and recorded routes.

Bounds.  The guarded launch IS the clipped launch with step_dev holding t - S (zero differing elements are asserted), and is held
to adam_cases.bounds with that step and the scale gs * coef like the clipped one (tests/test_host_clip.py shows the fp32
restatement inside them for these coefficients).  A skipped step changes no bit.  The decision itself has no tolerance: the flag
is 1 exactly when an element of the ranges is NaN or +-Inf (guard_cases.must_skip).

Measured on an MI355X.  Guarded launches: 0 elements differing from the clipped launch in every kind, size and S; worst use of a
bound 0.18 (n = 5) and 0.31 (n = 1023), the same for all four calls.  FusedAdam end to end (18 431 616 elements, all eight
variants): worst use of a bound 0.31 (p) / 0.07 (m) / 0.29 (v), the skipped step changing no bit; the frozen-accounting script's
last update 0.27 / 0.07 / 0.28.  Recorded against eager with a NaN feature during step 3: everything bit for bit, the loss of the
poisoned step finite (a hinge keeps no NaN) while its gradients are not.
"""
import math

import numpy as np
import pytest
import torch

import adam_cases as AC
import adamw_cases as WC
import clip_cases as CC
import guard_cases as GC
import test_gpu_clip as TC
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
P = _lib.CLIP_PARTIALS
PAD = 64
CANARY = 1e30


def _fig(what, **kw):
    print('GUARD-FIGURE %s %s' % (what, ' '.join('%s=%s' % (k, ('%.4g' % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the guard finalize
# ---------------------------------------------------------------------------------------------------------------------------
class Block:
    """out[3] and the counter, each between canary words"""

    def __init__(self, skipped=0):
        self.obuf = torch.full((8 + 4 + 8,), CANARY, dtype=torch.float32, device=DEV)
        self.out = self.obuf[8:12]
        self.cbuf = torch.full((3,), -7, dtype=torch.int64, device=DEV)
        self.cbuf[1] = skipped
        self.skipped = self.cbuf[1:2]

    def check(self):
        o = self.obuf.cpu().numpy()
        assert (o[:8] == np.float32(CANARY)).all() and (o[11:] == np.float32(CANARY)).all(), 'written around out[0:3]'
        c = self.cbuf.cpu().tolist()
        assert c[0] == -7 and c[2] == -7, 'written around the counter'
        return o[8:11].copy(), c[1]


def _partials_of(values, tables):
    """[partials after each table] of the values, with the gaps of the tables holding CANARY"""
    buf, g = TC._guarded(values)
    out = []
    for t in tables:
        part = torch.zeros(P, dtype=torch.float64, device=DEV)
        ops.grad_sq_partials(g, t, part)
        out.append(part)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('gs', [1.0, 0.5])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_guard_finalize_on_finite_input_is_clip_finalize(mode, gs):
    vals = np.random.default_rng(5 + mode).standard_normal(1025).astype(np.float32)
    part, = _partials_of(vals, [[(0, 1025)]])
    for mn in (1.0, 1e9, 7.0):
        sq_a = torch.tensor([12.5], dtype=torch.float64, device=DEV)
        sq_b = sq_a.clone()
        want = torch.full((2,), float('nan'), dtype=torch.float32, device=DEV)
        ops.clip_finalize(part, sq_a, mode, gs, mn, want)
        for count in (False, True):
            blk = Block(skipped=3)
            sq_b.fill_(12.5)
            ops.clip_finalize_guard(part, sq_b, mode, gs, mn, blk.out, blk.skipped, count)
            torch.cuda.synchronize()
            out, skipped = blk.check()
            assert (out[:2].view(np.uint32) == _bits(want)).all(), (mode, gs, mn, out, want)
            assert out[2] == 0.0 and skipped == 3
            assert torch.equal(sq_a.view(torch.int64), sq_b.view(torch.int64))
    # max_norm 0: no clipping -- the coefficient is 1 whatever the norm, the norm as ever
    blk = Block()
    sq = torch.tensor([12.5], dtype=torch.float64, device=DEV)
    ops.clip_finalize_guard(part, sq, mode, gs, 0.0, blk.out, None, False)
    torch.cuda.synchronize()
    out, _ = blk.check()
    assert out[0] == 1.0 and out[2] == 0.0 and out[1] == np.float32(math.sqrt(float(sq)) * gs)
    assert out[1] > 1.0                                         # (a bound of 1 would have clipped)


@pytest.mark.parametrize('n', GC.SIZES)
@pytest.mark.parametrize('bad', sorted(GC.BAD))
def test_guard_finalize_flags_one_non_finite_element(bad, n):
    for at in GC.positions(n):
        vals = np.random.default_rng(n + at).standard_normal(n).astype(np.float32)
        vals[at] = GC.BAD[bad]
        assert GC.must_skip(vals, [(0, n)])
        part, = _partials_of(vals, [[(0, n)]])
        for count, start in ((True, 0), (True, 5), (False, 5)):
            blk = Block(skipped=start)
            sq = torch.zeros(1, dtype=torch.float64, device=DEV)
            ops.clip_finalize_guard(part, sq, 0, 1.0, 1.0, blk.out, blk.skipped, count)
            torch.cuda.synchronize()
            out, skipped = blk.check()
            assert out[2] == 1.0, (bad, n, at, out)
            assert skipped == start + (1 if count else 0), (bad, n, at, count, skipped)
            assert not math.isfinite(float(sq))


@pytest.mark.parametrize('bad', sorted(GC.BAD))
def test_guard_finalize_over_a_table_of_ranges(bad):
    """the element in the SECOND range of a table (mode 1 adds it to a finite first sum, mode 2 takes the sum as it stands); a
    non-finite value in the gap between the ranges, or behind them, is nobody's"""
    L = 2100
    ranges = [(0, 1030), (1040, 1027)]
    vals = np.random.default_rng(17).standard_normal(L).astype(np.float32)
    vals[1030:1040] = GC.BAD[bad]                               # the gap
    vals[2067:] = GC.BAD[bad]
    assert not GC.must_skip(vals, ranges)
    first, second = _partials_of(vals, [[ranges[0]], [ranges[1]]])
    blk, sq = Block(), torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.clip_finalize_guard(first, sq, 0, 1.0, 1.0, blk.out, blk.skipped, False)
    ops.clip_finalize_guard(second, sq, 1, 1.0, 1.0, blk.out, blk.skipped, False)
    ops.clip_finalize_guard(None, sq, 2, 1.0, 1.0, blk.out, blk.skipped, True)
    torch.cuda.synchronize()
    assert blk.check()[0][2] == 0.0 and blk.check()[1] == 0 and math.isfinite(float(sq))
    for at in (1040, 1040 + 1026):                              # f32x4 body / scalar tail of the second range
        v2 = vals.copy()
        v2[at] = GC.BAD[bad]
        assert GC.must_skip(v2, ranges)
        first, second = _partials_of(v2, [[ranges[0]], [ranges[1]]])
        both, = _partials_of(v2, [ranges])
        blk, sq = Block(), torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.clip_finalize_guard(first, sq, 0, 1.0, 1.0, blk.out, blk.skipped, False)
        torch.cuda.synchronize()
        assert blk.check()[0][2] == 0.0
        ops.clip_finalize_guard(second, sq, 1, 1.0, 1.0, blk.out, blk.skipped, False)
        torch.cuda.synchronize()
        assert blk.check()[0][2] == 1.0 and blk.check()[1] == 0
        ops.clip_finalize_guard(None, sq, 2, 1.0, 1.0, blk.out, blk.skipped, True)        # (the one that counts)
        torch.cuda.synchronize()
        assert blk.check()[0][2] == 1.0 and blk.check()[1] == 1
        blk2, sq2 = Block(), torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.clip_finalize_guard(both, sq2, 0, 1.0, 1.0, blk2.out, blk2.skipped, True)     # one table with both ranges
        torch.cuda.synchronize()
        assert blk2.check()[0][2] == 1.0 and blk2.check()[1] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the guarded launches
# ---------------------------------------------------------------------------------------------------------------------------
class State:
    """p, g, m, v as 16-byte aligned slices of buffers whose other elements are CANARY"""

    def __init__(self, state):
        self.bufs, self.t = [], []
        for a in state:
            buf = torch.full((PAD + len(a) + PAD + 3,), CANARY, dtype=torch.float32, device=DEV)
            buf[PAD:PAD + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
            self.bufs.append(buf)
            self.t.append(buf[PAD:PAD + len(a)])
        self.p, self.g, self.m, self.v = self.t
        self.n = len(state[0])

    def result(self):
        return self.p, self.m, self.v

    def canaries_ok(self):
        return all(bool((b[:PAD] == CANARY).all()) and bool((b[PAD + self.n:] == CANARY).all()) for b in self.bufs)


KINDS = ['step', 'counted', 'ranges', 'groups']
SKIPPED = [0, 3]


def _ranges_of(n, table):
    if table == 'long':                          # a range longer than a block, mixed lags
        return [(0, 1300, 0), (1304, 7, 2), (1312, n - 1312, 1)]
    return [(0, 4, 0), (4, n - 4, 0)] if n > 4 else [(0, n, 0)]


def _launch(kind, s, t, h, rs=None, rows=None, step_dev=False):
    """one Adam call of `kind` with step t: by value, or (step_dev) from a device word -- `counted` from its counter either way.
    rows: [(lr, b1, b2, eps, wd, decoupled)] and rs with a group per range for `groups`."""
    sd = torch.tensor([t], dtype=torch.int64, device=DEV) if step_dev else None
    if kind == 'step':
        ops.adam_step(s.p, s.g, s.m, s.v, t, *h, step_dev=sd)
    elif kind == 'counted':
        count = torch.tensor([t - 1], dtype=torch.int64, device=DEV)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.adam_step_counted(s.p, s.g, s.m, s.v, *h, count, ticket, advance=True)
        torch.cuda.synchronize()
        assert int(count) == t and int(ticket) == 0, 'the counting epilogue'
    elif kind == 'ranges':
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, [(o, k, lag) for o, k, lag, *_ in rs], t, *h, step_dev=sd)
    else:
        table = torch.zeros(64, dtype=torch.float32, device=DEV)
        ops.adam_hyper_write(table, rows)
        ops.adam_step_groups(s.p, s.g, s.m, s.v, rs, table, len(rows), t, h[5], step_dev=sd)
    torch.cuda.synchronize()


def _diff(a, b):
    return [int((_bits(x) != _bits(y)).sum()) for x, y in zip(a, b)]


CASES = AC.CASES[::3]


@pytest.mark.parametrize('n', [5, 1023])
@pytest.mark.parametrize('kind', KINDS)
def test_guarded_adam_launches(kind, n):
    """flag 0, S in {0, 3}, the step t + S by value (`counted`: from its counter): zero elements differ from the clipped launch with
    the same coefficient and step_dev holding t, and the result is inside adam_cases.bounds with step t.  Flag 1 with NaN among the
    gradients: p, m, v and the canaries keep their bits, `counted` advances its counter all the same.  After the block: the plain
    launch."""
    worst = 0.0
    for c in CASES:
        h = AC.hyper32(c.hyper)
        state = AC.make_state(c, n)
        rs = [r + (0,) for r in _ranges_of(n, None)]
        rows = [tuple(h[:5]) + (False,)]
        coef = 0.37
        cbuf = torch.tensor([coef], dtype=torch.float32, device=DEV)
        want, plain = State(state), State(state)
        _launch(kind, plain, c.step, h, rs, rows)
        with ops.adam_clip(cbuf):
            _launch(kind, want, c.step, h, rs, rows, step_dev=True)
        for S in SKIPPED:
            out = torch.tensor([coef, 1.0, 0.0, CANARY], dtype=torch.float32, device=DEV)
            skipped = torch.tensor([S], dtype=torch.int64, device=DEV)
            got = State(state)
            with ops.adam_guard(out, skipped):
                _launch(kind, got, c.step + S, h, rs, rows)
            assert _diff(got.result(), want.result()) == [0, 0, 0], (c.id, S)
            assert got.canaries_ok() and int(skipped) == S and out.cpu().tolist()[2:] == [0.0, np.float32(CANARY)]
            use = CC.use_of_bounds([x.cpu().numpy() for x in got.result()], *state, c.step, h, coef)
            worst = max(worst, max(use))
            assert max(use) <= 1.0, (c.id, S, use)
        # flag 1: nothing is touched
        poisoned = [a.copy() for a in state]
        poisoned[1][n // 2] = np.nan
        got = State(poisoned)
        before = [b.clone() for b in got.bufs]
        out = torch.tensor([coef, float('nan'), 1.0, CANARY], dtype=torch.float32, device=DEV)
        with ops.adam_guard(out, torch.tensor([1], dtype=torch.int64, device=DEV)):
            _launch(kind, got, c.step + 1, h, rs, rows)
        for b, a in zip(before, got.bufs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (c.id, 'a skipped launch wrote something')
        # after the block: the plain launch
        after, none = State(state), State(state)
        _launch(kind, after, c.step, h, rs, rows)
        with ops.adam_guard(None):
            _launch(kind, none, c.step, h, rs, rows)
        assert _diff(after.result(), plain.result()) == [0, 0, 0], (c.id, 'the setting stuck')
        assert _diff(none.result(), plain.result()) == [0, 0, 0], c.id
        if c.mag == 1.0:
            assert sum(_diff(want.result(), plain.result())) > 0, (c.id, 'coefficient 0.37 changed nothing')
    _fig('guarded_adam', kind=kind, n=n, worst_use_of_a_bound=worst)


@pytest.mark.parametrize('kind', ['ranges', 'groups'])
def test_guarded_launches_over_a_long_table_with_lags(kind):
    """a range longer than one block, mixed lags, alignment gaps that hold canaries -- `groups`: three rows, the middle range on a
    DECOUPLED one.  Flag 0: the bits of the clipped launch with step_dev holding t - S (a lag that reaches below 1 clamps at 1 in
    both); flag 1: nothing is touched."""
    n = 2500
    for c in (AC.Case(0, 3, 1.0), AC.Case(1, 1000, 1e-3)):
        h = AC.hyper32(c.hyper)
        state = AC.make_state(c, n)
        base = _ranges_of(n, 'long')
        for a in state:                           # the gaps between the ranges belong to nobody
            a[1300:1304] = CANARY; a[1311:1312] = CANARY
        rs = [r + (g,) for r, g in zip(base, (0, 1, 2))]
        rows = [tuple(h[:5]) + (False,), WC.ROWS_W[0] + (True,), WC.ROW_COUPLED + (False,)]
        cbuf = torch.tensor([0.37], dtype=torch.float32, device=DEV)
        want = State(state)
        with ops.adam_clip(cbuf):
            _launch(kind, want, c.step, h, rs, rows, step_dev=True)
        assert sum(_diff(want.result(), State(state).result())) > 0
        for S in SKIPPED:
            got = State(state)
            out = torch.tensor([0.37, 1.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
            with ops.adam_guard(out, torch.tensor([S], dtype=torch.int64, device=DEV)):
                _launch(kind, got, c.step + S, h, rs, rows)
            assert _diff(got.result(), want.result()) == [0, 0, 0], (c.id, S)
            assert got.canaries_ok()
            for x in got.result():
                assert bool((x[1300:1304] == CANARY).all()) and bool((x[1311:1312] == CANARY).all())
        got = State(state)
        got.g[1305] = float('nan')
        before = [b.clone() for b in got.bufs]
        out = torch.tensor([0.37, 1.0, 1.0, 0.0], dtype=torch.float32, device=DEV)
        with ops.adam_guard(out, torch.tensor([0], dtype=torch.int64, device=DEV)):
            _launch(kind, got, c.step, h, rs, rows)
        for b, a in zip(before, got.bufs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), c.id


# ---------------------------------------------------------------------------------------------------------------------------
# 3. FusedAdam end to end
# ---------------------------------------------------------------------------------------------------------------------------
def _l2_weight(model):
    return next(n for n, _ in model.named_parameters() if model.param_group_of(n).startswith('L2_') and n.endswith('.weight'))


def _masks(model, optim):
    """per group: the mask of its trainable elements"""
    out = []
    names = optim.group_names()
    pd = dict(model.named_parameters())
    for grp in names:
        mask = torch.zeros(model.flat_params().numel(), dtype=torch.bool, device=DEV)
        for n in grp:
            o, k = model._offsets[n]
            mask[o:o + k] = pd[n].requires_grad
        out.append(mask)
    return out


def _use(after, before, grad, coef, step_of, model, optim):
    """worst use of a bound over the groups; step_of: mask -> Adam step, given as [(mask, step)] cut with each group's mask"""
    worst = [0.0, 0.0, 0.0]
    scaled = CC.scaled_g(grad, coef)
    for gmask, row in zip(_masks(model, optim), WC.rows_of(optim)):
        hyper = AC.hyper32(tuple(row[:5]) + (optim.grad_scale,))
        ref = WC.ref64w if row[5] else AC.ref64
        for mask, step in step_of:
            mk = gmask & mask
            if not bool(mk.any()):
                continue
            pn, mn, vn, G, A, V = ref(before[0][mk], scaled[mk], before[1][mk], before[2][mk], step, hyper)
            for i, (x, r, b) in enumerate(zip((after[0][mk], after[1][mk], after[2][mk]), (pn, mn, vn), AC.bounds(before[0][mk], before[1][mk], G, A, V))):
                worst[i] = max(worst[i], float(((x.double() - r).abs() / b).max()))
    return worst


def _build(variant):
    from lirec_amd.optim import FusedAdam
    model, loss, optim, batch = TC._fresh()
    if variant == 'groups':
        optim = FusedAdam(model, lr=TC.LR, param_groups=WC.two_groups(model), skip_nonfinite=True)
    else:
        optim.skip_nonfinite = True
    if variant == 'frozen':
        dict(model.named_parameters())[_l2_weight(model)].requires_grad_(False)
    return model, loss, optim, batch


def _torch_round_trip(model, optim, want_steps):
    """state_dict() -> torch.optim.Adam -> back: the same per-parameter steps and moments"""
    sd = optim.state_dict()
    steps = [int(sd['state'][i]['step']) for i in sorted(sd['state'])]
    assert steps == want_steps, (steps, want_steps)
    params = [torch.nn.Parameter(p.detach().clone()) for g in optim.param_groups for p in g['params']]
    sizes = [len(g['params']) for g in optim.param_groups]
    groups, at = [], 0
    for g, k in zip(optim.param_groups, sizes):
        groups.append(dict(params=params[at:at + k], lr=g['lr'], betas=g['betas'], eps=g['eps'], weight_decay=g['weight_decay'],
                           decoupled_weight_decay=bool(g.get('decoupled_weight_decay', False))))
        at += k
    stock = torch.optim.Adam(groups)
    stock.load_state_dict(sd)
    back = stock.state_dict()
    assert [int(back['state'][i]['step']) for i in sorted(back['state'])] == want_steps
    m, v = optim._m.clone(), optim._v.clone()
    optim.load_state_dict(back)
    torch.cuda.synchronize()
    assert torch.equal(optim._m, m) and torch.equal(optim._v, v) and int(optim.skipped_steps) == 0
    sd2 = optim.state_dict()
    assert [int(sd2['state'][i]['step']) for i in sorted(sd2['state'])] == want_steps


@pytest.mark.parametrize('bad', ['nan', 'pinf'])
@pytest.mark.parametrize('variant', ['plain', 'clipped', 'groups', 'frozen'])
def test_fused_adam_skips_a_non_finite_step(variant, bad):
    """five steps, a non-finite value written into one gradient element between backward and step() of step 3 -- a trainable one
    (step 3 changes no bit, steps 4 and 5 are Adam steps 3 and 4), or (`frozen`) one of a frozen slice: no skip."""
    try:
        model, loss, optim, batch = _build(variant)
        target = _l2_weight(model)
        to, tk = model._offsets[target]
        assert float(optim.found_nonfinite) == 0.0 and int(optim.skipped_steps) == 0 and optim.found_nonfinite.dim() == 0
        everything = torch.ones(model.flat_params().numel(), dtype=torch.bool, device=DEV)
        done = 0                                  # updates received by the trainable parameters
        for s in (1, 2, 3, 4, 5):
            TC._backward(model, loss, optim, batch)
            g = model.flat_grads(attach=False)
            if s == 3:
                g[to + tk // 2] = GC.BAD[bad]
                torch.cuda.synchronize()
            live = TC._live_mask(model)
            grad = g.clone()
            if variant == 'clipped' and s == 1:
                optim.max_grad_norm = 0.5 * math.sqrt(float((grad[live].double() ** 2).sum()))
            before = TC._state(model, optim)
            optim.step()
            torch.cuda.synchronize()
            after = TC._state(model, optim)
            assert torch.equal(model.flat_grads(attach=False).view(torch.int32), grad.view(torch.int32)), 'the step wrote the gradients'
            skip = s == 3 and variant != 'frozen'
            assert float(optim.found_nonfinite) == (1.0 if skip else 0.0), (s, float(optim.found_nonfinite))
            for a, b, what in zip(after, before, 'pmv'):
                assert torch.equal(a[~live].view(torch.int32), b[~live].view(torch.int32)), (what, 'written outside the trainable elements')
            if skip:
                for a, b, what in zip(after, before, 'pmv'):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, 'a skipped step changed bits')
                assert not math.isfinite(float(optim.grad_norm))
                continue
            done += 1
            sq = float((grad[live].double() ** 2).sum())
            coef = 1.0
            if variant == 'clipped':
                want, _ = CC.coef_of(sq, optim.grad_scale, optim.max_grad_norm)
                assert TC._adjacent(optim.clip_coef.cpu().numpy(), want), (s, float(optim.clip_coef), want)
                coef = float(optim.clip_coef)
            else:
                assert float(optim.clip_coef) == 1.0
            assert TC._adjacent(optim.grad_norm.cpu().numpy(), np.float32(math.sqrt(sq) * optim.grad_scale))
            use = _use(after, before, grad, coef, [(live & everything, done)], model, optim)
            _fig('fused_adam', variant=variant, bad=bad, call=s, adam_step=done, p=use[0], m=use[1], v=use[2])
            assert max(use) <= 1.0, (s, done, use)
        n_skipped = 0 if variant == 'frozen' else 1
        assert int(optim.skipped_steps) == n_skipped and optim.skipped_total() == n_skipped
        flags = [p.requires_grad for p in model._plist]
        by_group = [n for grp in optim.group_names() for n in grp]
        live_of = dict(zip(optim._names, flags))        # (a parameter frozen from the start has received nothing)
        _torch_round_trip(model, optim, [5 - n_skipped if live_of[n] else 0 for n in by_group])
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. frozen parameters and skipped steps
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_per_parameter_step_through_freezing_and_skipping():
    """step / freeze W, step / SKIP / unfreeze, SKIP / step: state['step'] is the count kept by hand, and the last update takes W
    with Adam step 2 and everything else with step 3"""
    try:
        model, loss, optim, batch = _build('plain')
        W = _l2_weight(model)
        wp = dict(model.named_parameters())[W]
        wo, wk = model._offsets[W]
        other = next(n for n in optim._names if n != W)
        oo, _ = model._offsets[other]
        led = GC.Ledger(len(optim._names))
        script = [(True, False), (False, False), (False, True), (True, True), (True, False)]      # (W trainable, skipped)
        for call, (w_live, skipped) in enumerate(script, 1):
            wp.requires_grad_(w_live)
            TC._backward(model, loss, optim, batch)
            g = model.flat_grads(attach=False)
            if skipped:
                g[oo] = float('nan')
                torch.cuda.synchronize()
            grad, live, before = g.clone(), TC._live_mask(model), TC._state(model, optim)
            optim.step()
            torch.cuda.synchronize()
            after = TC._state(model, optim)
            want = led.call([p.requires_grad for p in model._plist], skipped)
            assert float(optim.found_nonfinite) == float(skipped)
            sd = optim.state_dict()
            assert [int(sd['state'][i]['step']) for i in sorted(sd['state'])] == want, (call, want)
            if skipped:
                for a, b in zip(after, before):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), call
        # the last update: W with its own count, the rest with theirs
        wmask = torch.zeros_like(live)
        wmask[wo:wo + wk] = True
        steps = dict(zip(optim._names, want))
        assert steps[W] == 2 and steps[other] == 3
        use = _use(after, before, grad, 1.0, [(live & wmask, 2), (live & ~wmask, 3)], model, optim)
        _fig('frozen_accounting', p=use[0], m=use[1], v=use[2], skipped_total=optim.skipped_total())
        assert max(use) <= 1.0, use
        assert optim.skipped_total() == 2
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 5 - 6. recorded = eager; off is off
# ---------------------------------------------------------------------------------------------------------------------------
_runs = {}


def _poison_spot(batch):
    """a feature element of a candidate that IS part of its clip"""
    b, t = [int(x) for x in torch.nonzero(batch['mem_mask'].reshape(batch['mem_mask'].shape[0], -1) == 1)[0][:2]]
    f = batch['features']
    assert f.dtype == torch.float32
    return f.reshape(f.shape[0], -1, f.shape[-2], f.shape[-1])[b, t, 0, 40:41]


def _run(route, guard, steps=5, poison_at=3):
    key = (route, guard, steps, poison_at)
    if key not in _runs:
        try:
            _runs[key] = _run_once(route, guard, steps, poison_at)
        except BaseException as e:
            _runs[key] = e
    if isinstance(_runs[key], BaseException):
        raise _runs[key]
    return _runs[key]


def _snap(model, optim, lv):
    return TC._state(model, optim) + (optim._skipped_dev.clone() if optim._skipped_dev is not None else None, lv.detach().reshape(-1)[:1].clone())


def _run_once(route, guard, steps, poison_at):
    from lirec_amd.graph import RecordedTrainStep
    out = {'steps': []}
    try:
        model, loss, optim, batch = TC._fresh(side=route != 'plain')
        if guard != 'no keyword':
            optim.skip_nonfinite = guard
        spot = _poison_spot(batch)
        keep = spot.clone()

        def poison(s):
            if s == poison_at:
                spot.fill_(float('nan'))
            else:
                spot.copy_(keep)
        if route != 'recorded':
            for s in range(1, steps + 1):
                poison(s)
                optim.zero_grad()
                lv = loss(model(dict(batch)), batch)
                lv.backward()
                optim.step()
                torch.cuda.synchronize()
                out['steps'].append(_snap(model, optim, lv))
        else:
            poison(1)
            g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
            try:
                torch.cuda.synchronize()
                out['flags'] = (g.overwrite, g.fused, g.defer)
                lanes = {}
                out['commands'] = [(lanes.setdefault(s, len(lanes)), k) for s, k in (g.cmds.command(i) for i in range(g.cmds.size))]
                out['steps'] += [None, _snap(model, optim, g.loss_out)]
                for s in range(3, steps + 1):
                    poison(s)
                    lv = g.step()
                    torch.cuda.synchronize()
                    out['steps'].append(_snap(model, optim, lv))
                out['state'] = g.state.tolist()
                if guard is True:
                    optim.skip_nonfinite = False
                    with pytest.raises(RuntimeError, match='hyper-parameters changed'):
                        g.step()
                    optim.skip_nonfinite = True
            finally:
                g.release()
    finally:
        config.reset()
    return out


def test_recorded_is_eager_with_a_skipped_step():
    """five steps (recorded: one warm-up step, the recording step, three replays), the batch's features holding a NaN during step
    3: parameters, moments, the count of skipped steps and the loss values bit for bit; the replay after the skipped one updates
    with the step that was not consumed (it IS the eager loop's); a replay after skip_nonfinite changed raises (inside _run_once)."""
    eager, rec = _run('side', True), _run('recorded', True)
    assert rec['flags'][1:] == (False, False)
    assert len(rec['steps']) == 5 and rec['state'][1:] == [5, 5]
    assert [int(s[3]) for s in eager['steps']] == [0, 0, 1, 1, 1]
    # (the loss VALUE of the poisoned step may well be finite -- a hinge keeps no NaN -- while its gradients are not)
    for a, b in zip(eager['steps'][1][:3], eager['steps'][2][:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'the eager loop\'s step 3 was not skipped'
    assert not torch.equal(eager['steps'][2][0], eager['steps'][3][0])
    for s in range(1, 5):
        for x, y, what in zip(eager['steps'][s], rec['steps'][s], ('parameters', 'exp_avg', 'exp_avg_sq', 'skipped_steps', 'loss')):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (s + 1, what)
    plain = _run('plain', True)
    for x, y in zip(eager['steps'][4][:4], plain['steps'][4][:4]):
        assert torch.equal(x, y), 'plain vs side stream'


@pytest.mark.parametrize('route', ['plain', 'side', 'recorded'])
def test_off_is_off(route):
    """3 steps with skip_nonfinite=False against the route without the keyword: parameters and moments bit for bit, no counter
    made, and the recorded command list has the same commands on the same streams in the same order -- no extra launch."""
    base, got = _run(route, 'no keyword', 3, 0), _run(route, False, 3, 0)
    for s, (a, b) in enumerate(zip(base['steps'], got['steps'])):
        if a is None:
            continue
        for x, y, what in zip(a[:3], b[:3], ('parameters', 'exp_avg', 'exp_avg_sq')):
            assert torch.equal(x, y), (route, s + 1, what)
        assert a[3] is None and b[3] is None, 'the unguarded route made the guard\'s buffers'
    if route == 'recorded':
        assert got['flags'] == base['flags'] and got['commands'] == base['commands']
        on = _run('recorded', True)
        assert len(on['commands']) != len(base['commands']) and base['flags'][1:] == (True, True)
