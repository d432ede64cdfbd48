"""Gradient clipping by global norm on the device (include/lirec_hip.h, "gradient clipping"; lirec_amd/optim.py): the norm
kernels against float64, the clipped Adam launches against float64 and the fp32 restatement, and FusedAdam.step() with
``max_grad_norm`` on its plain, side-stream and recorded routes.

Bounds.  The sum of squares: every square of an fp32 value is exact in double, and a sum of n non-negative doubles in any order is
within (n - 1) 2^-53 of exact, relatively: |device - fsum| <= n 2^-53 fsum.  The clipped update: adam_cases.bounds with the scale
gs * coef (tests/test_host_clip.py shows the fp32 restatement inside them for the coefficients used here).  coef and norm: the
float32 nearest to the float64 value computed from the DEVICE's sum of squares, or a neighbour of it.

Measured on an MI355X.  Sum of squares, relative error against fsum: 0 in 20 of the 24 (size, magnitude) pairs, at most 2.4e-16
otherwise (n = 1025: bound 1.1e-13; n = 1 049 603: 1.2e-16 against a bound of 1.2e-10); the range tables: at most 1.9e-16.  Clipped
Adam launches: the worst use of a bound 0.24 (n = 5) and 0.31 (n = 1023), the same for all three calls, and 0 elements differing
from the fp32 restatement -- lirec_adam_step_counted included.  FusedAdam end to end (18 431 616 elements): norms 694.4 / 26.7 / 45.7 over the three steps,
coefficients 0.5 / 1 / 1, worst use of a bound 0.27 (p) / 0.07 (m) / 0.37 (v).  Recorded against eager, max_grad_norm 347.2:
coefficients 0.5, 1, 1, 1, 1 over the five steps, everything bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import adam_cases as AC
import clip_cases as CC
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
P = _lib.CLIP_PARTIALS
GUARD = 64
CANARY = 1e30                                   # (a guard or gap element that leaked into a sum of squares shows at once)
U53 = 2.0 ** -53


def _fig(what, **kw):
    print('CLIP-FIGURE %s %s' % (what, ' '.join('%s=%s' % (k, ('%.4g' % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


class Norm:
    """partials (between guard doubles), the device double and the (coef, norm) pair of one norm computation"""

    def __init__(self):
        self.pbuf = torch.full((P + 16,), float('nan'), dtype=torch.float64, device=DEV)
        self.partials = self.pbuf[8:8 + P]
        self.sq = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
        self.out = torch.full((2,), float('nan'), dtype=torch.float32, device=DEV)

    def run(self, g, tables, grad_scale=1.0, max_norm=1.0):
        self.partials.fill_(float('nan'))
        for i, t in enumerate(tables):
            ops.grad_sq_partials(g, t, self.partials)
            ops.clip_finalize(self.partials, self.sq, 0 if i == 0 else 1, grad_scale, max_norm, self.out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.pbuf[:8]).all()) and bool(torch.isnan(self.pbuf[8 + P:]).all()), 'guards of the partials were written'
        assert not bool(torch.isnan(self.partials).any()), 'not every partial was written'
        return float(self.sq)


def _guarded(values):
    """the values as a 16-byte aligned slice of a buffer whose other elements are CANARY"""
    n = len(values)
    buf = torch.full((GUARD + n + GUARD + 3,), CANARY, dtype=torch.float32, device=DEV)
    buf[GUARD:GUARD + n] = torch.from_numpy(values).to(DEV)
    g = buf[GUARD:GUARD + n]
    assert g.data_ptr() % 16 == 0
    return buf, g


def _fsum_sq(values):
    v = np.asarray(values, np.float64)
    return math.fsum((v * v).tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# 1. partials and finalize against float64
# ---------------------------------------------------------------------------------------------------------------------------
N_LONG = P * 1024 + 1027                         # workgroups 0 and 1 take a second block; a scalar tail of three
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, N_LONG]


@pytest.mark.parametrize('n', SIZES)
def test_sum_of_squares_against_float64(n):
    nm = Norm()
    for mag in (1.0, 1e-12, 1e3):
        vals = (mag * np.random.default_rng(n % 1000 + int(-math.log10(mag)) + 20).standard_normal(n)).astype(np.float32)
        vals[vals == 0] = np.float32(mag)
        buf, g = _guarded(vals)
        keep = buf.clone()
        sq = nm.run(g, [[(0, n)]])
        want = _fsum_sq(vals)
        parts = nm.partials.cpu().numpy()
        err, err_parts = abs(sq - want) / want, abs(math.fsum(parts.tolist()) - want) / want
        _fig('sum_sq', n=n, mag=mag, rel_err=err, rel_err_of_fsum_of_partials=err_parts, bound=n * U53)
        assert err <= n * U53 and err_parts <= n * U53, (n, mag, err, err_parts)
        assert torch.equal(buf, keep), 'the gradient buffer was written'
        nblocks = (n + 1023) // 1024
        assert bool((nm.partials[min(nblocks, P):] == 0).all()), 'a workgroup without work stored something'
        assert bool((nm.partials[:min(nblocks, P)] > 0).all())
        coef, norm = CC.coef_of(sq, 1.0, 1.0)
        assert abs(int(_bits(nm.out)[0]) - int(coef.view(np.uint32))) <= 1 and abs(int(_bits(nm.out)[1]) - int(norm.view(np.uint32))) <= 1


# ---------------------------------------------------------------------------------------------------------------------------
# 2. range tables
# ---------------------------------------------------------------------------------------------------------------------------
TABLES = {
    'three_ranges_with_gaps': [[(0, 1500), (1504, 7), (3000, 2049)]],
    'length_1_at_a_multiple_of_4': [[(1028, 1)]],
    '64_ranges_of_5': [[(8 * i, 5) for i in range(64)]],
    '65_ranges_in_two_calls': [[(8 * i, 5) for i in range(64)], [(8 * 64, 5)]],
    'an_empty_range_between': [[(0, 9), (12, 0), (16, 1030)]],
}


@pytest.mark.parametrize('what', sorted(TABLES))
def test_range_tables(what):
    tables = TABLES[what]
    L = 6000
    vals = np.random.default_rng(len(what)).standard_normal(L).astype(np.float32)
    inside = np.zeros(L, bool)
    for t in tables:
        for o, k in t:
            inside[o:o + k] = True
    vals[~inside] = CANARY                        # the gaps
    buf, g = _guarded(vals)
    nm = Norm()
    sq = nm.run(g, tables)
    want, n = _fsum_sq(vals[inside]), int(inside.sum())
    err = abs(sq - want) / want
    _fig('ranges', table=what, n=n, rel_err=err, bound=n * U53)
    assert err <= n * U53, (what, sq, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_same_bits_in_every_launch():
    n = 300 * 1024 + 77
    vals = np.random.default_rng(9).standard_normal(n).astype(np.float32)
    _, g = _guarded(vals)
    table = [[(0, 100000), (100000, n - 100000)]]
    a, b, c = Norm(), Norm(), Norm()
    a.run(g, table)
    b.run(g, table)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c.run(g, table)
    for x, where in ((b, 'a second launch'), (c, 'a launch on another stream')):
        assert torch.equal(a.sq.view(torch.int64), x.sq.view(torch.int64)), where
        assert torch.equal(a.partials.view(torch.int64), x.partials.view(torch.int64)), where
        assert torch.equal(a.out.view(torch.int32), x.out.view(torch.int32)), where


# ---------------------------------------------------------------------------------------------------------------------------
# 4. finalize arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def _finalize(sq_value, gs, mn, mode=2, partials=None):
    sq = torch.tensor([sq_value], dtype=torch.float64, device=DEV)
    out = torch.full((2,), float('nan'), dtype=torch.float32, device=DEV)
    ops.clip_finalize(partials, sq, mode, gs, mn, out)
    torch.cuda.synchronize()
    return float(sq), out.cpu().numpy()


def _adjacent(got, want):
    return abs(int(np.float32(got).view(np.uint32)) - int(np.float32(want).view(np.uint32))) <= 1


@pytest.mark.parametrize('gs,mn', [(1.0, 1.0), (0.5, 1.0), (1.0, 1e9)])
def test_finalize_arithmetic(gs, mn):
    for sq0 in (0.0, 1e-30, 1.0, 1e6):
        sq, out = _finalize(sq0, gs, mn)
        assert sq == sq0                                         # (mode 2: taken as it stands)
        coef, norm = CC.coef_of(sq, gs, mn)
        x = float(np.float32(mn)) / (math.sqrt(sq) * gs + 1e-6)
        _fig('finalize', sq=sq0, gs=gs, mn=mn, coef=float(out[0]), norm=float(out[1]), x=x)
        assert _adjacent(out[0], coef) and _adjacent(out[1], norm), (sq0, out, coef, norm)
        if x >= 1.0:
            assert out[0] == np.float32(1.0)
        else:
            assert out[0] < 1.0
    assert np.isnan(_finalize(float('nan'), gs, mn)[1][0])
    sq, out = _finalize(float('inf'), gs, mn)
    assert out[0] == 0.0 and np.isinf(out[1])


def test_finalize_modes():
    parts = torch.zeros(P, dtype=torch.float64, device=DEV)
    parts[:3] = torch.tensor([1.5, 2.25, 0.25], dtype=torch.float64)
    parts[P - 1] = 5.0
    assert _finalize(100.0, 1.0, 1.0, 0, parts)[0] == 9.0
    assert _finalize(100.0, 1.0, 1.0, 1, parts)[0] == 109.0
    sq, out = _finalize(100.0, 1.0, 1.0, 2, parts)
    assert sq == 100.0 and out[1] == 10.0


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the clipped Adam launches
# ---------------------------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, state):
        self.p, self.g, self.m, self.v = (torch.from_numpy(a.copy()).to(DEV) for a in state)

    def result(self):
        return self.p, self.m, self.v


def _call(kind, s, c, h, gs=None):
    h = h if gs is None else h[:5] + (gs,)
    n = s.p.numel()
    if kind == 'step':
        ops.adam_step(s.p, s.g, s.m, s.v, c.step, *h)
    elif kind == 'counted':
        count = torch.tensor([c.step - 1], dtype=torch.int64, device=DEV)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.adam_step_counted(s.p, s.g, s.m, s.v, *h, count, ticket, advance=True)
        torch.cuda.synchronize()
        assert int(count) == c.step and int(ticket) == 0
    else:
        rs = [(0, 4, 0), (4, n - 4, 0)]
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, rs, c.step, *h)
    torch.cuda.synchronize()


def _same_bits(a, b):
    return [int((_bits(x) != _bits(y)).sum()) for x, y in zip(a, b)]


@pytest.mark.parametrize('n', [5, 1023])
@pytest.mark.parametrize('kind', ['step', 'counted', 'ranges'])
def test_clipped_adam_launches(kind, n):
    """With a coefficient buffer set by hand (0.37, 1.0): within adam_cases.bounds of ref64 with the scale gs * coef; the bits of the
    SAME call with the fp32 product gs32 * coef32 handed in as grad_scale and nothing set; coefficient 1.0: the bits of the call with
    nothing set; after clearing, today's bits.  All three calls are the fp32 restatement clip_cases.ref32 bit for bit --
    lirec_adam_step_counted too, whose bias corrections come from the device's double-precision pow / sqrt (0 differing elements
    measured)."""
    worst, differ32 = 0.0, 0
    for c in AC.CASES:
        h = AC.hyper32(c.hyper)
        state = AC.make_state(c, n)
        plain = State(state)
        _call(kind, plain, c, h)
        for coef in (0.37, 1.0):
            cbuf = torch.tensor([coef], dtype=torch.float32, device=DEV)
            got, byhand = State(state), State(state)
            with ops.adam_clip(cbuf):
                _call(kind, got, c, h)
            _call(kind, byhand, c, h, gs=float(np.float32(h[5]) * np.float32(coef)))
            assert torch.equal(got.g, plain.g) and float(cbuf) == float(np.float32(coef))
            use = CC.use_of_bounds([x.cpu().numpy() for x in got.result()], *state, c.step, h, coef)
            want = CC.ref32(*state, c.step, h, coef)
            d32 = sum(int((_bits(x) != w.view(np.uint32)).sum()) for x, w in zip(got.result(), want))
            worst, differ32 = max(worst, max(use)), differ32 + d32
            assert max(use) <= 1.0, (c.id, coef, use)
            assert _same_bits(got.result(), byhand.result()) == [0, 0, 0], (c.id, coef)
            assert d32 == 0, (c.id, coef, 'elements whose bits differ from the fp32 restatement', d32)
            if coef == 1.0:
                assert _same_bits(got.result(), plain.result()) == [0, 0, 0], (c.id, 'coefficient 1.0 is not the unclipped call')
            elif c.mag == 1.0:                   # (a gradient of 1e-12 can vanish beside the weight-decay term, clipped or not)
                assert sum(_same_bits(got.result(), plain.result())) > 0, (c.id, 'coefficient 0.37 changed nothing')
        after = State(state)
        _call(kind, after, c, h)                 # (the setting does not stick)
        assert _same_bits(after.result(), plain.result()) == [0, 0, 0], c.id
    _fig('clipped_adam', kind=kind, n=n, worst_use_of_a_bound=worst, differ_from_ref32=differ32)


# ---------------------------------------------------------------------------------------------------------------------------
# 6 - 8. FusedAdam
# ---------------------------------------------------------------------------------------------------------------------------
B, T, R = 4, 8, 18
LR = 1e-3


def _fresh(side=True, **kw):
    """the small model of tests/test_gpu_optim.py's route tests"""
    from lirec_amd import model as M
    from lirec_amd.data import synthetic_batch, to_device_batch
    from oracle import lirec_oracle as O
    config.recipe('int_rel_ch', rels_n_clips=R, dropout_seed=77, lr=LR)
    opt.device = 'cuda'
    opt.adam_on_side_stream = side
    model, loss, optim = M.create_model(101, n_rels=15)
    model.load_state_dict(O.fill_params(O.param_shapes(O.OracleCfg(), 101, 15), 5), strict=True)
    model.train()
    batch = to_device_batch(synthetic_batch(11, 'int_rel_ch', B, T=T, R=R), 'cuda')
    for k, v in kw.items():
        setattr(optim, k, v)
    return model, loss, optim, batch


def _hyper_of(optim):
    g = optim.param_groups[0]
    return AC.hyper32((g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], optim.grad_scale))


def _backward(model, loss, optim, batch):
    optim.zero_grad()
    lv = loss(model(dict(batch)), batch)
    lv.backward()
    optim._ensure_state()
    torch.cuda.synchronize()


def _state(model, optim):
    return tuple(t.clone() for t in (model.flat_params(), optim._m, optim._v))


def _live_mask(model):
    mask = torch.zeros(model.flat_params().numel(), dtype=torch.bool, device=DEV)
    for (n, p) in model.named_parameters():
        o, k = model._offsets[n]
        mask[o:o + k] = p.requires_grad
    return mask


@pytest.mark.parametrize('freeze', [False, True], ids=['all_trainable', 'one_L2_weight_frozen'])
def test_fused_adam_clips_end_to_end(freeze):
    """three steps; norm, coefficient, parameters and both moments computed on the host side in float64 from the device's own
    gradients, read back in front of each update.  Step 1 and 2: max_grad_norm = half of step 1's norm (step 1 clips); step 3: four
    times its own norm (coefficient exactly 1).  p.grad keeps its bits.  Frozen: the slice's gradient is filled with 1e30."""
    try:
        model, loss, optim, batch = _fresh()
        frozen = None
        if freeze:
            frozen = next(n for n, _ in model.named_parameters() if model.param_group_of(n).startswith('L2_') and n.endswith('.weight'))
            dict(model.named_parameters())[frozen].requires_grad_(False)
            fo, fk = model._offsets[frozen]
        hyper = None
        assert float(optim.clip_coef) == 1.0 and float(optim.grad_norm) == 0.0 and optim.clip_coef.dim() == 0
        clipped = []
        for s in (1, 2, 3):
            _backward(model, loss, optim, batch)
            hyper = hyper or _hyper_of(optim)
            g = model.flat_grads(attach=False)
            if freeze:
                g[fo:fo + fk] = 1e30
                torch.cuda.synchronize()
            live = _live_mask(model)
            grad = g.clone()
            sq = float((grad[live].double() ** 2).sum())
            if s == 1:
                optim.max_grad_norm = 0.5 * math.sqrt(sq)
            elif s == 3:
                optim.max_grad_norm = 4.0 * math.sqrt(sq)
            before = _state(model, optim)
            optim.step()
            torch.cuda.synchronize()
            after = _state(model, optim)
            coef, norm = CC.coef_of(sq, optim.grad_scale, optim.max_grad_norm)
            got_coef, got_norm = optim.clip_coef.cpu().numpy(), optim.grad_norm.cpu().numpy()
            _fig('fused_adam', frozen=freeze, step=s, norm=float(got_norm), coef=float(got_coef), want_norm=float(norm), want_coef=float(coef))
            # (the device sums in another order than torch: n 2^-53 relative on the sum of squares is far below half an fp32 ulp,
            #  but a value next to a rounding boundary may still land on the neighbour)
            assert _adjacent(got_coef, coef) and _adjacent(got_norm, norm)
            assert torch.equal(model.flat_grads(attach=False), grad), 'the step wrote the gradients'
            scaled = CC.scaled_g(grad, float(got_coef))
            if freeze:
                scaled[fo:fo + fk] = 0.0              # (no update there: checked bit for bit below)
            use = AC.use_of_bounds([t[live] for t in after], before[0][live], scaled[live], before[1][live], before[2][live], s, hyper)
            _fig('fused_adam_bounds', frozen=freeze, step=s, p=use[0], m=use[1], v=use[2])
            assert max(use) <= 1.0, (s, use)
            # the alignment gaps and the frozen slice keep their bits
            for a, b, what in zip(after, before, 'pmv'):
                assert torch.equal(a[~live], b[~live]), (what, 'written outside the trainable elements')
            clipped.append(float(got_coef) < 1.0)
            assert not model.lanes.bucket0_on_side
        assert clipped[0] and not clipped[2] and float(optim.clip_coef) == 1.0, clipped
    finally:
        config.reset()


def test_a_clipped_step_with_nothing_trainable_updates_nothing():
    """after a step that clipped (coefficient 0.5), everything is frozen: the next step issues no update, grad_norm is 0 and the
    coefficient 1 -- not the earlier step's values --, and parameters and moments keep their bits"""
    try:
        model, loss, optim, batch = _fresh()
        _backward(model, loss, optim, batch)
        optim.max_grad_norm = 0.5 * float((model.flat_grads(attach=False).double() ** 2).sum().sqrt())
        optim.step()
        torch.cuda.synchronize()
        assert 0.0 < float(optim.clip_coef) < 1.0 and float(optim.grad_norm) > 0.0
        for p in model.parameters():
            p.requires_grad_(False)
        _backward(model, loss, optim, batch)
        before = _state(model, optim)
        optim.step()
        torch.cuda.synchronize()
        assert float(optim.clip_coef) == 1.0 and float(optim.grad_norm) == 0.0
        for a, b in zip(_state(model, optim), before):
            assert torch.equal(a, b)
    finally:
        config.reset()


_runs = {}


def _run(route, clip, steps, key=None):
    """[(flat, m, v, norm, coef) after step s] of a route ('plain' | 'side' | 'recorded') with max_grad_norm = clip"""
    key = key or (route, clip, steps)
    if key in _runs:
        if isinstance(_runs[key], BaseException):
            raise _runs[key]
        return _runs[key]
    try:
        _runs[key] = _run_once(route, clip, steps)
    except BaseException as e:
        _runs[key] = e
        raise
    return _runs[key]


def _snapshot(model, optim):
    return _state(model, optim) + (optim.grad_norm.clone(), optim.clip_coef.clone())


def _run_once(route, clip, steps):
    from lirec_amd.graph import RecordedTrainStep
    out = {'steps': []}
    try:
        model, loss, optim, batch = _fresh(side=route != 'plain')
        if clip != 'no keyword':
            optim.max_grad_norm = clip
        if route != 'recorded':
            for s in range(steps):
                _backward(model, loss, optim, batch)
                optim.step()
                torch.cuda.synchronize()
                out['steps'].append(_snapshot(model, optim))
        else:
            g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
            try:
                torch.cuda.synchronize()
                out['flags'] = (g.overwrite, g.fused, g.defer)
                lanes = {}
                out['commands'] = [(lanes.setdefault(s, len(lanes)), k) for s, k in (g.cmds.command(i) for i in range(g.cmds.size))]
                out['steps'] += [None, _snapshot(model, optim)]      # (the warm-up step's state is not kept)
                for _ in range(steps - 2):
                    g.step()
                    torch.cuda.synchronize()
                    out['steps'].append(_snapshot(model, optim))
                out['state'] = g.state.tolist()
                if clip not in ('no keyword', None, 0):
                    optim.max_grad_norm = 2.0 * float(clip)
                    with pytest.raises(RuntimeError, match='hyper-parameters changed'):
                        g.step()
                    optim.max_grad_norm = clip
            finally:
                g.release()
    finally:
        config.reset()
    return out


@pytest.mark.parametrize('clip', [None, 0, 1e30], ids=['None', '0', '1e30'])
@pytest.mark.parametrize('route', ['plain', 'side', 'recorded'])
def test_off_is_off(route, clip):
    """3 steps: parameters and both moments bit for bit those of the route without the keyword.  None / 0: the recorded command
    list has the same commands on the same streams in the same order.  1e30: clipping is ON -- another schedule -- with the
    coefficient exactly 1: the same values."""
    base, got = _run(route, 'no keyword', 3), _run(route, clip, 3)
    for s, (a, b) in enumerate(zip(base['steps'], got['steps'])):
        if a is None:
            continue
        for x, y, what in zip(a[:3], b[:3], ('parameters', 'exp_avg', 'exp_avg_sq')):
            assert torch.equal(x, y), (route, clip, s + 1, what, int((x != y).sum()))
        assert float(b[4]) == 1.0
        assert (float(b[3]) > 0) == (clip == 1e30)
    if route == 'recorded':
        if clip == 1e30:
            assert got['flags'][1:] == (False, False) and base['flags'][1:] == (True, True), (got['flags'], base['flags'])
            assert len(got['commands']) != len(base['commands'])
        else:
            assert got['flags'] == base['flags'] and got['commands'] == base['commands']


def _clip_bound():
    """half of the first step's gradient norm of the small model (measured once, on an unclipped run's first backward)"""
    if 'bound' not in _runs:
        try:
            model, loss, optim, batch = _fresh()
            _backward(model, loss, optim, batch)
            _runs['bound'] = 0.5 * float((model.flat_grads(attach=False).double() ** 2).sum().sqrt())
        finally:
            config.reset()
    return _runs['bound']


def test_recorded_is_eager_with_clipping_active():
    """five steps (recorded: one warm-up step, the recording step, three replays): parameters, moments, grad_norm and clip_coef bit
    for bit; the coefficient is below 1 in at least one step; a replay after max_grad_norm changed raises (inside _run_once)."""
    M = _clip_bound()
    eager, rec = _run('side', M, 5), _run('recorded', M, 5)
    assert rec['flags'][1:] == (False, False)
    coefs = [float(s[4]) for s in eager['steps']]
    _fig('recorded_vs_eager', max_grad_norm=M, coefs=coefs, norms=[float(s[3]) for s in eager['steps']])
    assert min(coefs) < 1.0 and coefs[0] < 1.0
    assert len(rec['steps']) == 5 and rec['state'][1:] == [5, 5]
    for s in range(1, 5):
        for x, y, what in zip(eager['steps'][s], rec['steps'][s], ('parameters', 'exp_avg', 'exp_avg_sq', 'grad_norm', 'clip_coef')):
            assert torch.equal(x, y), (s + 1, what)
    plain = _run('plain', M, 5)
    for x, y, what in zip(eager['steps'][4], plain['steps'][4], ('parameters', 'exp_avg', 'exp_avg_sq', 'grad_norm', 'clip_coef')):
        assert torch.equal(x, y), ('plain vs side stream', what)
