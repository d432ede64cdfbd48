"""Gradient accumulation on the device (include/lirec_hip.h, "gradient accumulation"; lirec_amd/optim.py, graph.py, train.py):
the head launch of a micro-step (lirec_accum_begin) over chains of calls, the Adam / EMA launches under the hold gate
(lirec_set_adam_hold), FusedAdam(accumulate_steps=k) in the eager loop for every recipe and with clip / guard / frozen / AdamW
groups / EMA on top, the recorded accumulating step against the eager loop bit for bit, training(), and accumulate_steps = 1
against an optimiser built without the argument.

Bounds.  An apply step is held, over every element of the flat buffers, to accum_cases.ref64_window: adam_cases.bounds widened
by the (k - 1) u sum|g_i| of the fp32 accumulation, pushed through the update (derived there; tests/test_host_accum.py shows the
fp32 restatement inside it).  The restatement is fed each micro-batch's own gradient, computed by a twin model with the same
parameters on a zeroed buffer (dropout off: a second forward of the model under test would consume a dropout key).  Everything
else is bit identity: a hold changes no bit; k = 2 is the bits of two backwards without zero_grad, grad_scale 0.5 and one plain
step; recorded is eager.  The clipped norm is held to the clip tests' own criterion (the neighbouring fp32 of the float64 value)
against the float64 norm of the accumulated buffer times grad_scale / k.

Measured on an MI355X.  Eager, all four recipes, k = 2 and 3: worst use of a bound 0.13 (p) / 0.22 (m) / 0.35 (v); the accumulated
buffer up to 1.00 of (k - 1) u sum|g_i| of the float64 sum.  The idiom, recorded against eager (phase 0 and 1, an eager step in
between, the side stream held back), training() eager / 'bind' / 'list' and accumulate_steps = 1: zero differing elements.
"""
import math

import numpy as np
import pytest
import torch

import accum_cases as XC
import adam_cases as AC
import adamw_cases as WC
import clip_cases as CC
import test_gpu_clip as TC
import test_gpu_guard as GG
import test_gpu_optim as GO
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)
RECIPES = {'int_rel_ch': dict(T=4, R=3), 'int_rels': dict(R=3), 'int_ch': dict(T=4), 'modalties': {}}
B, LR = 4, 1e-3
KS = [2, 3]


def _fig(what, **kw):
    print('ACCUM-FIGURE %s %s' % (what, ' '.join('%s=%s' % (k, ('%.4g' % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _eq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the head launch
# ---------------------------------------------------------------------------------------------------------------------------
CTR0 = [5, 2 ** 40 + 3, -2 ** 35]


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('nbytes', GO.BYTES)
def test_head_launch_over_a_chain_of_calls(nbytes, k):
    """2k + 1 calls from phase 0 and from phase 1, the buffer refilled before each: zeroed exactly on the calls that open a window,
    untouched -- the bytes around it always -- otherwise; the counters, the hold flag, the phase and the ticket as restated"""
    for phase0 in (0, 1):
        cbuf = torch.full((7,), -7, dtype=torch.int64, device=DEV)
        cbuf[2:5] = torch.tensor(CTR0, dtype=torch.int64)
        ctr = cbuf[2:5]
        wbuf = torch.full((8,), -9, dtype=torch.int64, device=DEV)
        wbuf[2:6] = torch.tensor([phase0, 77, 0, 123], dtype=torch.int64)
        win = wbuf[2:6]
        assert win.data_ptr() % 16 == 0
        for zeroed, hold, phase, counters in XC.head_chain(k, 2 * k + 1, phase0, CTR0):
            buf, view = GO._filled(nbytes)
            ops.accum_begin(view, ctr, [1, 0, 0], [0, 1, 1], win, k)
            torch.cuda.synchronize()
            if zeroed:
                GO._zeroed_and_guards_kept(buf, nbytes)
            else:
                assert bool((buf == GO.FILL).all()), 'a call inside a window wrote the buffer'
            assert cbuf.tolist() == [-7, -7] + list(counters) + [-7, -7]
            assert wbuf.tolist() == [-9, -9, phase, hold, 0, 123, -9, -9]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the gated launches
# ---------------------------------------------------------------------------------------------------------------------------
def _call(kind, s, t, h, rs, rows, count=None, ticket=None):
    if kind == 'step':
        ops.adam_step(s.p, s.g, s.m, s.v, t, *h)
    elif kind == 'counted':
        ops.adam_step_counted(s.p, s.g, s.m, s.v, *h, count, ticket, advance=True)
    elif kind == 'ranges':
        ops.adam_step_ranges(s.p, s.g, s.m, s.v, [(o, n, lag) for o, n, lag, *_ in rs], t, *h)
    else:
        table = torch.zeros(64, dtype=torch.float32, device=DEV)
        ops.adam_hyper_write(table, rows)
        ops.adam_step_groups(s.p, s.g, s.m, s.v, rs, table, len(rows), t, h[5])
    torch.cuda.synchronize()


def _window(hold):
    w = torch.tensor([0, hold, 0, 0], dtype=torch.int64, device=DEV)
    return w, w[1:2]


@pytest.mark.parametrize('n', [1, 5, 1023, AC.N_BIG])
@pytest.mark.parametrize('kind', GG.KINDS)
def test_gated_adam_launches(kind, n):
    """held: p, g, m, v and the canaries keep their bits, counter and ticket do not move.  Not held: the bits of the ungated launch
    with the scale (float)(grad_scale / k), the counter advanced.  With the guard also set: a no-op when either flag says so."""
    cases = [next(c for c in AC.BIG_CASES if c.hyper == 3)] if n == AC.N_BIG else AC.CASES[::6]
    for c in cases:
        for k in (2, 3):
            h = AC.hyper32(c.hyper)
            hk = XC.window_hyper(h, k)
            state = AC.make_state(c, n)
            rs = [r + (0,) for r in GG._ranges_of(n, None)]
            rows = [tuple(h[:5]) + (False,)]
            fresh = lambda: (torch.tensor([c.step - 1], dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
            # the ungated launch with the folded scale
            want = GG.State(state)
            cnt, tk = fresh()
            _call(kind, want, c.step, hk, rs, rows, cnt, tk)
            # held
            got = GG.State(state)
            before = [b.clone() for b in got.bufs]
            cnt, tk = fresh()
            w, hold = _window(1)
            with ops.adam_hold(hold, k):
                _call(kind, got, c.step, h, rs, rows, cnt, tk)
            for b, a in zip(before, got.bufs):
                assert _eq(a, b), (c.id, k, 'a held launch wrote something')
            assert int(cnt) == c.step - 1 and int(tk) == 0 and w.tolist() == [0, 1, 0, 0], (c.id, 'a held launch moved its counter')
            # not held
            got = GG.State(state)
            cnt, tk = fresh()
            w, hold = _window(0)
            with ops.adam_hold(hold, k):
                _call(kind, got, c.step, h, rs, rows, cnt, tk)
            assert GG._diff(got.result(), want.result()) == [0, 0, 0], (c.id, k)
            assert got.canaries_ok() and int(tk) == 0 and int(cnt) == (c.step if kind == 'counted' else c.step - 1)
            if c.mag == 1.0 and n > 1:
                plain = GG.State(state)
                _call(kind, plain, c.step, h, rs, rows, *fresh())
                assert sum(GG._diff(plain.result(), want.result())) > 0, (c.id, 'the factor 1 / k changed nothing')
            # after the block the plain launch is back
            after, plain = GG.State(state), GG.State(state)
            _call(kind, after, c.step, h, rs, rows, *fresh())
            with ops.adam_hold(None):
                _call(kind, plain, c.step, h, rs, rows, *fresh())
            assert GG._diff(after.result(), plain.result()) == [0, 0, 0], (c.id, 'the setting stuck')
        # hold and guard together (k = 2): either flag makes the launch a no-op
        if n == 1023:
            for hold_flag, skip_flag in ((1, 0.0), (0, 1.0), (1, 1.0)):
                got = GG.State(state)
                before = [b.clone() for b in got.bufs]
                w, hold = _window(hold_flag)
                out = torch.tensor([0.37, 1.0, skip_flag, 0.0], dtype=torch.float32, device=DEV)
                with ops.adam_guard(out, torch.zeros(1, dtype=torch.int64, device=DEV)), ops.adam_hold(hold, 2):
                    _call(kind, got, c.step, h, rs, rows, *fresh())
                for b, a in zip(before, got.bufs):
                    assert _eq(a, b), (c.id, hold_flag, skip_flag)
            # both clear: the guarded launch with the coefficient, on the folded scale
            got, want = GG.State(state), GG.State(state)
            w, hold = _window(0)
            out = torch.tensor([0.37, 1.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
            sk = torch.zeros(1, dtype=torch.int64, device=DEV)
            with ops.adam_guard(out, sk), ops.adam_hold(hold, 2):
                _call(kind, got, c.step, h, rs, rows, *fresh())
            with ops.adam_guard(out, sk):
                _call(kind, want, c.step, XC.window_hyper(h, 2), rs, rows, *fresh())
            assert GG._diff(got.result(), want.result()) == [0, 0, 0], c.id
        # hold with a clip coefficient (lirec_set_adam_clip; the table forms then run the template's instantiation, not the
        # hand-written clip kernels): held, no bit moves; not held, the bits of the clipped launch on the folded scale
        if n in (5, 1023):
            cbuf = torch.tensor([0.37], dtype=torch.float32, device=DEV)
            for k in (2, 3):
                got = GG.State(state)
                before = [b.clone() for b in got.bufs]
                cnt, tk = fresh()
                w, hold = _window(1)
                with ops.adam_clip(cbuf), ops.adam_hold(hold, k):
                    _call(kind, got, c.step, h, rs, rows, cnt, tk)
                for b, a in zip(before, got.bufs):
                    assert _eq(a, b), (c.id, k, 'a held clipped launch wrote something')
                assert int(cnt) == c.step - 1 and int(tk) == 0
                got, want = GG.State(state), GG.State(state)
                w, hold = _window(0)
                with ops.adam_clip(cbuf), ops.adam_hold(hold, k):
                    _call(kind, got, c.step, h, rs, rows, *fresh())
                with ops.adam_clip(cbuf):
                    _call(kind, want, c.step, XC.window_hyper(h, k), rs, rows, *fresh())
                assert GG._diff(got.result(), want.result()) == [0, 0, 0], (c.id, k, 'hold + clip')
                assert got.canaries_ok() and float(cbuf) == np.float32(0.37)


@pytest.mark.parametrize('n', [1, 5, 1023, AC.N_BIG])
def test_gated_ema_launch(n):
    r = np.random.default_rng(n)
    e0, p0 = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    w8 = ops.ema_weight(0.9)

    def run(hold_flag):
        s = GG.State((e0, p0, p0, p0))
        before = [b.clone() for b in s.bufs]
        if hold_flag is None:
            ops.ema_step(s.p, s.g, w8)
        else:
            _, hold = _window(hold_flag)
            with ops.adam_hold(hold, 3):
                ops.ema_step(s.p, s.g, w8)
        torch.cuda.synchronize()
        return s, before
    plain, _ = run(None)
    held, before = run(1)
    for b, a in zip(before, held.bufs):
        assert _eq(a, b), 'a held average moved'
    free, _ = run(0)
    assert _eq(free.p, plain.p) and free.canaries_ok() and not _eq(plain.p, before[0][GG.PAD:GG.PAD + n])
    again, _ = run(None)
    assert _eq(again.p, plain.p), 'the setting stuck'


# ---------------------------------------------------------------------------------------------------------------------------
# 3. FusedAdam in the eager loop
# ---------------------------------------------------------------------------------------------------------------------------
def _make(kind='int_rel_ch', seed=11, dropout=0.0, side=True, **flags):
    from lirec_amd import model as M
    config.recipe(kind, joint_dim=16, dropout=dropout, dropout_seed=77, lr=LR, **DIMS,
                  **({} if kind in ('int_ch', 'modalties') else {'rels_n_clips': 3}), **flags)
    opt.device = 'cuda'
    opt.adam_on_side_stream = side
    torch.manual_seed(seed)
    model, loss, optim = M.create_model(11, n_rels=5 if kind != 'modalties' else 0)
    model.train()
    return model, loss, optim


def _batches(kind, n=3):
    from lirec_amd.data import synthetic_batch, to_device_batch
    kw = dict(n_classes=11, n_rels=5 if kind != 'modalties' else 0, **DIMS, **RECIPES[kind])
    return [to_device_batch(synthetic_batch(21 + i, kind, B, **kw), 'cuda') for i in range(n)]


def _micro(model, loss, optim, batch):
    optim.zero_grad()
    lv = loss(model(dict(batch)), batch)
    lv.backward()
    optim.step()
    return lv.detach().reshape(-1)[:1].clone()


def _state(model, optim):
    torch.cuda.synchronize()
    out = TC._state(model, optim)
    return out + ((optim.ema.clone(),) if optim.ema is not None else ())


def _twin_gradient(twin, model, batch):
    """this micro-batch's own gradient at the model's present parameters: a single backward on a zeroed buffer"""
    tm, tl, to = twin
    tm.load_state_dict(model.state_dict())
    to.zero_grad()
    tl(tm(dict(batch)), batch).backward()
    torch.cuda.synchronize()
    return tm.flat_grads(attach=False).clone()


def _steps_of(optim):
    sd = optim.state_dict()
    return [int(sd['state'][i]['step']) for i in sorted(sd['state'])]


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('kind', sorted(RECIPES))
def test_eager_accumulation_in_every_recipe(kind, k):
    """three windows and one open micro-step.  Hold: parameters and moments bit-identical to the window's start.  Apply: every
    element of the three flat buffers within the widened bound of the float64 restatement of the window; p.grad is the fp32 sum of
    the micro-batch gradients.  k = 2: the bits of the idiom one can write without the feature.  state_dict counts windows, goes to
    torch.optim.Adam and back, and a stock Adam in float64 takes the third window's step to the same place within the bound."""
    try:
        model, loss, optim = _make(kind)
        optim.accumulate_steps = k
        twin = _make(kind)
        idiom = _make(kind) if k == 2 else None
        assert optim.accum_phase == 0 and (idiom is None or _eq(idiom[0].flat_params(), model.flat_params()))
        batches = _batches(kind)
        hyper = TC._hyper_of(optim)
        worst, grads, start, stock, acc_worst = [0.0, 0.0, 0.0], [], None, None, 0.0
        optim._ensure_state()
        for j in range(3 * k + 1):
            batch, phase, window = batches[j % len(batches)], j % k, j // k + 1
            assert optim.accum_phase == phase
            if phase == 0:
                grads, start = [], _state(model, optim)
            if window == 3 and phase == 0:
                # a stock Adam in float64 from this state, for the third window's step.  (tests/test_gpu_optim.py holds a step to
                # adam_cases.bounds of the float64 definition, adam_cases.ref64; tests/test_gpu_frozen.py does the same against a stock
                # torch.optim.Adam.  The criterion here is that one: the stock optimiser in float64 IS the definition, fed the
                # float64 sum of the window times gs / k, and the bound is adam_cases.bounds widened as accum_cases derives.)
                sd = optim.state_dict()
                ps = [torch.nn.Parameter(p.detach().double().clone()) for p in model.parameters()]
                stock = torch.optim.Adam(ps, lr=hyper[0], betas=(hyper[1], hyper[2]), eps=hyper[3], weight_decay=hyper[4])
                own = stock.state_dict()
                own['state'] = sd['state']
                stock.load_state_dict(own)
            grads.append(_twin_gradient(twin, model, batch))
            _micro(model, loss, optim, batch)
            after = _state(model, optim)
            # p.grad: the unscaled sum of the window so far, within the fp32 accumulation's own error
            acc = model.flat_grads(attach=False)
            err = (acc.double() - XC.sum64(grads)).abs()
            room = (len(grads) - 1) * AC.U * XC.abs_sum64(grads) + AC.DENORM
            acc_worst = max(acc_worst, float((err / room).max()))
            assert bool((err <= room).all()), (j, 'p.grad is not the unscaled sum of the window so far', float((err / room).max()))
            if phase < k - 1:
                for a, b, what in zip(after, start, 'pmv'):
                    assert _eq(a, b), (j, what, 'a hold step changed bits')
                assert optim._step == window - 1
                continue
            before = start
            use = XC.use_of_window_bounds(after[:3], before[0], grads, before[1], before[2], window, hyper)
            worst = [max(a, b) for a, b in zip(worst, use)]
            assert max(use) <= 1.0, (kind, k, window, use)
            assert optim._step == window and set(_steps_of(optim)) == {window}
            if idiom is not None:
                im, il, io = idiom
                io.grad_scale = 0.5
                io.zero_grad()
                for b2 in (batches[(j - 1) % len(batches)], batch):
                    il(im(dict(b2)), b2).backward()
                io.step()
                torch.cuda.synchronize()
                for a, b, what in zip(after[:3], TC._state(im, io), 'pmv'):
                    assert _eq(a, b), (window, what, 'k = 2 is not the two-backwards idiom')
            if window == 3:
                s64 = XC.sum64(grads) * XC.accum_scale(1.0, k)
                for p, (n, (o, cnt)) in zip(stock.param_groups[0]['params'], ((n, model._offsets[n]) for n, _ in model.named_parameters())):
                    p.grad = s64[o:o + cnt].view(p.shape).clone()
                stock.step()
                _, (bp, _, _) = XC.ref64_window(before[0], grads, before[1], before[2], window, hyper)
                for p, (n, (o, cnt)) in zip(stock.param_groups[0]['params'], ((n, model._offsets[n]) for n, _ in model.named_parameters())):
                    d = (after[0][o:o + cnt].double() - p.detach().reshape(-1)).abs()
                    assert bool((d <= bp[o:o + cnt] * (1 + 1e-9) + 1e-300).all()), (n, float((d / bp[o:o + cnt]).max()))
        assert optim.accum_phase == 1 and optim._step == 3
        GG._torch_round_trip(model, optim, [3] * len(optim._names))
        _fig('eager', recipe=kind, k=k, p=worst[0], m=worst[1], v=worst[2], accumulated_gradient=acc_worst)
    finally:
        config.reset()


def _first_start(model, optim):
    optim._ensure_state()
    return _state(model, optim)


def _variant(name):
    from lirec_amd.optim import FusedAdam
    model, loss, optim = _make('int_rel_ch')
    if name == 'groups':
        optim = FusedAdam(model, lr=LR, param_groups=WC.two_groups(model))
    elif name == 'clip':
        optim.max_grad_norm = 1e-3
    elif name == 'ema':
        optim.ema_decay = 0.9
    elif name == 'frozen':
        dict(model.named_parameters())[GG._l2_weight(model)].requires_grad_(False)
    return model, loss, optim


@pytest.mark.parametrize('name', ['clip', 'frozen', 'groups', 'ema'])
def test_features_on_top_act_at_the_apply_step(name):
    """k = 2, three windows, against the idiom (two backwards, grad_scale 0.5, one plain step of an optimiser with the same
    feature): parameters, moments and the average bit for bit after every window, untouched on every hold.  Clip: the norm is that
    of the accumulated buffer times grad_scale / 2, and it clipped.  Frozen: the slice keeps its bits and its step 0.  EMA: one
    lerp per window."""
    try:
        model, loss, optim = _variant(name)
        im, il, io = _variant(name)
        optim.accumulate_steps = 2
        io.grad_scale = 0.5
        batches = _batches('int_rel_ch')
        optim._ensure_state()
        for w in range(3):
            start = _state(model, optim)
            _micro(model, loss, optim, batches[w % 3])
            for a, b in zip(_state(model, optim), start):
                assert _eq(a, b), (name, w, 'a hold step changed bits')
            _micro(model, loss, optim, batches[(w + 1) % 3])
            io.zero_grad()
            for b2 in (batches[w % 3], batches[(w + 1) % 3]):
                il(im(dict(b2)), b2).backward()
            io.step()
            after, want = _state(model, optim), _state(im, io)
            assert len(after) == len(want) == (4 if name == 'ema' else 3)
            for a, b, what in zip(after, want, 'pmve'):
                assert _eq(a, b), (name, w, what)
            assert not _eq(after[0], start[0])
            if name == 'clip':
                acc = model.flat_grads(attach=False)
                sq = float((acc.double() ** 2).sum())
                coef, norm = CC.coef_of(sq, XC.accum_scale(1.0, 2), 1e-3)
                assert TC._adjacent(optim.grad_norm.cpu().numpy(), norm) and TC._adjacent(optim.clip_coef.cpu().numpy(), coef)
                assert float(optim.clip_coef) < 1.0, 'the bound was meant to clip'
                _fig('clip', window=w + 1, norm=float(optim.grad_norm), coef=float(optim.clip_coef))
            if name == 'frozen':
                o, n = model._offsets[GG._l2_weight(model)]
                for a, b in zip(after, start):
                    assert _eq(a[o:o + n], b[o:o + n])
            if name == 'ema':
                assert optim.ema_updates() == w + 1
        steps = dict(zip([n for grp in optim.group_names() for n in grp], _steps_of(optim)))
        frozen = GG._l2_weight(model) if name == 'frozen' else None
        assert all(s == (0 if n == frozen else 3) for n, s in steps.items()), steps
        GG._torch_round_trip(model, optim, [steps[n] for grp in optim.group_names() for n in grp])
    finally:
        config.reset()


def test_a_nan_in_the_window_skips_the_window_once():
    """k = 3, skip_nonfinite: a NaN planted into the buffer after micro-batch 1 of window 2 stays in the sum; the window's apply step
    changes no bit, found_nonfinite is 1 and ONE step is counted; window 3 applies as the second update"""
    try:
        model, loss, optim = _make('int_rel_ch')
        optim.skip_nonfinite = True
        optim.accumulate_steps = 3
        twin = _make('int_rel_ch')
        batches = _batches('int_rel_ch')
        hyper = TC._hyper_of(optim)
        name = GG._l2_weight(model)
        o, n = model._offsets[name]
        for window in (1, 2, 3):
            start = _first_start(model, optim)
            grads = []
            for j in range(3):
                grads.append(_twin_gradient(twin, model, batches[j]))
                optim.zero_grad()
                loss(model(dict(batches[j])), batches[j]).backward()
                if window == 2 and j == 0:
                    model.flat_grads(attach=False)[o + n // 2] = float('nan')
                optim.step()
                torch.cuda.synchronize()
                if j < 2:
                    for a, b in zip(_state(model, optim), start):
                        assert _eq(a, b)
            after = _state(model, optim)
            if window == 2:
                for a, b in zip(after, start):
                    assert _eq(a, b), 'the skipped window changed bits'
                assert float(optim.found_nonfinite) == 1.0 and int(optim.skipped_steps) == 1
                assert math.isnan(float(model.flat_grads(attach=False)[o + n // 2]))
                continue
            assert float(optim.found_nonfinite) == 0.0 and int(optim.skipped_steps) == (0 if window == 1 else 1)
            use = XC.use_of_window_bounds(after[:3], start[0], grads, start[1], start[2], 1 if window == 1 else 2, hyper)
            assert max(use) <= 1.0, (window, use)
        assert optim.skipped_total() == 1 and set(_steps_of(optim)) == {2}
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. recorded == eager
# ---------------------------------------------------------------------------------------------------------------------------
def _snap(model, optim, lv):
    return _state(model, optim) + (model.flat_grads(attach=False).clone(), lv.detach().reshape(-1)[:1].clone())


def _eager_run(k, n, variant='plain', dropout=0.3):
    model, loss, optim = _build_rec(variant, dropout)
    optim.accumulate_steps = k
    batch = _batches('int_rel_ch', 1)[0]
    return [_snap(model, optim, _micro(model, loss, optim, batch)) for j in range(n)], optim


def _build_rec(variant, dropout=0.3):
    from lirec_amd.optim import FusedAdam
    model, loss, optim = _make('int_rel_ch', dropout=dropout)
    if variant == 'groups':
        optim = FusedAdam(model, lr=LR, param_groups=WC.two_groups(model))
    elif variant == 'ema':
        optim.ema_decay = 0.9
    elif variant == 'frozen':
        dict(model.named_parameters())[GG._l2_weight(model)].requires_grad_(False)
    return model, loss, optim


def _recorded_run(k, n, phase0, variant='plain', eager_at=None, lag=False, dropout=0.3):
    """micro-steps 1 .. phase0 eager, micro-step phase0 + 1 is the recording step (no warm-up), the rest replays -- micro-step
    ``eager_at`` eager between release() and resume().  One batch throughout (a recorded list holds the launch shapes of its batch):
    the micro-batches differ through the dropout key, which every micro-step advances."""
    from lirec_amd.graph import RecordedTrainStep
    model, loss, optim = _build_rec(variant, dropout)
    optim.accumulate_steps = k
    static = _batches('int_rel_ch', 1)[0]
    out, g, held = [], None, None
    try:
        for j in range(n):
            if j < phase0:
                lv = _micro(model, loss, optim, static)
            elif g is None:
                if lag:
                    held = model._wgrad_lane()
                    assert held is not None
                    with held[1]:
                        _lib.lib().lirec_debug_set(131072, -1)
                g = RecordedTrainStep(model, loss, optim, static, warmup=0)
                assert (g.overwrite, g.fused, g.defer, g.accum) == (False, False, False, k)
                lv = g.loss_out
            elif j == eager_at:
                g.release()
                lv = _micro(model, loss, optim, static)
                g.resume()
            else:
                lv = g.step()
            torch.cuda.synchronize()
            assert optim.accum_phase == (j + 1) % k and optim._step == (j + 1) // k
            out.append(_snap(model, optim, lv))
        state, win = g.state.tolist(), g.win.tolist()
        assert state[0] == model._fwd_train_calls and state[1] == state[2] == n // k and win[0] == n % k and win[2] == 0, (state, win)
    finally:
        if held is not None:
            with held[1]:
                _lib.lib().lirec_debug_set(0, -1)
        if g is not None:
            g.release()
    return out, optim


def _agree(eager, rec, what):
    names = ('parameters', 'exp_avg', 'exp_avg_sq') + (('ema',) if len(eager[0]) == 6 else ()) + ('gradient buffer', 'loss')
    assert len(eager) == len(rec)
    for j, (a, b) in enumerate(zip(eager, rec)):
        assert len(a) == len(b) == len(names)
        for x, y, name in zip(a, b, names):
            assert _eq(x, y), (what, 'micro-step %d' % (j + 1), name, int((x != y).sum()))


@pytest.mark.parametrize('phase0', [0, 1])
@pytest.mark.parametrize('k', KS)
def test_recorded_is_eager_bit_for_bit(k, phase0):
    """2k + 1 replays behind the recording step, recorded at phase 0 and at phase 1, one eager step between release() and
    resume() in the middle: parameters, moments, the gradient buffer at every phase and every loss value"""
    try:
        n = phase0 + 1 + 2 * k + 1
        eager, _ = _eager_run(k, n)
        rec, _ = _recorded_run(k, n, phase0, eager_at=phase0 + k + 1)
        _agree(eager, rec, 'k=%d recorded at phase %d' % (k, phase0))
        assert not _eq(eager[-1][0], eager[0][0])
    finally:
        config.reset()


@pytest.mark.parametrize('variant', ['groups', 'frozen', 'ema'])
def test_recorded_is_eager_with_groups_frozen_parameters_and_the_average(variant):
    try:
        eager, eo = _eager_run(2, 6, variant)
        rec, ro = _recorded_run(2, 6, 1, variant)
        _agree(eager, rec, variant)
        if variant == 'ema':
            assert eo.ema_updates() == ro.ema_updates() == 3
    finally:
        config.reset()


def test_recorded_is_eager_with_the_side_stream_held_back():
    """the weight-gradient side stream of every replay starts ~2 ms late (lirec_debug_set bit 131072 in that stream's library
    context): the head launch of the next micro-step, and the gated update, are ordered behind it by the step's own join"""
    try:
        eager, _ = _eager_run(2, 6)
        rec, _ = _recorded_run(2, 6, 0, lag=True)
        _agree(eager, rec, 'lagging side stream')
    finally:
        config.reset()


def test_recorded_accumulation_refuses_clip_and_guard_and_the_pipeline_form():
    from lirec_amd.graph import RecordedTrainStep
    try:
        model, loss, optim = _make('int_rel_ch')
        optim.accumulate_steps = 2
        batch = _batches('int_rel_ch', 1)[0]
        _micro(model, loss, optim, batch)
        _micro(model, loss, optim, batch)
        for kw, word in ((dict(max_grad_norm=1.0), 'max_grad_norm'), (dict(skip_nonfinite=True), 'skip_nonfinite')):
            for a, v in kw.items():
                setattr(optim, a, v)
            with pytest.raises(_lib.LirecError, match=word):
                RecordedTrainStep(model, loss, optim, batch, warmup=0)
            optim.max_grad_norm, optim.skip_nonfinite = None, False
            assert optim._win_dev is None and optim._step_dev is None and model._seed_dev is None
        with pytest.raises(_lib.LirecError, match='accumulation'):
            RecordedTrainStep(model, loss, optim, batch, warmup=0, next_batch=dict(batch))
        assert optim.arm_first_layer_update() is False
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. training()
# ---------------------------------------------------------------------------------------------------------------------------
class _Counting:
    def __init__(self):
        self.calls = 0

    def step(self):
        self.calls += 1


def _world(tmp_path, mode, k):
    """three epochs of five batches (the last one short) over a resident block store, accumulate_steps = k: 15 micro-batches, so a
    window crosses every epoch's end and one micro-batch is left in an open window"""
    import test_gpu_blockstore_recorded as BR
    from lirec_amd import blockstore as BS
    from lirec_amd.data import SyntheticMixedFeaturesDataset
    kw, R = BR.RECIPES['int_rels']
    model, loss, optim = BR._model('int_rels', R, batch_size=5, num_workers=0, epochs=3, test_fr=1000, store_root=str(tmp_path),
                                   save_model=False, record_block_store=mode, accumulate_steps=k)
    assert optim.accumulate_steps == k
    ds = BS.ResidentBlockDataset(SyntheticMixedFeaturesDataset('int_rels', 24, seed=31, soft_gt=opt.soft_gt, **kw))
    return model, loss, optim, ds, BR._UpdatingSampler(24)


def _by_hand(tmp_path, k):
    """the loop a user writes, over the loader and the sampler training() draws with: the stock three lines on every batch, a
    one-label batch skipped, the evaluation training() runs behind epoch 0, a counting scheduler stepped where an update was
    applied, the trailing partial window dropped.  No _Stepper, no recording."""
    from lirec_amd.loader import make_loader
    from lirec_amd.test import testing
    model, loss, optim, ds, sampler = _world(tmp_path, '', k)
    loader = make_loader(ds, opt.batch_size, shuffle=False, sampler=sampler)
    to_dev = getattr(ds, 'to_device', None)
    updates, micro = 0, 0
    for epoch in range(opt.epochs):
        model.train()
        ds.epoch = epoch
        for batch in loader:
            if to_dev is not None:
                batch = to_dev(batch)
            if len(batch['labels']) == 1:
                continue
            optim.zero_grad()
            loss(model(batch), batch).backward()
            optim.step()
            micro += 1
            updates += micro % k == 0
        if epoch % opt.test_fr == 0:
            testing(ds, model, loss, total_iter=epoch, mode='train', train_start_time='by hand', verbose=False)
    optim.drop_window()
    torch.cuda.synchronize()
    return {'params': model.flat_params().clone(), 'm': optim._m.clone(), 'v': optim._v.clone(), 'step': optim._step,
            'phase': optim.accum_phase, 'micro': micro, 'updates': updates}


def _train(monkeypatch, tmp_path, mode, k):
    """training() over that world under ``opt.record_block_store = mode``"""
    from lirec_amd import train
    model, loss, optim, ds, sampler = _world(tmp_path, mode, k)
    lines, sched = [], _Counting()
    monkeypatch.setattr(train, '_print', lambda *a, **kw2: lines.append(' '.join(str(x) for x in a)))
    train.training(ds, model=model, loss=loss, optimizer=optim, sampler=sampler, scheduler=sched)
    torch.cuda.synchronize()
    last = train.training.last
    return {'params': model.flat_params().clone(), 'm': optim._m.clone(), 'v': optim._v.clone(), 'step': optim._step,
            'phase': optim.accum_phase, 'sched': sched.calls, 'replays': last['replays'],
            'losses': [l for l in lines if l.startswith('loss: ')], 'said': [l for l in lines if 'not used' in l]}


def test_training_accumulates_across_epochs_eager_bind_and_list(monkeypatch, tmp_path):
    """training() with opt.record_block_store '' (every step eager), 'bind' and 'list' (recorded on the fourth batch, i.e. at
    phase 1; eight replays, an eager short batch inside each epoch) against the loop written by hand (_by_hand): the same
    parameter and moment bits in all three; the scheduler stepped once per applied window, as often as the hand-written loop
    applied one; the trailing micro-batch dropped; the three modes print the same losses"""
    try:
        hand = _by_hand(tmp_path, 2)
        assert (hand['micro'], hand['updates'], hand['step'], hand['phase']) == (15, 7, 7, 0)
        runs = {mode: _train(monkeypatch, tmp_path, mode, 2) for mode in ('', 'bind', 'list')}
        ref = runs['']
        assert ref['replays'] == 0 and len(ref['losses']) == 3
        for mode in ('', 'bind', 'list'):
            r = runs[mode]
            assert not r['said'], r['said']
            assert r['replays'] == (0 if mode == '' else 8), (mode, r['replays'])
            assert r['step'] == hand['step'] and r['sched'] == hand['updates'] and r['phase'] == 0, (mode, r['step'], r['sched'])
            for key in ('params', 'm', 'v'):
                assert torch.equal(r[key], hand[key]), (mode, key, int((r[key] != hand[key]).sum()))
            assert r['losses'] == ref['losses']
        plain = _train(monkeypatch, tmp_path, '', 1)
        assert plain['step'] == 15 and plain['sched'] == 15 and not torch.equal(plain['params'], ref['params'])
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. accumulate_steps = 1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['eager', 'recorded'])
def test_one_is_off(route):
    """five steps with accumulate_steps=1 by keyword against an optimiser built without the argument: parameters and moments bit
    for bit; recorded: the same commands on the same streams, the same flags"""
    from lirec_amd.graph import RecordedTrainStep
    from lirec_amd.optim import FusedAdam
    try:
        got = []
        for keyword in (False, True):
            model, loss, optim = _make('int_rel_ch', dropout=0.3)
            if keyword:
                optim = FusedAdam(model, lr=LR, weight_decay=opt.weight_decay, accumulate_steps=1)
            batch = _batches('int_rel_ch', 1)[0]
            cmds = None
            if route == 'eager':
                for _ in range(5):
                    _micro(model, loss, optim, batch)
            else:
                g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
                try:
                    for _ in range(3):
                        g.step()
                    lanes = {}
                    cmds = ([(lanes.setdefault(s, len(lanes)), c) for s, c in (g.cmds.command(i) for i in range(g.cmds.size))],
                            (g.overwrite, g.fused, g.defer), g.hyper_key(optim))
                finally:
                    g.release()
            assert optim._step == 5 and optim.accum_phase == 0 and optim._win_dev is None
            got.append((_state(model, optim), cmds))
        for a, b, what in zip(got[0][0], got[1][0], 'pmv'):
            assert _eq(a, b), (route, what)
        assert got[0][1] == got[1][1]
    finally:
        config.reset()
