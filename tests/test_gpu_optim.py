"""The update side of the step against float64, on every route: lirec_adam_step with the step from the host and from a device
counter (`step_dev`), lirec_adam_step_counted (the side stream's own step counter, its ticket and `advance`), the zeroing /
counter launches in front of a step (lirec_zero_count, lirec_counter_add, lirec_memset_zero), and FusedAdam.step() as a whole --
every element of the flat buffers exactly one update per step -- on its plain, side-stream and recorded routes (the last one with
the first-layer bucket folded into the weight-gradient reduce, lirec_fused_adam; tests/test_gpu_layer1_persistent.py pins that
launch to ops.adam_step bit for bit).

Yardstick and bounds: tests/adam_cases.py (ref64, and 16 u of the update's own terms per output; tests/test_host_optim.py shows
that a correct fp32 implementation uses less than half of each).  Sizes: 1, 3, 4, 5 (the float4 body and the scalar tail on their
own), 1023, and 2 x 2 097 152 + 3 x 1024 + 3 -- the launch is capped at 2048 workgroups x 256 threads x 4 elements, so that size
takes the grid-stride loop round twice, a partial third time, and leaves a tail of three.  The state are slices of larger buffers
at different multiples of 16 bytes, with 64 guard elements on both sides that must keep their bits.

Measured on an MI355X -- the worst |kernel - ref64| as a fraction of its bound over all cases of a route, for p' / m' / v' (the
fp32 restatement on the host: 0.30 / 0.19 / 0.32):
  lirec_adam_step, host step        0.30 / 0.17 / 0.32    (n = 4 197 379: 0.30 / 0.13 / 0.32; n <= 5: at most 0.08 / 0.17 / 0.24)
  lirec_adam_step, step_dev         0.30 / 0.17 / 0.32
  lirec_adam_step_counted           0.30 / 0.07 / 0.23
  FusedAdam.step(), plain and side  0.26 / 0.07 / 0.29    (18 431 616 elements x 6 steps; the two routes: the same figures)
  FusedAdam.step(), recorded        0.26 / 0.07 / 0.27    (the replays of steps 4 - 6; the eager routes' figures at those steps)
Bit for bit against ref32 (host step): 0 differing elements in every case at every size -- the kernel IS the fp32 restatement.
step_dev against the host-step call of the same step: 0 differing elements in all 20 (hyper-parameter set, step) pairs at n = 5 and
1023 and in the four cases at n = 4 197 379 -- the device's pow / sqrt gave the host's float here; not asserted (a neighbouring
float would be as good an answer).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_cases as AC
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
CANARY = 1234.5


def _fig(what, **kw):
    """a measured figure, printed before anything is asserted on it"""
    print('OPTIM-FIGURE %s %s' % (what, ' '.join('%s=%s' % (k, ('%.4f' % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


class Placed:
    """p, m, v as slices [a : a + n] of larger canary-filled buffers (a: another multiple of 4 for each), g in a buffer of its own"""

    def __init__(self, state, leads=(64, 68, 76)):
        p, g, m, v = state
        self.n = n = p.size
        self.bufs, self.views, self.leads = [], [], leads
        for arr, a in zip((p, m, v), leads):
            buf = torch.full((a + n + GUARD + 5,), CANARY, device=DEV)
            buf[a:a + n] = torch.from_numpy(arr).to(DEV)
            self.bufs.append(buf); self.views.append(buf[a:a + n])
            assert buf[a:a + n].data_ptr() % 16 == 0
        self.g = torch.from_numpy(g).to(DEV)
        self.p, self.m, self.v = self.views
        self.state0 = tuple(t.clone() for t in (self.p, self.g, self.m, self.v))

    def guards_untouched(self):
        for buf, a, what in zip(self.bufs, self.leads, 'pmv'):
            front, back = buf[a - GUARD:a], buf[a + self.n:a + self.n + GUARD]
            assert bool((front == CANARY).all()) and bool((back == CANARY).all()), 'guard elements of %s were written' % what
        assert torch.equal(self.g, self.state0[1]), 'the gradient was written'

    def result(self):
        return self.p, self.m, self.v


def _cases_at(n):
    return AC.CASES if n < AC.N_BIG else AC.BIG_CASES


# ---------------------------------------------------------------------------------------------------------------------------
# lirec_adam_step, the step from the host
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', AC.SIZES)
def test_adam_step_is_the_float64_update_within_the_bounds_and_the_fp32_restatement_bit_for_bit(n):
    """Every case of the grid (at the large size: one per hyper-parameter set): |kernel - ref64| within the bounds for p', m', v';
    the guards keep their bits; and the kernel's bits are those of ref32 -- each operation is IEEE single precision, contraction
    is off, and the fp32 divide and square root are correctly rounded, so nothing is left to differ."""
    worst, differ = [0.0, 0.0, 0.0], 0
    for c in _cases_at(n):
        h = AC.hyper32(c.hyper)
        state = AC.make_state(c, n)
        pl = Placed(state)
        ops.adam_step(pl.p, pl.g, pl.m, pl.v, c.step, *h)
        torch.cuda.synchronize()
        pl.guards_untouched()
        use = AC.use_of_bounds(pl.result(), *pl.state0, c.step, h)
        want = AC.ref32(*state, c.step, h)
        d = [int((_bits(x) != w.view(np.uint32)).sum()) for x, w in zip(pl.result(), want)]
        _fig('host_step', n=n, case=c.id, p=use[0], m=use[1], v=use[2], bits_differ=sum(d))
        assert all(bool(torch.isfinite(x).all()) for x in pl.result()), c.id
        assert max(use) <= 1.0, (c.id, use)
        worst = [max(a, b) for a, b in zip(worst, use)]
        differ += sum(d)
        assert d == [0, 0, 0], (c.id, 'elements whose bits differ from the fp32 restatement (p, m, v)', d)
    _fig('host_step_worst', n=n, p=worst[0], m=worst[1], v=worst[2], bits_differ=differ)


# ---------------------------------------------------------------------------------------------------------------------------
# the step read from a device counter
# ---------------------------------------------------------------------------------------------------------------------------
# every hyper-parameter set at every step (the first case of the grid that has the pair)
STEP_DEV_CASES = [next(c for c in AC.CASES if (c.hyper, c.step) == (hh, t)) for hh in range(len(AC.HYPERS)) for t in AC.STEPS]


@pytest.mark.parametrize('n', [5, 1023, AC.N_BIG])
def test_step_from_a_device_counter_is_the_float64_update_of_that_step(n):
    """`step_dev` holds the step, `step` another one: the device's value counts.  Within the bounds of ref64 at that step.  Against
    the host-step call of the same step the bias corrections come from the device's double-precision pow / sqrt instead of the
    host's and may round to a neighbouring float: not compared bit for bit; the number of differing elements is reported."""
    cases = STEP_DEV_CASES if n < AC.N_BIG else AC.BIG_CASES
    assert n == AC.N_BIG or {(c.hyper, c.step) for c in cases} == {(hh, t) for hh in range(4) for t in AC.STEPS}
    worst, differ = [0.0, 0.0, 0.0], {}
    for c in cases:
        h = AC.hyper32(c.hyper)
        state = AC.make_state(c, n)
        pl, host = Placed(state), Placed(state)
        sd = torch.tensor([c.step], dtype=torch.int64, device=DEV)
        ops.adam_step(pl.p, pl.g, pl.m, pl.v, 2 if c.step == 1 else 1, *h, step_dev=sd)
        ops.adam_step(host.p, host.g, host.m, host.v, c.step, *h)
        torch.cuda.synchronize()
        pl.guards_untouched()
        assert int(sd) == c.step
        use = AC.use_of_bounds(pl.result(), *pl.state0, c.step, h)
        d = sum(int((_bits(a) != _bits(b)).sum()) for a, b in zip(pl.result(), host.result()))
        differ[c.id] = d
        _fig('step_dev', n=n, case=c.id, p=use[0], m=use[1], v=use[2], differ_from_host_step=d)
        assert max(use) <= 1.0, (c.id, use)
        worst = [max(a, b) for a, b in zip(worst, use)]
    _fig('step_dev_worst', n=n, p=worst[0], m=worst[1], v=worst[2], differ_from_host_step=sum(differ.values()),
         cases_that_differ=sum(1 for d in differ.values() if d))


def test_step_dev_without_a_host_step():
    """step = 0 is accepted when the device holds the step (the recorded step's form)"""
    c = AC.Case(0, 3, 1.0)
    h = AC.hyper32(c.hyper)
    state = AC.make_state(c, 1023)
    a, b = Placed(state), Placed(state)
    sd = torch.tensor([7], dtype=torch.int64, device=DEV)
    ops.adam_step(a.p, a.g, a.m, a.v, 0, *h, step_dev=sd)
    ops.adam_step(b.p, b.g, b.m, b.v, 3, *h, step_dev=sd)
    torch.cuda.synchronize()
    assert max(AC.use_of_bounds(a.result(), *a.state0, 7, h)) <= 1.0
    assert all(torch.equal(x, y) for x, y in zip(a.bufs, b.bufs))


# ---------------------------------------------------------------------------------------------------------------------------
# lirec_adam_step_counted
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k', [(1, 0), (1023, 0), (1023, 999), (AC.N_BIG, 2)])
def test_counted_step_is_the_counter_plus_one_and_advances_once_per_chain(n, k):
    """Three adjacent sub-ranges of one buffer, `advance` on the last call only: all three take step k + 1 -- the bits of the
    step_dev = k + 1 call --, the counter reads k until the last call has run and k + 1 after it, the ticket is back at 0 after
    every call (n = 1: one workgroup; the large size: 2048).  A second chain takes k + 2.  With advance = 0 throughout, the
    counter stays."""
    c = AC.Case(0, 3, 1.0)
    h = AC.hyper32(c.hyper)
    r4 = lambda x: (x + 3) // 4 * 4
    sizes = [n, min(n, 1023), n]
    starts = [GUARD]
    for s in sizes[:-1]:
        starts.append(starts[-1] + r4(s))                 # (up to three elements between two sub-ranges belong to nobody)
    L = starts[-1] + sizes[-1] + GUARD
    p0, g0, m0, v0 = (torch.from_numpy(a).to(DEV) for a in AC.make_state(c, L))
    got = [p0.clone(), m0.clone(), v0.clone()]
    want = [p0.clone(), m0.clone(), v0.clone()]
    count = torch.tensor([k], dtype=torch.int64, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)

    def chain(advance_last, step):
        for i, (a, s) in enumerate(zip(starts, sizes)):
            before = int(count)
            adv = advance_last and i == len(sizes) - 1
            ops.adam_step_counted(got[0][a:a + s], g0[a:a + s], got[1][a:a + s], got[2][a:a + s], *h, count, ticket, advance=adv)
            torch.cuda.synchronize()
            assert int(ticket) == 0, 'the ticket is not back at 0 after call %d' % i
            assert int(count) == before + (1 if adv else 0), ('the counter after call %d' % i, int(count), before, adv)
            assert before == step - 1
        sd = torch.tensor([step], dtype=torch.int64, device=DEV)
        for a, s in zip(starts, sizes):
            ops.adam_step(want[0][a:a + s], g0[a:a + s], want[1][a:a + s], want[2][a:a + s], 0, *h, step_dev=sd)
        torch.cuda.synchronize()
        for x, y, what in zip(got, want, 'pmv'):
            assert torch.equal(x, y), (what, 'counted chain differs from step_dev = %d' % step, int((x != y).sum()))

    a, s = starts[0], sizes[0]
    chain(True, k + 1)
    use = AC.use_of_bounds([t[a:a + s] for t in got], p0[a:a + s], g0[a:a + s], m0[a:a + s], v0[a:a + s], k + 1, h)
    _fig('counted', n=n, k=k, p=use[0], m=use[1], v=use[2])
    assert max(use) <= 1.0, use
    assert int(count) == k + 1
    chain(True, k + 2)
    assert int(count) == k + 2
    chain(False, k + 3)
    assert int(count) == k + 2 and int(ticket) == 0
    # nothing outside the three sub-ranges was written
    inside = torch.zeros(L, dtype=torch.bool, device=DEV)
    for a, s in zip(starts, sizes):
        inside[a:a + s] = True
    for x, x0, what in zip(got, (p0, m0, v0), 'pmv'):
        assert torch.equal(x[~inside], x0[~inside]), what + ': written outside the sub-ranges'
        assert bool((x[inside] != x0[inside]).any())


# ---------------------------------------------------------------------------------------------------------------------------
# lirec_zero_count, lirec_counter_add, lirec_memset_zero
# ---------------------------------------------------------------------------------------------------------------------------
# zero_count_kernel: 2048 workgroups x 256 threads, four 16-byte words per thread and unrolled iteration (2 097 152 words), then one
# word per thread and remainder iteration (524 288), then up to 15 single bytes.  The last size: one unrolled iteration, two
# remainder iterations and 100 words of a third, seven bytes.
BYTES = [0, 1, 15, 16, 17, 4096 + 5, (6 * 524288 + 100) * 16 + 7]
FILL = 0xA5
CTR0 = [5, 2 ** 40 + 3, -2 ** 35, 7, 11, 13]
INCS = [-3, 2 ** 33 + 1, -(2 ** 34), 2 ** 61]


def _filled(nbytes, lead=256):
    buf = torch.full((lead + nbytes + 256,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[lead:lead + nbytes]


def _zeroed_and_guards_kept(buf, nbytes, lead=256):
    assert not bool(buf[lead:lead + nbytes].any()), 'bytes of the range left unzeroed'
    assert bool((buf[:lead] == FILL).all()) and bool((buf[lead + nbytes:] == FILL).all()), 'bytes outside the range were written'


@pytest.mark.parametrize('nc', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('nbytes', BYTES)
def test_zero_count_zeroes_the_range_and_adds_to_the_counters_exactly(nbytes, nc):
    buf, view = _filled(nbytes)
    assert nbytes == 0 or view.data_ptr() % 16 == 0
    ctr = torch.tensor(CTR0, dtype=torch.int64, device=DEV)
    ops.zero_count(view, ctr if nc else None, INCS[:nc])
    torch.cuda.synchronize()
    _zeroed_and_guards_kept(buf, nbytes)
    assert ctr.tolist() == [c + i for c, i in zip(CTR0, INCS[:nc])] + CTR0[nc:]


def test_zero_count_with_no_increments_leaves_given_counters_alone():
    """n = 0 with a counter pointer all the same (ops.zero_count passes NULL then; the C call is made directly here)"""
    buf, view = _filled(4096 + 5)
    ctr = torch.tensor(CTR0, dtype=torch.int64, device=DEV)
    arr = (C.c_int64 * 4)(*INCS)
    rc = _lib.lib().lirec_zero_count(view.data_ptr(), view.numel(), ctr.data_ptr(), arr, 0, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0 and ctr.tolist() == CTR0
    _zeroed_and_guards_kept(buf, 4096 + 5)


@pytest.mark.parametrize('nc', [1, 2, 3, 4])
def test_counter_add_is_exact_and_ordered_on_its_stream(nc):
    """negative increments, values above 2^32 on both sides, and two launches back to back on one stream (the second reads what
    the first wrote)"""
    ctr = torch.tensor(CTR0, dtype=torch.int64, device=DEV)
    ops.counter_add(ctr, INCS[:nc])
    ops.counter_add(ctr, INCS[:nc])
    torch.cuda.synchronize()
    assert ctr.tolist() == [c + 2 * i for c, i in zip(CTR0, INCS[:nc])] + CTR0[nc:]
    # ... the same through the zeroing launch, twice, and mixed with the plain one
    buf, view = _filled(4096 + 5)
    ops.zero_count(view, ctr, [-i for i in INCS[:nc]])
    ops.counter_add(ctr, [1] * nc)
    ops.zero_count(view, ctr, [-i for i in INCS[:nc]])
    torch.cuda.synchronize()
    assert ctr.tolist() == [c + 1 for c in CTR0[:nc]] + CTR0[nc:]
    _zeroed_and_guards_kept(buf, 4096 + 5)


@pytest.mark.parametrize('lead', [256, 259])
@pytest.mark.parametrize('nbytes', BYTES)
def test_memset_zero_zeroes_the_range_only(nbytes, lead):
    """lirec_memset_zero has no alignment requirement: also from an odd address"""
    buf, view = _filled(nbytes, lead)
    ops.zero_(view)
    torch.cuda.synchronize()
    _zeroed_and_guards_kept(buf, nbytes, lead)


# ---------------------------------------------------------------------------------------------------------------------------
# FusedAdam.step(): every element of the flat buffers once per step, on every route
# ---------------------------------------------------------------------------------------------------------------------------
B, T, R = 4, 8, 18
LR = 1e-3                     # (one update is thousands of bound widths: an element updated twice, or not at all, cannot hide)
EAGER_STEPS, WARMUP, REPLAYS = 6, 2, 3
_routes = {}


def _fresh(side):
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
    assert optim.param_groups[0]['lr'] == LR
    return model, loss, optim, batch


def _hyper_of(optim):
    g = optim.param_groups[0]
    return AC.hyper32((g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], optim.grad_scale))


def _check_step(route, step, before, grad, after, hyper):
    """every element of the new flat / m / v, alignment gaps included, against ref64 of the snapshot"""
    use = AC.use_of_bounds(after, before[0], grad, before[1], before[2], step, hyper)
    _fig('route', route=route, step=step, n=before[0].numel(), p=use[0], m=use[1], v=use[2])
    assert max(use) <= 1.0, (route, step, use)
    # (what the comparison can see: where there is a gradient, the typical update is hundreds of bound widths)
    pn, _, _, G, A, V = AC.ref64(before[0], grad, before[1], before[2], step, hyper)
    widths = (pn - before[0].double()).abs() / AC.bounds(before[0], before[1], G, A, V)[0]
    assert float(widths[grad != 0].median()) > 100
    return use


def _run_route(route):
    """[(flat, m, v) after step s], s = 1 .. EAGER_STEPS, of the route (the recorded one: from its last recording step on)"""
    if route in _routes:
        if isinstance(_routes[route], BaseException):
            raise _routes[route]              # (a route that failed is not run a second time)
        return _routes[route]
    try:
        _routes[route] = _run_route_once(route)
    except BaseException as e:
        _routes[route] = e
        raise
    return _routes[route]


def _shadow_is_current(model):
    """the q32b copy of every first-layer weight == lirec_to_q32b of the weight as it is now.  Only the fused reduce writes the
    copy from the NEW weights: a step whose first-layer bucket went through lirec_adam_step leaves it at the old ones."""
    pd = dict(model.named_parameters())
    assert model._w1q_valid and len(model._w1q) == 8
    base = model._w1q_buf.data_ptr()
    for n, addr in model._w1q.items():
        ref = ops.to_q32b(pd[n].data.contiguous()).data
        k = 4 * pd[n].numel()
        assert torch.equal(model._w1q_buf[addr - base:addr - base + k], ref[:k]), 'q32b shadow of %s is stale' % n


def _run_route_once(route):
    out = {}
    try:
        model, loss, optim, batch = _fresh(side=route != 'plain')
        hyper = None
        if route != 'recorded':
            for s in range(1, EAGER_STEPS + 1):
                optim.zero_grad()
                lv = loss(model(dict(batch)), batch)
                lv.backward()
                optim._ensure_state()
                torch.cuda.synchronize()
                hyper = hyper or _hyper_of(optim)
                before = tuple(t.clone() for t in (model.flat_params(), optim._m, optim._v))
                grad = model.flat_grads(attach=False).clone()
                optim.step()
                torch.cuda.synchronize()
                assert bool(model.lanes.bucket0_on_side) == (route == 'side'), 'the step took another route'
                assert optim._step == s
                after = tuple(t.clone() for t in (model.flat_params(), optim._m, optim._v))
                _check_step(route, s, before, grad, after, hyper)
                out[s] = after
        else:
            from lirec_amd.graph import RecordedTrainStep
            # (did the backward of each step taken while recording fold the armed first-layer update in?  The flag is consumed by
            #  optim.step(): read it in front of it)
            applied, step0 = [], optim.step
            optim.step = lambda *a, **k: (applied.append(bool(model.lanes.fold_applied)), step0(*a, **k))[1]
            try:
                g = RecordedTrainStep(model, loss, optim, batch, warmup=WARMUP)
            finally:
                del optim.step
            try:
                # the recording step -- the one the replays re-issue -- took the fused update: its backward says so, and the
                # shadow of the first-layer weights, which an update from optim.step() would have marked stale, is valid
                assert len(applied) == WARMUP + 1 and applied[-1], applied
                assert getattr(model, '_w1q_valid', False), 'the recording step updated the first layers from optim.step()'
                torch.cuda.synchronize()
                hyper = _hyper_of(optim)
                # the recorded step is the one with everything folded in: gradients overwrite their buffer, the first-layer bucket
                # is updated by the launch that reduces its gradient (lirec_fused_adam, reading the step from the device), and
                # the first bucket by the counted launch on the side stream
                assert g.overwrite and g.fused and g.defer, (g.overwrite, g.fused, g.defer)
                assert optim._step_dev is not None and model.lanes.step_side_dev is not None and model.lanes.bucket0_on_side
                assert optim._step == WARMUP + 1
                out[optim._step] = tuple(t.clone() for t in (model.flat_params(), optim._m, optim._v))
                for _ in range(REPLAYS):
                    before = tuple(t.clone() for t in (model.flat_params(), optim._m, optim._v))
                    g.step()
                    torch.cuda.synchronize()
                    s = optim._step
                    # the shared step counter and the side stream's own both stand at this step: the counted launch advanced its
                    # counter exactly once
                    assert g.state.tolist() == [model._fwd_train_calls, s, s], (g.state.tolist(), s)
                    assert int(model.lanes.side_ticket) == 0
                    _shadow_is_current(model)      # (written by this replay's fused reduce from the weights it has just updated)
                    grad = model.flat_grads(attach=False).clone()       # (the fused reduce still stores the gradient)
                    after = tuple(t.clone() for t in (model.flat_params(), optim._m, optim._v))
                    _check_step(route, s, before, grad, after, hyper)
                    out[s] = after
            finally:
                g.release()
    finally:
        config.reset()
    return out


@pytest.mark.parametrize('route', ['plain', 'side', 'recorded'])
def test_every_element_is_updated_once_per_step(route):
    out = _run_route(route)
    assert len(out) == (EAGER_STEPS if route != 'recorded' else REPLAYS + 1)


def test_the_routes_agree_bit_for_bit():
    """the side stream moves launches and changes no number; the recorded step is the eager step (both pinned at the bench shape by
    tests/test_gpu_recorded_bench_shape.py) -- here for parameters AND both moments, after every step"""
    plain, side, rec = (_run_route(r) for r in ('plain', 'side', 'recorded'))
    for s in sorted(plain):
        for a, b, what in zip(plain[s], side[s], ('parameters', 'exp_avg', 'exp_avg_sq')):
            assert torch.equal(a, b), ('plain vs side stream', s, what, int((a != b).sum()))
    assert sorted(rec) == list(range(WARMUP + 1, WARMUP + 1 + REPLAYS + 1))
    for s in sorted(rec):
        for a, b, what in zip(side[s], rec[s], ('parameters', 'exp_avg', 'exp_avg_sq')):
            assert torch.equal(a, b), ('eager vs recorded', s, what, int((a != b).sum()))
