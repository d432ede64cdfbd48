"""Parameter groups and device-resident hyper-parameters on the GPU (include/lirec_hip.h, "parameter groups"; lirec_amd/optim.py):
lirec_adam_step_groups against float64 and, bit for bit, against lirec_adam_step_ranges called once per group with that group's
values by value; the table read anew by every launch; FusedAdam with three groups on its plain, side-stream and recorded routes;
one group with device_hyper against the by-value path; a learning-rate schedule through ONE recording in the headline form, also
with the side stream held back (the test of the per-stream tables); off is off; groups with a frozen parameter and with clipping.

Bounds: adam_cases.bounds, unchanged -- tests/test_host_groups.py shows the fp32 restatement inside them for every kernel case
here (largest use 0.27) and the float64 yardstick equal to torch.optim.Adam in float64 (2e-14 relative).  A whole FusedAdam step is
checked as tests/test_gpu_optim.py checks it: ref64 fed the device's own gradients, step by step.

The models have 38 parameters, so no frozen set gives 65 ranges: the 64-per-call chunking of FusedAdam._update is exercised with a
stand-in model of 140 small parameters (alternate ones frozen, three groups: 70 ranges, two calls) through FusedAdam.step() in all
three step forms -- by value, step_dev, and counted on a side stream the stand-in hands to step() -- not through a model's routes.

The recorded command lists are compared as (stream, command kind) sequences: lirec_cmdlist_command gives no kernel symbol, so "the
same kernels" is shown by the same bits on every step together with the same sequence, as tests/test_gpu_clip.py does it."""
import ctypes

import numpy as np
import pytest
import torch

import adam_cases as AC
import clip_cases as CC
import group_cases as GC
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt
from lirec_amd.lanes import Lane, StepLanes
from lirec_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _fig(what, **kw):
    print('GROUP-FIGURE %s %s' % (what, ' '.join('%s=%s' % (k, ('%.4g' % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(a, b):
    if torch.is_tensor(a) and torch.is_tensor(b):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    a, b = (_np(x) if torch.is_tensor(x) else x for x in (a, b))
    return np.array_equal(_bits(a), _bits(b))


def _table(rows):
    t = torch.full((8 * _lib.ADAM_MAX_GROUPS,), float('nan'), dtype=torch.float32, device=DEV)
    ops.adam_hyper_write(t, rows)
    return t


class Bufs:
    def __init__(self, state):
        self.p, self.g, self.m, self.v = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in state)
        assert all(t.data_ptr() % 16 == 0 for t in (self.p, self.g, self.m, self.v))

    def result(self):
        torch.cuda.synchronize()
        return _np(self.p), _np(self.m), _np(self.v)


def _per_group_by_value(b, rs, rows, step, grad_scale):
    """the existing kernel: lirec_adam_step_ranges with step_dev, once per group, that group's values by value"""
    step_dev = torch.tensor([step], dtype=torch.int64, device=DEV)
    for grp in sorted({r[3] for r in rs}):
        mine = [(o, k, lag) for o, k, lag, g_ in rs if g_ == grp]
        ops.adam_step_ranges(b.p, b.g, b.m, b.v, mine, 0, *rows[grp], grad_scale, step_dev=step_dev)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lirec_adam_step_groups
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [False, True], ids=['unclipped', 'clipped'])
@pytest.mark.parametrize('form', ['by_value', 'step_dev', 'counted'])
@pytest.mark.parametrize('step', GC.STEPS)
def test_adam_step_groups_against_float64_and_the_existing_kernel(step, form, clip):
    state, rs = GC.build(step)
    if form == 'by_value' and step == 1:
        # (a by-value step minus the lag must be >= 1 -- as for lirec_adam_step_ranges: refused, and run with every lag 0; the
        #  device forms count a step below 1 as 1 and run the case as it is)
        bad = Bufs(state)
        with pytest.raises(Exception):
            ops.adam_step_groups(bad.p, bad.g, bad.m, bad.v, rs, _table(GC.ROWS), 3, step, GC.GRAD_SCALE)
        assert all(_same(a, b) for a, b in zip(bad.result(), (state[0], state[2], state[3])))
        rs = [(o, k, 0, grp) for o, k, _, grp in rs]
    coef = GC.COEF if clip else 1.0
    cbuf = torch.tensor([coef], dtype=torch.float32, device=DEV) if clip else None
    got, want = Bufs(state), Bufs(state)
    table = _table(GC.ROWS)
    count = ticket = None
    with ops.adam_clip(cbuf):
        if form == 'by_value':
            ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, table, 3, step, GC.GRAD_SCALE)
        elif form == 'step_dev':
            sd = torch.tensor([step], dtype=torch.int64, device=DEV)
            ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, table, 3, 0, GC.GRAD_SCALE, step_dev=sd)
        else:
            count = torch.tensor([step - 1], dtype=torch.int64, device=DEV)
            ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, table, 3, 0, GC.GRAD_SCALE, count_dev=count, ticket=ticket, advance=True)
        _per_group_by_value(want, rs, GC.ROWS, step, GC.GRAD_SCALE)
    res, ref = got.result(), want.result()
    if form == 'counted':
        assert int(count) == step and int(ticket) == 0                    # advanced once, the ticket left at zero
    use = GC.use_of_bounds(res, *state, rs, step, GC.ROWS, GC.GRAD_SCALE, coef)
    _fig('adam_step_groups', step=step, form=form, clip=clip, p=use[0], m=use[1], v=use[2])
    assert max(use) <= 1.0, use
    mask = GC.inside(rs, len(state[0]))
    for x, y, orig, what in zip(res, ref, (state[0], state[2], state[3]), 'pmv'):
        assert _same(x, y), (what, 'bits differ from lirec_adam_step_ranges per group', int((_bits(x) != _bits(y)).sum()))
        assert _same(x[~mask], orig[~mask]), (what, 'a guard word was written')
        assert not _same(x[mask], orig[mask])
    assert _same(_np(got.g), state[1]), 'the gradients were written'
    # the three groups really were updated with three different rows: with one row for all, two of them come out differently
    one_row = GC.ref32(*state, rs, step, [GC.ROWS[0]] * 3, GC.GRAD_SCALE, coef)
    for grp in (1, 2):
        o, k = next((o, k) for o, k, _, g_ in rs if g_ == grp and k > 100)
        assert not _same(res[0][o:o + k], one_row[0][o:o + k])


def test_counted_form_without_advance_and_an_empty_call():
    step = 3
    state, rs = GC.build(step)
    b = Bufs(state)
    table = _table(GC.ROWS)
    count = torch.tensor([step - 1], dtype=torch.int64, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    # all lengths 0, count 0: no launch, no advance
    ops.adam_step_groups(b.p, b.g, b.m, b.v, [(o, 0, lag, grp) for o, _, lag, grp in rs], table, 3, 0, 1.0, count_dev=count, ticket=ticket)
    ops.adam_step_groups(b.p, b.g, b.m, b.v, [], table, 3, 0, 1.0, count_dev=count, ticket=ticket)
    assert all(_same(x, y) for x, y in zip(b.result(), (state[0], state[2], state[3]))) and int(count) == step - 1
    # an update cut into two calls: the first does not advance, both use the same step
    ops.adam_step_groups(b.p, b.g, b.m, b.v, rs[:5], table, 3, 0, GC.GRAD_SCALE, count_dev=count, ticket=ticket, advance=False)
    torch.cuda.synchronize()
    assert int(count) == step - 1 and int(ticket) == 0
    ops.adam_step_groups(b.p, b.g, b.m, b.v, rs[5:], table, 3, 0, GC.GRAD_SCALE, count_dev=count, ticket=ticket, advance=True)
    want = Bufs(state)
    _per_group_by_value(want, rs, GC.ROWS, step, GC.GRAD_SCALE)
    assert all(_same(x, y) for x, y in zip(b.result(), want.result()))
    assert int(count) == step and int(ticket) == 0


def test_the_table_is_read_by_every_launch():
    """launch, write other rows on the same stream, launch again: the second launch used the new rows -- bit for bit the by-value
    call with them --, the first the old ones; nothing synchronises in between"""
    step = 3
    state, rs = GC.build(step)
    got = Bufs(state)
    table = _table(GC.ROWS)
    sd = torch.tensor([step], dtype=torch.int64, device=DEV)
    ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, table, 3, 0, GC.GRAD_SCALE, step_dev=sd)
    ops.adam_hyper_write(table, GC.ROWS_B)
    ops.counter_add(sd, [1])
    ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, table, 3, 0, GC.GRAD_SCALE, step_dev=sd)
    want = Bufs(state)
    _per_group_by_value(want, rs, GC.ROWS, step, GC.GRAD_SCALE)
    first = want.result()
    _per_group_by_value(want, rs, GC.ROWS_B, step + 1, GC.GRAD_SCALE)
    res, ref = got.result(), want.result()
    for x, y, what in zip(res, ref, 'pmv'):
        assert _same(x, y), (what, int((_bits(x) != _bits(y)).sum()))
    stale = Bufs((first[0], state[1], first[1], first[2]))
    _per_group_by_value(stale, rs, GC.ROWS, step + 1, GC.GRAD_SCALE)
    assert not _same(stale.result()[0], res[0]), 'the second launch cannot be told from one with the old rows'
    t = _np(table).reshape(8, 8)
    assert np.array_equal(t[:3, :5], np.asarray(GC.ROWS_B, np.float32)) and (t[:3, 5:] == 0).all() and np.isnan(t[3:]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. FusedAdam, the small model
# ---------------------------------------------------------------------------------------------------------------------------
def _small(side, groups='three', dropout=0.3, **kw):
    from lirec_amd import model as M
    from lirec_amd.data import synthetic_batch, to_device_batch
    config.recipe('int_rel_ch', joint_dim=GC.JOINT, rels_n_clips=GC.R, dropout=dropout, dropout_seed=77, **GC.DIMS)
    opt.device = 'cuda'
    opt.adam_on_side_stream = side
    torch.manual_seed(3)
    model, loss, _ = M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)
    model.train()
    pg = GC.three_groups(model) if groups == 'three' else groups
    optim = FusedAdam(model, lr=3e-5, weight_decay=1e-5, param_groups=pg, **kw)
    batch = to_device_batch(synthetic_batch(5, 'int_rel_ch', GC.B, n_classes=GC.N_CLASSES, n_rels=GC.N_RELS, T=GC.T, R=GC.R, **GC.DIMS), 'cuda')
    return model, loss, optim, batch


def _backward(model, loss, optim, batch):
    optim.zero_grad()
    lv = loss(model(dict(batch)), batch)
    lv.backward()
    optim._ensure_state()
    torch.cuda.synchronize()


def _snap(model, optim):
    """parameters and both moments as they are now (device copies: the default-dimension model has 18 M elements)"""
    return [t.detach().clone() for t in (model.flat_params(), optim._m, optim._v)]


def _check_step(model, optim, before, grad, after, step, what, coef=1.0, rs=None, rows=None):
    """every element of the flat buffers: the trainable parameters within adam_cases.bounds of ref64 per group, fed the device's own
    gradient; everything else -- alignment gaps, frozen parameters -- bit for bit as it was"""
    rows = GC.rows_of(optim) if rows is None else rows
    if rs is None and len(rows) == 1 and optim.all_trainable() and coef == 1.0:
        # (one group, everything trainable: adam_cases' yardstick on the device, as tests/test_gpu_optim.py uses it -- every element
        #  of the buffers, alignment gaps included)
        use = AC.use_of_bounds(after, before[0], grad, before[1], before[2], step, GC.hyper_of(rows[0], optim.grad_scale))
        _fig('fused_adam', route=what, step=step, p=use[0], m=use[1], v=use[2])
        assert max(use) <= 1.0, (what, step, use)
        assert float(((after[0] != before[0]) & (grad != 0)).float().sum() / (grad != 0).float().sum()) > 0.5
        return use
    before, after, grad = [_np(t) if torch.is_tensor(t) else t for t in before], [_np(t) if torch.is_tensor(t) else t for t in after], \
        (_np(grad) if torch.is_tensor(grad) else grad)
    rs = GC.model_ranges(model, optim) if rs is None else rs
    use = GC.use_of_bounds(after, before[0], grad, before[1], before[2], rs, step, rows, optim.grad_scale, coef)
    _fig('fused_adam', route=what, step=step, p=use[0], m=use[1], v=use[2])
    assert max(use) <= 1.0, (what, step, use)
    mask = GC.inside(rs, len(grad))
    for a, b, w in zip(after, before, 'pmv'):
        assert _same(a[~mask], b[~mask]), (what, step, w, 'written outside the trainable parameters')
    moved = np.abs(after[0][mask].astype(np.float64) - before[0][mask]) > 0
    assert moved.mean() > 0.5, 'most parameters with a gradient move in a step'
    return use


_runs = {}


def _cached(key, fn):
    if key in _runs:
        if isinstance(_runs[key], BaseException):
            raise _runs[key]                      # (a run that failed is not run a second time)
        return _runs[key]
    try:
        _runs[key] = fn()
    except BaseException as e:
        _runs[key] = e
        raise
    return _runs[key]


STEPS = 5


def _route(route, make, steps=STEPS, check=True, between=None):
    """{step: [flat, m, v]} of `steps` steps on a route ('plain' | 'side' | 'recorded': one warm-up step, the recording step,
    replays).  `make(side)` -> (model, loss, optim, batch); `between(step, optim)`: called after every step that can be followed by
    a change of the hyper-parameters (recorded: from the recording step on)."""
    from lirec_amd.graph import RecordedTrainStep
    out = {}
    try:
        model, loss, optim, batch = make(route != 'plain')
        if route != 'recorded':
            for s in range(1, steps + 1):
                _backward(model, loss, optim, batch)
                before, grad = out.get(s - 1) or _snap(model, optim), model.flat_grads(attach=False).clone()
                rows = GC.rows_of(optim)
                optim.step()
                torch.cuda.synchronize()
                assert bool(model.lanes.bucket0_on_side) == (route == 'side'), 'the step took another route'
                out[s] = _snap(model, optim)
                if check:
                    _check_step(model, optim, before, grad, out[s], s, route, rows=rows)
                if between is not None and s >= 2:
                    between(s, optim)
        else:
            g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
            try:
                torch.cuda.synchronize()
                out['flags'] = (g.overwrite, g.fused, g.defer)
                lanes = {}
                out['commands'] = [(lanes.setdefault(s, len(lanes)), k) for s, k in (g.cmds.command(i) for i in range(g.cmds.size))]
                out[2] = _snap(model, optim)
                size, handle = g.cmds.size, g.cmds.handle
                if between is not None:
                    between(2, optim)
                for s in range(3, steps + 1):
                    before, rows = out[s - 1], GC.rows_of(optim)
                    g.step()
                    g.flush()
                    torch.cuda.synchronize()
                    out[s] = _snap(model, optim)
                    if check and g.overwrite:               # (the replay stored this step's gradients: nothing was accumulated)
                        _check_step(model, optim, before, model.flat_grads(attach=False).clone(), out[s], s, route, rows=rows)
                    if between is not None:
                        between(s, optim)
                    assert g.cmds.size == size and g.cmds.handle is handle
                out['state'] = g.state.tolist()
                out['model'] = model
                if out['flags'][1]:
                    out['shadow_ok'] = _shadow_is_current(model)
            finally:
                g.release()
    finally:
        config.reset()
    return out


def _shadow_is_current(model):
    """the q32b copy of every first-layer weight == lirec_to_q32b of the weight as it is now (tests/test_gpu_optim.py)"""
    pd = dict(model.named_parameters())
    assert model._w1q_valid and len(model._w1q) == 8
    base = model._w1q_buf.data_ptr()
    for n, addr in model._w1q.items():
        ref = ops.to_q32b(pd[n].data.contiguous()).data
        k = 4 * pd[n].numel()
        assert torch.equal(model._w1q_buf[addr - base:addr - base + k], ref[:k]), 'q32b shadow of %s is stale' % n
    return True


def _agree(a, b, what, steps):
    for s in steps:
        for x, y, w in zip(a[s], b[s], ('parameters', 'exp_avg', 'exp_avg_sq')):
            assert _same(x, y), (what, s, w, int((_bits(x) != _bits(y)).sum()))


@pytest.mark.parametrize('route', ['plain', 'side', 'recorded'])
def test_three_groups_within_the_bounds_on_every_route(route):
    out = _cached(('three', route), lambda: _route(route, lambda side: _small(side)))
    assert sorted(k for k in out if isinstance(k, int)) == (list(range(1, STEPS + 1)) if route != 'recorded' else list(range(2, STEPS + 1)))


def test_three_groups_the_routes_agree_bit_for_bit():
    plain, side, rec = (_cached(('three', r), lambda r=r: _route(r, lambda side: _small(side))) for r in ('plain', 'side', 'recorded'))
    _agree(plain, side, 'plain vs side stream', range(1, STEPS + 1))
    _agree(side, rec, 'eager vs recorded', range(2, STEPS + 1))
    assert rec['state'][1:] == [STEPS, STEPS]


def test_three_groups_differ_from_one_group():
    """the groups' values reach the update: against one group with the constructor's values, the biases (lr 1e-3 instead of 3e-5)
    and the embeddings' weights (lr 1e-5, other betas) end elsewhere"""
    three = _cached(('three', 'plain'), lambda: _route('plain', lambda side: _small(side)))
    one = _cached(('one', 'plain'), lambda: _route('plain', lambda side: _small(side, groups=None), check=False))
    assert not _same(three[STEPS][0], one[STEPS][0])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. 70 ranges: two calls per update
# ---------------------------------------------------------------------------------------------------------------------------
class ManyParams:
    """a stand-in for the model: 140 parameters of 5 .. 9 elements in one flat buffer, each on a multiple of 4 (what FusedAdam
    reads of a model on its single-GPU routes, and nothing else).  `lanes`: a real StepLanes around a lane of the stand-in's own;
    `side_after_backward()` leaves what a backward that left its first bucket to the side stream would hand step(), here the
    whole buffer."""
    grad_sync = None
    _lane = None

    def side_after_backward(self):
        self.lanes.bucket0_end = self._n_flat
        self.lanes.after_backward = (self.lanes.sides[0].handle, ops.current_stream_handle())

    def __init__(self, n=140):
        r = np.random.default_rng(2)
        self._offsets, at = {}, 0
        for i in range(n):
            k = 5 + i % 5
            self._offsets['q%03d' % i] = (at, k)
            at = (at + k + 3) // 4 * 4
        self._n_flat = at + 4
        vals = np.zeros(self._n_flat, np.float32)
        for o, k in self._offsets.values():
            vals[o:o + k] = (0.1 * r.standard_normal(k)).astype(np.float32)
        self._flat = torch.from_numpy(vals).to(DEV)
        self._flat_grad = torch.zeros_like(self._flat)
        self._plist = [torch.nn.Parameter(self._flat[o:o + k]) for o, k in self._offsets.values()]
        if ManyParams._lane is None:
            stream = torch.cuda.Stream()
            ManyParams._lane = Lane(stream, None, ctypes.c_void_p(stream.cuda_stream))
        self.lanes = StepLanes({0: ManyParams._lane})

    def parameters(self):
        return iter(self._plist)

    def named_parameters(self):
        return iter(zip(self._offsets, self._plist))

    def flat_params(self):
        return self._flat

    def flat_grads(self, attach=True):
        return self._flat_grad


@pytest.mark.parametrize('form', ['by_value', 'step_dev', 'counted'])
def test_more_than_64_ranges_take_two_calls(form):
    opt.adam_on_side_stream = True
    model = ManyParams()
    names = list(model._offsets)
    groups = [dict(params=[n for i, n in enumerate(names) if i % 3 == j], lr=lr, weight_decay=wd)
              for j, (lr, wd) in enumerate(((1e-3, 0.0), (3e-4, 1e-5), (1e-2, 1e-2)))]
    optim = FusedAdam(model, lr=3e-5, param_groups=groups)
    for i, p in enumerate(model._plist):
        p.requires_grad_(i % 2 == 0)
    rs = optim.trainable_ranges()
    assert len(rs) == 70 and len(FusedAdam._chunks(rs)) == 2
    calls, f0 = [], ops.adam_step_groups
    ops.adam_step_groups = lambda *a, **k: (calls.append(len(a[4])), f0(*a, **k))[1]
    try:
        r = np.random.default_rng(4)
        if form != 'by_value':
            optim._step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        if form == 'counted':
            # (the side route of step(): the update on the side stream, the step from that stream's own counter of completed steps,
            #  advanced by the LAST of the two calls only)
            model.lanes.step_side_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        for step in (1, 2):
            model._flat_grad.copy_(torch.from_numpy(r.standard_normal(model._n_flat).astype(np.float32)))
            optim._ensure_state()
            before, grad = _snap(model, optim), model._flat_grad.clone()
            if form != 'by_value':
                optim._step_dev.fill_(step)
            torch.cuda.synchronize()
            if form == 'counted':
                model.side_after_backward()
            optim.step()
            torch.cuda.synchronize()
            if form != 'by_value':
                optim._step += 1
                optim._advance_lags()
            if form == 'counted':
                assert int(model.lanes.step_side_dev) == step and int(model.lanes.side_ticket) == 0 and model.lanes.bucket0_on_side
                assert sorted(optim._tables) == ['main', 'side']
            after = _snap(model, optim)
            full = [(o, k, lag, grp) for o, k, lag, grp in GC.model_ranges(model, optim)]
            # (the lags of model_ranges are those AFTER the step's bookkeeping: the frozen ones', which are not in it)
            _check_step(model, optim, before, grad, after, step, 'many-' + form, rs=full)
    finally:
        ops.adam_step_groups = f0
        config.reset()
    assert calls == [64, 6, 64, 6], calls


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the headline form: the default dimensions, where the recorded step folds the first-layer update in
# ---------------------------------------------------------------------------------------------------------------------------
BB, BT, BR = 4, 8, 18
LR = 1e-3


def _big(side, **kw):
    """the model of tests/test_gpu_optim.py's route tests"""
    from lirec_amd import model as M
    from lirec_amd.data import synthetic_batch, to_device_batch
    from oracle import lirec_oracle as O
    config.recipe('int_rel_ch', rels_n_clips=BR, dropout_seed=77, lr=LR)
    opt.device = 'cuda'
    opt.adam_on_side_stream = side
    model, loss, optim = M.create_model(101, n_rels=15)
    if kw:
        optim = FusedAdam(model, lr=opt.lr, weight_decay=opt.weight_decay, **kw)
    model.load_state_dict(O.fill_params(O.param_shapes(O.OracleCfg(), 101, 15), 5), strict=True)
    model.train()
    batch = to_device_batch(synthetic_batch(11, 'int_rel_ch', BB, T=BT, R=BR), 'cuda')
    return model, loss, optim, batch


def _big_run(variant, route):
    def make(side):
        if variant == 'no_keywords':
            return _big(side)
        if variant == 'param_groups_none':
            return _big(side, param_groups=None)
        if variant == 'device_hyper':
            return _big(side, device_hyper=True)
        model, loss, optim, batch = _big(side)
        return model, loss, FusedAdam(model, lr=opt.lr, weight_decay=opt.weight_decay,
                                      param_groups=[dict(params=[n for n, _ in model.named_parameters()])]), batch
    return _cached(('big', variant, route), lambda: _route(route, make, check=False))


@pytest.mark.parametrize('route', ['plain', 'side', 'recorded'])
def test_one_group_with_device_hyper_is_the_by_value_path_bit_for_bit(route):
    base, got = _big_run('no_keywords', route), _big_run('device_hyper', route)
    _agree(base, got, 'device_hyper vs by value, ' + route, [s for s in range(1, STEPS + 1) if s in base])
    if route == 'recorded':
        # the headline form both ways: overwrite mode, the first-layer update folded in (by value: the kernel as it was; device_hyper:
        # the row kernel), the side stream left un-joined
        assert base['flags'] == (True, True, True) and got['flags'] == (True, True, True), (base['flags'], got['flags'])
        assert got['shadow_ok'] and base['shadow_ok']
        assert got['commands'] == base['commands']


@pytest.mark.parametrize('variant', ['param_groups_none', 'one_explicit_group'])
@pytest.mark.parametrize('route', ['plain', 'side', 'recorded'])
def test_off_is_off(route, variant):
    """the constructor without the new keywords, with param_groups=None and with one explicit group naming every parameter: the same
    bits after every step, and the same recorded command list -- commands, streams, order"""
    base, got = _big_run('no_keywords', route), _big_run(variant, route)
    _agree(base, got, variant + ', ' + route, [s for s in range(1, STEPS + 1) if s in base])
    if route == 'recorded':
        assert got['flags'] == base['flags'] == (True, True, True)
        assert got['commands'] == base['commands'] and len(base['commands']) > 5


def _schedule(s):
    """three warm-up steps, then decay"""
    return (s + 1) / 4.0 if s < 3 else 0.9 ** (s - 3)


def _scheduled(route, hold_side=False, every_replay=False):
    """2 + 8 steps under torch.optim.lr_scheduler.LambdaLR, the weight decay changed half-way; `route` 'side' (the eager
    device_hyper loop) or 'recorded' (ONE recording, then 8 replays).  `hold_side`: the side stream's share of every step starts
    ~2 ms late (lirec_debug_set bit 131072 in that stream's library context, as tests/test_gpu_recorded_bench_shape.py uses it)."""
    sched = []

    def between(s, optim):
        if not sched:
            sched.append(torch.optim.lr_scheduler.LambdaLR(optim, (lambda k: 1.0 / (1.0 + 0.37 * k)) if every_replay else _schedule))
        else:
            sched[0].step()
        if s == 6:
            optim.param_groups[0]['weight_decay'] = 1e-3
        lrs.append(optim.param_groups[0]['lr'])
    lrs = []

    def make(side):
        m = _big(side, device_hyper=True)
        if hold_side:
            lane = m[0]._wgrad_lane()
            assert lane is not None
            with lane[1]:
                _lib.lib().lirec_debug_set(131072, -1)
            held.append(lane)
        return m
    held = []
    import warnings
    try:
        with warnings.catch_warnings():
            warnings.filterwarnings('error', message='Detected call of')      # (a replayed step is an optimiser step: no order warning)
            out = _route(route, make, steps=10, check=not hold_side, between=between)
    finally:
        for lane in held:
            with lane[1]:
                _lib.lib().lirec_debug_set(0, -1)
    out['lrs'] = lrs
    return out


def test_a_schedule_through_one_recording_in_the_headline_form():
    """record once; 8 replays under LambdaLR (3 warm-up steps, then decay) and one weight-decay change: no raise, the command list
    unchanged (asserted after every replay in _route), parameters and moments bit for bit those of the eager device_hyper loop under
    the same schedule, every step within the bounds of ref64 (checked in _route on both), the W1 shadow current"""
    eager = _cached(('sched', 'side'), lambda: _scheduled('side'))
    rec = _cached(('sched', 'recorded'), lambda: _scheduled('recorded'))
    assert rec['flags'] == (True, True, True), rec['flags']              # overwrite mode, fused, deferred side join
    assert rec['lrs'] == eager['lrs'] and len(set(rec['lrs'])) >= 8, rec['lrs']
    _fig('schedule', lrs=['%.3g' % x for x in rec['lrs']])
    _agree(eager, rec, 'eager device_hyper vs replays under a schedule', range(2, 11))
    assert rec['shadow_ok'] and rec['state'][1:] == [10, 10]
    # the schedule reached the update: the by-value run without one ends elsewhere
    assert not _same(_big_run('no_keywords', 'side')[STEPS][0], eager[STEPS][0])
    # (memory: the snapshots of these runs are device copies, 0.2 GB a step)


def test_a_schedule_with_the_side_stream_held_back():
    """the learning rate changes in front of EVERY replay while the side stream's share of each step -- the heads' and the gate's
    update among it -- starts after the main stream has begun the next step: that update must still read ITS step's learning rate
    (the side stream's own table, written on the side stream).  The eager loop's bits."""
    eager = _cached(('sched-every', 'side'), lambda: _scheduled('side', every_replay=True))
    rec = _scheduled('recorded', hold_side=True, every_replay=True)
    assert rec['flags'] == (True, True, True), rec['flags']
    assert rec['lrs'] == eager['lrs'] and len(set(rec['lrs'])) == 9
    _agree(eager, rec, 'eager vs replays with the side stream held back', range(2, 11))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. with a frozen parameter, against torch in float64; with clipping
# ---------------------------------------------------------------------------------------------------------------------------
def _torch64_step(model, optim, before, grad, step_of):
    """one step of a stock torch.optim.Adam on float64 copies of the device's state before the step, with the optimiser's groups,
    fed the device's gradient: (p', m', v') as flat float64 arrays (elements outside the trainable parameters as they were)"""
    qs, groups = {}, []
    names = [n for n, _ in model.named_parameters()]
    by_obj = {id(p): n for n, p in model.named_parameters()}
    for g in optim.param_groups:
        mine = []
        for p in g['params']:
            n = by_obj[id(p)]
            o, k = model._offsets[n]
            q = torch.nn.Parameter(torch.from_numpy(before[0][o:o + k].astype(np.float64)))
            q.grad = torch.from_numpy(grad[o:o + k].astype(np.float64) * optim.grad_scale) if p.requires_grad else None
            qs[n] = q
            mine.append(q)
        groups.append(dict(params=mine, lr=float(np.float32(g['lr'])), betas=tuple(float(np.float32(b)) for b in g['betas']),
                           eps=float(np.float32(g['eps'])), weight_decay=float(np.float32(g['weight_decay']))))
    ref = torch.optim.Adam(groups)
    for n in names:
        o, k = model._offsets[n]
        ref.state[qs[n]] = {'step': torch.tensor(float(step_of[n])), 'exp_avg': torch.from_numpy(before[1][o:o + k].astype(np.float64)),
                            'exp_avg_sq': torch.from_numpy(before[2][o:o + k].astype(np.float64))}
    ref.step()
    out = [a.astype(np.float64) for a in before]
    for n in names:
        o, k = model._offsets[n]
        st = ref.state[qs[n]]
        out[0][o:o + k], out[1][o:o + k], out[2][o:o + k] = qs[n].detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()
    return out


@pytest.mark.parametrize('route', ['plain', 'side'])
def test_groups_with_a_parameter_frozen_for_two_steps_against_torch_float64(route):
    """one weight in the middle of the embeddings' group is frozen for steps 2 and 3 and trains again in 4 and 5 -- two updates
    behind, as torch.optim.Adam counts it: every step against a stock float64 Adam with the same groups started from the device's
    state, within adam_cases.bounds; the frozen weight and its moments keep their bits"""
    try:
        model, loss, optim, batch = _small(route == 'side')
        frozen = 'vis2_ctx.weight'
        assert frozen in GC.three_groups(model)[2]['params'][1:-1]
        fp = dict(model.named_parameters())[frozen]
        fo, fk = model._offsets[frozen]
        step_of = {n: 0 for n, _ in model.named_parameters()}
        for s in range(1, 6):
            fp.requires_grad_(s not in (2, 3))
            _backward(model, loss, optim, batch)
            before, grad = [_np(t) for t in _snap(model, optim)], _np(model.flat_grads(attach=False))
            rs = GC.model_ranges(model, optim)
            optim.step()
            torch.cuda.synchronize()
            after = [_np(t) for t in _snap(model, optim)]
            want = _torch64_step(model, optim, before, grad, step_of)
            for n, p in model.named_parameters():
                step_of[n] += int(p.requires_grad)
            bounds = GC.ref64(before[0], grad, before[1], before[2], rs, s, GC.rows_of(optim), optim.grad_scale)[3:]
            mask = GC.inside(rs, len(grad))
            use = [float((np.abs(a.astype(np.float64) - w)[mask] / b[mask]).max()) for a, w, b in zip(after, want, bounds)]
            _fig('frozen_in_a_group', route=route, step=s, p=use[0], m=use[1], v=use[2])
            assert max(use) <= 1.0, (s, use)
            for a, b in zip(after, before):
                assert _same(a[~mask], b[~mask])
            if s in (2, 3):
                assert not mask[fo:fo + fk].any() and len(rs) == 37
        assert optim._lag == {frozen: 2} and step_of[frozen] == 3
        sd = optim.state_dict()
        assert sorted({int(float(st['step'])) for st in sd['state'].values()}) == [3, 5]
    finally:
        config.reset()


def test_groups_with_max_grad_norm_1():
    """one global norm over all trainable parameters of all groups, one coefficient: grad_norm and clip_coef against
    torch.nn.utils.clip_grad_norm_ over float64 copies of all gradients (equal or adjacent fp32 values, as tests/test_gpu_clip.py
    holds them), the update within the bounds with that coefficient"""
    try:
        model, loss, optim, batch = _small(True, dropout=0.0)
        optim.max_grad_norm = 1.0
        clipped = []
        for s in range(1, 4):
            _backward(model, loss, optim, batch)
            before, grad = [_np(t) for t in _snap(model, optim)], _np(model.flat_grads(attach=False))
            optim.step()
            torch.cuda.synchronize()
            after = [_np(t) for t in _snap(model, optim)]
            copies = []
            for n, p in model.named_parameters():
                o, k = model._offsets[n]
                q = torch.nn.Parameter(torch.zeros(k, dtype=torch.float64))
                q.grad = torch.from_numpy(grad[o:o + k].astype(np.float64) * optim.grad_scale)
                copies.append(q)
            norm = float(torch.nn.utils.clip_grad_norm_(copies, 1.0))
            coef = min(1.0, 1.0 / (norm + 1e-6))
            got_coef, got_norm = float(optim.clip_coef), float(optim.grad_norm)
            _fig('clip_with_groups', step=s, norm=got_norm, coef=got_coef, torch_norm=norm, torch_coef=coef)
            adjacent = lambda a, b: abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32))) <= 1
            assert adjacent(got_norm, norm) and adjacent(got_coef, coef), (got_norm, norm, got_coef, coef)
            _check_step(model, optim, before, grad, after, s, 'clipped', coef=got_coef)
            assert _same(_np(model.flat_grads(attach=False)), grad)
            clipped.append(got_coef < 1.0)
            assert not model.lanes.bucket0_on_side        # (a clipped update runs whole on the caller's stream)
        assert any(clipped), 'max_grad_norm = 1 never clipped: the test shows nothing'
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. training(..., scheduler=)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('every', ['step', 'epoch'])
def test_training_steps_the_scheduler(every, tmp_path):
    """lirec_amd.train.training with three groups and a torch scheduler: stepped once per optimiser step (or per epoch), after it --
    torch's order warning would be an error here --, and the checkpoint names the groups' members"""
    import os
    import warnings
    from lirec_amd import model as M
    from lirec_amd.data import SyntheticMixedFeaturesDataset
    from lirec_amd.train import training
    try:
        config.recipe('int_rel_ch', joint_dim=GC.JOINT, batch_size=4, num_workers=0, epochs=2, test_fr=1, store_root=str(tmp_path),
                      rels_n_clips=GC.R, **GC.DIMS)
        opt.device = 'cuda'
        kw = dict(T=GC.T, R=GC.R, n_classes=GC.N_CLASSES, n_rels=GC.N_RELS, n_mgd=11, soft_gt=opt.soft_gt, **GC.DIMS)
        mk = lambda n, seed: SyntheticMixedFeaturesDataset('int_rel_ch', n, seed=seed, **kw)
        model, loss, _ = M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)
        optim = FusedAdam(model, lr=3e-5, param_groups=GC.three_groups(model))
        sched = torch.optim.lr_scheduler.LambdaLR(optim, lambda s: 0.5 ** s)
        with warnings.catch_warnings():
            warnings.filterwarnings('error', message='Detected call of')
            training(mk(9, 1), model=model, loss=loss, optimizer=optim, test_dataset=mk(8, 2), scheduler=sched, scheduler_every=every)
        assert optim._step == 4                                     # (two batches of four an epoch; the single clip left over is skipped)
        n = sched.last_epoch
        assert n == (4 if every == 'step' else 2)
        assert [g['lr'] for g in optim.param_groups] == [h['lr'] * 0.5 ** n for h in GC.GROUP_HYPERS]
        ck = torch.load(os.path.join(str(tmp_path), '1.pth.tar'), weights_only=False)
        assert ck['param_group_names'] == optim.group_names() and len(ck['optimizer']['param_groups']) == 3
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the folded update with a BY-VALUE step reading its row
# ---------------------------------------------------------------------------------------------------------------------------
def test_folded_update_with_a_by_value_step_reads_the_row():
    """The recorded step arms the folded first-layer update with step_dev; here it is armed by hand in the eager loop, where the
    step comes by value and the row kernel computes the bias corrections from it: three steps, the learning rate changed before
    the third, bit for bit the loop that leaves the first layers to step() (lirec_adam_step_groups)."""
    def run(arm):
        try:
            model, loss, optim, batch = _big(False, device_hyper=True)
            applied = []
            for s in range(3):
                if s == 2:
                    optim.param_groups[0]['lr'] = 3e-4
                optim.zero_grad()
                lv = loss(model(dict(batch)), batch)
                if arm:
                    assert optim.arm_first_layer_update() and optim._step_dev is None
                lv.backward()
                applied.append(bool(model.lanes.fold_applied))
                optim.step()
                torch.cuda.synchronize()
            return _snap(model, optim), applied
        finally:
            config.reset()
    (plain, a0), (folded, a1) = run(False), run(True)
    assert a0 == [False] * 3 and a1 == [True] * 3, (a0, a1)
    for x, y, what in zip(plain, folded, ('parameters', 'exp_avg', 'exp_avg_sq')):
        assert _same(x, y), (what, int((x != y).sum()))
