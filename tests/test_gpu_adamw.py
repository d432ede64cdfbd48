"""Decoupled weight decay (AdamW) per parameter group on the GPU (include/lirec_hip.h, "DECOUPLED WEIGHT DECAY";
lirec_amd/optim.py): lirec_adam_step_groups with decoupled and coupled rows in one launch -- the decoupled ranges bit for bit the
fp32 restatement adamw_cases.ref32w and inside adam_cases.bounds against ref64w, the coupled ones bit for bit
lirec_adam_step_ranges by value --; one decoupled range of 4 M elements; the flag word lirec_adam_hyper_write stores; the folded
first-layer update reading a decoupled row, and one row PER PARAMETER (lirec_set_adam_hyper_map), against the unfused gradient
followed by one grouped launch; FusedAdam with weights that decay and biases that do not on its plain, side-stream and recorded
routes, clipped, with a parameter frozen for a step, and with lr and the flag changed in front of every replay while the side
stream is held back; the recorded step at the dimensions where the persistent kernels run, the fold armed across two groups.

Bounds: adam_cases.bounds with G = |g gs| (tests/adamw_cases.py); tests/test_host_adamw.py shows the yardstick equal to
torch.optim.AdamW in float64 and ref32w under half of every bound on the cases here.  The helpers of tests/test_gpu_groups.py
(routes, snapshots, the big model) and tests/test_gpu_layer1_persistent.py (heads of the layer-1 kernels) are used as they are."""
import numpy as np
import pytest
import torch

import adam_cases as AC
import adamw_cases as WC
import group_cases as GC
import test_gpu_groups as TG
import test_gpu_layer1_persistent as TP
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt
from lirec_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_np, _bits, _same, Bufs = TG._np, TG._bits, TG._same, TG.Bufs


def _fig(what, **kw):
    print('ADAMW-FIGURE %s %s' % (what, ' '.join('%s=%s' % (k, ('%.4g' % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _table(rows6):
    t = torch.full((8 * _lib.ADAM_MAX_GROUPS,), float('nan'), dtype=torch.float32, device=DEV)
    ops.adam_hyper_write(t, rows6)
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lirec_adam_step_groups, mixed rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [False, True], ids=['unclipped', 'clipped'])
@pytest.mark.parametrize('form', ['by_value', 'step_dev', 'counted'])
@pytest.mark.parametrize('table', sorted(WC.TABLES))
@pytest.mark.parametrize('step', GC.STEPS)
def test_adam_step_groups_with_mixed_rows(step, table, form, clip):
    rows, flags = WC.TABLES[table]
    state, rs = GC.build(step)
    if form == 'by_value' and step == 1:
        rs = [(o, k, 0, grp) for o, k, _, grp in rs]        # (a by-value step minus the lag must be >= 1: run with every lag 0)
    coef = GC.COEF if clip else 1.0
    cbuf = torch.tensor([coef], dtype=torch.float32, device=DEV) if clip else None
    got, want = Bufs(state), Bufs(state)
    tab = _table(WC.rows6(rows, flags))
    count = ticket = None
    with ops.adam_clip(cbuf):
        if form == 'by_value':
            ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, tab, 3, step, GC.GRAD_SCALE)
        elif form == 'step_dev':
            sd = torch.tensor([step], dtype=torch.int64, device=DEV)
            ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, tab, 3, 0, GC.GRAD_SCALE, step_dev=sd)
        else:
            count = torch.tensor([step - 1], dtype=torch.int64, device=DEV)
            ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.adam_step_groups(got.p, got.g, got.m, got.v, rs, tab, 3, 0, GC.GRAD_SCALE, count_dev=count, ticket=ticket, advance=True)
        # the coupled group: the existing kernel with that group's values by value
        TG._per_group_by_value(want, [r for r in rs if not flags[r[3]]], rows, step, GC.GRAD_SCALE)
    res, ref = got.result(), want.result()
    if form == 'counted':
        assert int(count) == step and int(ticket) == 0                    # advanced once, the ticket left at zero
    r32 = WC.ref32(*state, rs, step, rows, flags, GC.GRAD_SCALE, coef)
    dec = [r for r in rs if flags[r[3]]]
    use = WC.use_of_bounds(res, *state, dec, step, rows, flags, GC.GRAD_SCALE, coef)
    _fig('adam_step_groups', step=step, table=table, form=form, clip=clip, p=use[0], m=use[1], v=use[2])
    assert max(use) <= 1.0, use
    mask = GC.inside(rs, len(state[0]))
    for x, y, z, orig, what in zip(res, ref, r32, (state[0], state[2], state[3]), 'pmv'):
        for o, k, _, grp in rs:
            if flags[grp]:
                assert _same(x[o:o + k], z[o:o + k]), (what, 'a decoupled range differs from ref32w', o, k, int((_bits(x[o:o + k]) != _bits(z[o:o + k])).sum()))
            else:
                assert _same(x[o:o + k], y[o:o + k]), (what, 'a coupled range differs from lirec_adam_step_ranges by value', o, k)
                assert _same(x[o:o + k], z[o:o + k])
        assert _same(x[~mask], orig[~mask]), (what, 'a guard word was written')
        assert not _same(x[mask], orig[mask])
    assert _same(_np(got.g), state[1]), 'the gradients were written'
    # the flag reached the update: with every group coupled the visible decoupled ranges come out differently -- and the
    # invisible row (table B, group 2) has the bits of wd = 0
    coupled = WC.ref32(*state, rs, step, rows, [False] * 3, GC.GRAD_SCALE, coef)
    o, k = next((o, k) for o, k, _, g_ in rs if g_ == 0 and k > 100)
    assert not _same(res[0][o:o + k], coupled[0][o:o + k])
    if table == 'B':
        nodecay = WC.ref32(*state, rs, step, [rows[0], rows[1], rows[2][:4] + (0.0,)], flags, GC.GRAD_SCALE, coef)
        for o, k, _, g_ in rs:
            if g_ == 2:
                assert all(_same(a[o:o + k], b[o:o + k]) for a, b in zip(res, nodecay))


def test_one_decoupled_range_of_four_million_elements():
    """adam_cases.N_BIG: every workgroup takes several blocks, and a scalar tail of three; bit for bit ref32w, inside the bounds"""
    step, row = 3, WC.ROWS_W[0]
    state = AC.make_state(AC.Case(1, step, 1.0), AC.N_BIG)
    b = Bufs(state)
    ops.adam_step_groups(b.p, b.g, b.m, b.v, [(0, AC.N_BIG, 0, 0)], _table(WC.rows6([row], [True])), 1, step, GC.GRAD_SCALE)
    res = b.result()
    h = AC.hyper32(tuple(row) + (GC.GRAD_SCALE,))
    for x, y, what in zip(res, WC.ref32w(*state, step, h), 'pmv'):
        assert _same(x, y), (what, int((_bits(x) != _bits(y)).sum()))
    pn, mn, vn, G, A, V = WC.ref64w(*state, step, h)
    use = [float((np.abs(x.astype(np.float64) - r) / bd).max()) for x, r, bd in zip(res, (pn, mn, vn), AC.bounds(state[0], state[2], G, A, V))]
    _fig('n_big', p=use[0], m=use[1], v=use[2])
    assert max(use) <= 1.0, use


def test_hyper_write_stores_the_flag_word():
    t = _np(_table([GC.ROWS_B[0] + (True,), GC.ROWS_B[1], GC.ROWS_B[2] + (0,), GC.ROWS_B[0] + (3,)])).reshape(8, 8)
    assert np.array_equal(t[:4, :5], np.asarray([GC.ROWS_B[i] for i in (0, 1, 2, 0)], np.float32))
    assert t[:4, 5].tolist() == [1.0, 0.0, 0.0, 1.0] and (t[:4, 6:] == 0).all() and np.isnan(t[4:]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the folded first-layer update: a decoupled row, and one row per parameter
# ---------------------------------------------------------------------------------------------------------------------------
FOLD_ROWS = {'single': [(1e-3, .9, .999, 1e-8, 1e-2, True)],
             'per_parameter': [(1e-3, .9, .999, 1e-8, 1e-2, True), (5e-3, .9, .999, 1e-8, 0.0, False)]}


# (the step by value at every shape; read from the device at the smallest)
FOLD_SHAPES = [pytest.param(256, 33, [256, 512], 'f32', 2, 'by_value', id='256-33-f32-2'),
               pytest.param(256, 33, [256, 512], 'f32', 2, 'step_dev', id='256-33-f32-2-step_dev7'),
               pytest.param(256, 256, [256, 512], 'q16c', 3, 'by_value', id='256-256-q16c-3'),
               pytest.param(256, 257, [256, 512], 'q16c', 3, 'by_value', id='256-257-q16c-3')]


@pytest.mark.parametrize('rows_kind', sorted(FOLD_ROWS))
@pytest.mark.parametrize('J,rows,dims,storage,mode,step_form', FOLD_SHAPES)
def test_folded_first_layer_update(J, rows, dims, storage, mode, step_form, rows_kind):
    """tests/test_gpu_layer1_persistent.py::test_fused_first_layer_adam with the hyper-parameters read from a table: `single` --
    lirec_set_adam_hyper_row, the row decoupled; `per_parameter` -- lirec_set_adam_hyper_map, the weights in a decoupled group
    (wd 1e-2), the biases in a coupled one with wd 0 and another lr.  Parameters and moments: bit for bit the unfused gradient
    followed by ONE lirec_adam_step_groups launch with the same table; the shadow: the conversion of the new weights; nothing
    outside W1 / b1 is touched."""
    g = torch.Generator().manual_seed(J + rows)
    h = TP.Head('plain', rows, J, dims, 0)
    D = (sum(dims) + 63) // 64 * 64
    X0 = TP.make_block(rows, 2, D, g)
    X, Xref = TP.stored(X0, storage)
    ops.ensure_scratch(DEV)
    offs, o = [], 0
    for d in dims:
        offs.append(o); o += J * d
    w_end, boffs = o, []
    for _ in dims:
        boffs.append(o); o += J
    b_end = o
    n = (o + 63) // 64 * 64
    n_params = sum(J * d + J for d in dims)
    flat = torch.zeros(n, device=DEV)
    s = TP.setup_head(h, X, Xref, 2, D, mode, 0.3, g)
    for i, d in enumerate(dims):
        flat[offs[i]:offs[i] + J * d].copy_(s['W1'][i].view(-1)); s['W1'][i] = flat[offs[i]:offs[i] + J * d].view(J, d)
        flat[boffs[i]:boffs[i] + J].copy_(s['b1'][i]); s['b1'][i] = flat[boffs[i]:boffs[i] + J]
    s['W1ref'] = [TP.bf(w).double() if mode == 3 else w.double() for w in s['W1']]
    gflat0 = (torch.randn(n, generator=g) * 0.01).to(DEV)
    m0 = (torch.randn(n, generator=g) * 0.01).to(DEV)
    v0 = (torch.rand(n, generator=g) * 1e-4).to(DEV)
    step = 3 if step_form == 'by_value' else 0
    step_dev = None if step_form == 'by_value' else torch.tensor([7], dtype=torch.int64, device=DEV)
    table = _table(FOLD_ROWS[rows_kind])
    if rows_kind == 'single':
        ranges = [(0, b_end, 0, 0)]
        setting = lambda: ops.adam_hyper_row(table[0:8])
    else:
        ranges = [(0, w_end, 0, 0), (w_end, b_end - w_end, 0, 1)]
        setting = lambda: ops.adam_hyper_map(table, [(a, k, grp) for a, k, _, grp in ranges])
    L = _lib.lib()
    ops.set_gemm_mode(mode)
    try:
        p0 = flat.clone()
        ops.profile_enable(True)
        ops.embed_fwd(args=TP.fwd_args(h, s, X, D))
        fs = TP.prof_sites()
        TP.check_forward(h, s, mode, 0.3, 'adamw fwd')
        TP.init_grads(h, s, True, g)
        results = []
        for fused in (False, True):
            gflat = gflat0.clone()
            s['gW1'] = [gflat[offs[i]:offs[i] + J * d].view(J, d) for i, d in enumerate(dims)]
            s['gb1'] = [gflat[boffs[i]:boffs[i] + J] for i in range(len(dims))]
            for t, t0 in zip(s['gW1'] + s['gb1'], s['g0'][:2 * len(dims)]):
                t0.copy_(t)
            for t, t0 in zip(s['gW2'] + s['gb2'], s['g0'][2 * len(dims):]):
                t.copy_(t0)
            flat.copy_(p0)
            m, v = m0.clone(), v0.clone()
            wq = torch.zeros(4 * n, dtype=torch.uint8, device=DEV)
            # (the five by-value values are ignored under either setting: deliberately other ones)
            adam = ops.fused_adam_args(flat, gflat, m, v, n_params, step, 0.5, 0.1, 0.2, 1e-3, 0.25, grad_scale=GC.GRAD_SCALE,
                                       step_dev=step_dev, wq=wq, wq_first=0) if fused else None
            ops.profile_enable(True)
            if fused:
                with setting():
                    ops.embed_bwd(args=TP.bwd_args(h, s, X, D, adam=adam))
            else:
                ops.embed_bwd(args=TP.bwd_args(h, s, X, D, adam=None))
            TP.assert_persistent(fs, TP.prof_sites())
            results.append((gflat.clone(), flat.clone(), m, v, wq))
    finally:
        ops.profile_enable(False)
        L.lirec_debug_set(0, -1)
        ops.set_gemm_mode(_lib.default_gemm_mode())
    (g1, _, _, _, _), (g2, p2, m2, v2, wq) = results
    assert torch.equal(g1, g2), 'the fused call stores another gradient'
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    ops.adam_step_groups(pr, g1, mr, vr, ranges, table, len(FOLD_ROWS[rows_kind]), step, GC.GRAD_SCALE, step_dev=step_dev)
    rng = torch.zeros(n, dtype=torch.bool, device=DEV)
    rng[:b_end] = True
    for got, want, orig, what in ((p2, pr, p0, 'parameters'), (m2, mr, m0, 'exp_avg'), (v2, vr, v0, 'exp_avg_sq')):
        assert torch.equal(got[rng], want[rng]), (what + ' differ from lirec_adam_step_groups on the unfused gradient', int((got[rng] != want[rng]).sum()))
        assert torch.equal(got[~rng], orig[~rng]), what + ': outside W1 / b1'
    assert bool((pr[rng] != p0[rng]).any()) and bool((vr[rng] != v0[rng]).any())
    # ... which is the decoupled rule, not the coupled one with the same values (host restatement, the weights' range)
    hw = AC.hyper32(FOLD_ROWS[rows_kind][0][:5] + (GC.GRAD_SCALE,))
    t = 3 if step_dev is None else 7
    a = (_np(p0[:w_end]), _np(g1[:w_end]), _np(m0[:w_end]), _np(v0[:w_end]))
    assert _same(_np(p2[:w_end]), WC.ref32w(*a, t, hw)[0]) and not _same(_np(p2[:w_end]), AC.ref32(*a, t, hw)[0])
    if rows_kind == 'per_parameter':
        hb = AC.hyper32(FOLD_ROWS[rows_kind][1][:5] + (GC.GRAD_SCALE,))
        a = (_np(p0[w_end:b_end]), _np(g1[w_end:b_end]), _np(m0[w_end:b_end]), _np(v0[w_end:b_end]))
        assert _same(_np(p2[w_end:b_end]), AC.ref32(*a, t, hb)[0]), 'the biases were not updated with the row of their own group'
    for i, d in enumerate(dims):
        neww = pr[offs[i]:offs[i] + J * d].view(J, d).contiguous()
        if mode == 3:
            want = ops.to_q16c(neww).data[:int(L.lirec_q16b_bytes(J, d))]
        else:
            want = ops.to_q32b(neww).data[:int(L.lirec_q32b_bytes(J, d))]
        assert torch.equal(wq[4 * offs[i]:4 * offs[i] + want.numel()], want), 'W1[%d] shadow differs from the conversion of the new weights' % i


def test_a_map_that_misses_a_parameter_is_refused():
    """a folded update under a map that does not hold every weight and bias of the call: LIREC_EINVAL from the launch that would
    have applied it -- parameters and moments untouched"""
    L = _lib.lib()
    J, dims = 256, [256]
    g = torch.Generator().manual_seed(1)
    h = TP.Head('plain', 33, J, dims, 0)
    D = 256
    X, Xref = TP.stored(TP.make_block(33, 2, D, g), 'f32')
    ops.ensure_scratch(DEV)
    n = J * 256 + J
    flat = torch.zeros(n, device=DEV)
    s = TP.setup_head(h, X, Xref, 2, D, 2, 0.3, g)
    flat[:J * 256].copy_(s['W1'][0].view(-1)); s['W1'][0] = flat[:J * 256].view(J, 256)
    flat[J * 256:].copy_(s['b1'][0]); s['b1'][0] = flat[J * 256:]
    s['W1ref'] = [w.double() for w in s['W1']]
    ops.set_gemm_mode(2)
    try:
        ops.embed_fwd(args=TP.fwd_args(h, s, X, D))
        TP.check_forward(h, s, 2, 0.3, 'adamw refused fwd')
        TP.init_grads(h, s, True, g)
        gflat, m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        s['gW1'], s['gb1'] = [gflat[:J * 256].view(J, 256)], [gflat[J * 256:]]
        p0 = flat.clone()
        adam = ops.fused_adam_args(flat, gflat, m, v, n, 3, 1e-3, .9, .999, 1e-8, 0.0, wq=None, wq_first=0)
        with ops.adam_hyper_map(_table(FOLD_ROWS['per_parameter']), [(0, J * 256, 0)]):          # (the bias is in no entry)
            with pytest.raises(_lib.LirecError, match=r'embed_bwd.*\(code %d\)' % _lib.LIREC_EINVAL):
                ops.embed_bwd(args=TP.bwd_args(h, s, X, D, adam=adam))
        torch.cuda.synchronize()
        assert torch.equal(flat, p0) and not bool(m.any()) and not bool(v.any())
    finally:
        L.lirec_debug_set(0, -1)
        ops.set_gemm_mode(_lib.default_gemm_mode())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. FusedAdam.step(): the small model, weights decoupled at 1e-2, biases at 0
# ---------------------------------------------------------------------------------------------------------------------------
def _check_step(model, optim, before, grad, after, step, what, coef=1.0, rs=None, rows=None):
    """TG._check_step with the flag: every element of the flat buffers -- the trainable parameters within the bounds of the
    yardstick of their group's rule, fed the device's own gradient; alignment gaps and frozen parameters bit for bit as they were"""
    rows = WC.rows_of(optim) if rows is None else rows
    before, after, grad = [_np(t) if torch.is_tensor(t) else t for t in before], [_np(t) if torch.is_tensor(t) else t for t in after], \
        (_np(grad) if torch.is_tensor(grad) else grad)
    rs = GC.model_ranges(model, optim) if rs is None else rs
    flags = [r[5] for r in rows]
    use = WC.use_of_bounds(after, before[0], grad, before[1], before[2], rs, step, rows, flags, optim.grad_scale, coef)
    _fig('fused_adam', route=what, step=step, p=use[0], m=use[1], v=use[2])
    assert max(use) <= 1.0, (what, step, use)
    mask = GC.inside(rs, len(grad))
    for a, b, w in zip(after, before, 'pmv'):
        assert _same(a[~mask], b[~mask]), (what, step, w, 'written outside the trainable parameters')
    return use


@pytest.fixture
def flagged(monkeypatch):
    """the routes of tests/test_gpu_groups.py with the yardstick that knows the flag"""
    monkeypatch.setattr(TG, '_check_step', _check_step)
    monkeypatch.setattr(GC, 'rows_of', WC.rows_of)


def _small(side, **kw):
    from lirec_amd import model as M
    from lirec_amd.data import synthetic_batch, to_device_batch
    config.recipe('int_rel_ch', joint_dim=GC.JOINT, rels_n_clips=GC.R, dropout=0.3, dropout_seed=77, **GC.DIMS)
    opt.device = 'cuda'
    opt.adam_on_side_stream = side
    torch.manual_seed(3)
    model, loss, _ = M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)
    model.train()
    optim = FusedAdam(model, lr=WC.LR, param_groups=WC.two_groups(model), **kw)
    batch = to_device_batch(synthetic_batch(5, 'int_rel_ch', GC.B, n_classes=GC.N_CLASSES, n_rels=GC.N_RELS, T=GC.T, R=GC.R, **GC.DIMS), 'cuda')
    return model, loss, optim, batch


STEPS = 3
_frozen_end = {}           # route -> (p, m, v) after the three steps of the frozen test


def _three_routes(make, between=None):
    return [TG._route(r, make, steps=STEPS, between=between) for r in ('plain', 'side', 'recorded')]


def _routes_agree(plain, side, rec):
    TG._agree(plain, side, 'plain vs side stream', range(1, STEPS + 1))
    TG._agree(side, rec, 'eager vs recorded', range(2, STEPS + 1))
    assert rec['state'][1:] == [STEPS, STEPS]


def test_two_groups_on_every_route(flagged):
    plain, side, rec = _three_routes(_small)
    _routes_agree(plain, side, rec)
    # the decay reached the weights: the same groups coupled end elsewhere
    def coupled(side_):
        m = _small(side_)
        m[2].param_groups[0]['decoupled_weight_decay'] = False
        return m
    other = TG._route('plain', coupled, steps=STEPS)
    assert not _same(plain[STEPS][0], other[STEPS][0])


def test_two_groups_clipped(flagged, monkeypatch):
    """max_grad_norm set: the clip scales g only, the decay is not clipped -- the bounds hold with the coefficient the step
    reports, in the eager loop and in the recorded step, which agree bit for bit"""
    def check(model, optim, before, grad, after, step, what, coef=1.0, rs=None, rows=None):
        return _check_step(model, optim, before, grad, after, step, what, coef=float(optim.clip_coef), rs=rs, rows=rows)
    monkeypatch.setattr(TG, '_check_step', check)
    coefs = []
    make = lambda side: _small(side, max_grad_norm=0.01)
    plain = TG._route('plain', make, steps=STEPS, between=lambda s, optim: coefs.append(float(optim.clip_coef)))
    # (a clipped update runs whole on the caller's stream -- the coefficient needs every gradient --: there is no side route)
    rec = TG._route('recorded', make, steps=STEPS)
    assert coefs and max(coefs) < 1.0, ('max_grad_norm never clipped: the test shows nothing', coefs)
    TG._agree(plain, rec, 'eager vs recorded, clipped', range(2, STEPS + 1))


@pytest.mark.parametrize('route', ['plain', 'side'])
def test_two_groups_with_a_parameter_frozen_for_a_step(flagged, route):
    """two weights of the decoupled group frozen for step 2 and released: no update and NO DECAY while frozen (its bits stay), one
    step behind afterwards -- a lagging decoupled range, on the side route in the side stream's grouped update --; every step
    within the bounds; the two routes agree bit for bit"""
    try:
        model, loss, optim, batch = _small(route == 'side')
        # (one in the embeddings -- updated on the caller's stream -- and one in the heads: the first bucket, the side stream's share)
        frozen = ['vis2_ctx.weight', 'out_ctx.weight']
        pd = dict(model.named_parameters())
        assert all(n in WC.two_groups(model)[0]['params'] for n in frozen) and model.param_group_of(frozen[1]) == 'out_ctx'
        where = [model._offsets[n] for n in frozen]
        for s in range(1, 4):
            for n in frozen:
                pd[n].requires_grad_(s != 2)
            TG._backward(model, loss, optim, batch)
            before, grad = [_np(t) for t in TG._snap(model, optim)], _np(model.flat_grads(attach=False))
            rs = GC.model_ranges(model, optim)
            optim.step()
            torch.cuda.synchronize()
            after = [_np(t) for t in TG._snap(model, optim)]
            assert bool(model.lanes.bucket0_on_side) == (route == 'side'), 'the step took another route'
            _check_step(model, optim, before, grad, after, s, 'frozen-' + route, rs=rs)
            for fo, fk in where:
                if s == 2:
                    assert all(_same(a[fo:fo + fk], b[fo:fo + fk]) for a, b in zip(after, before)) and len(rs) == 36
                else:
                    assert not _same(after[0][fo:fo + fk], before[0][fo:fo + fk])
        assert optim._lag == {n: 1 for n in frozen}
        _frozen_end[route] = after
        if len(_frozen_end) == 2:
            for a, b, w in zip(_frozen_end['plain'], _frozen_end['side'], 'pmv'):
                assert _same(a, b), (w, 'plain and side route differ with a parameter frozen for a step')
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the dimensions where the persistent kernels run: the fold armed across two groups
# ---------------------------------------------------------------------------------------------------------------------------
BB, BT, BR = 8, 16, 18


def _big(side, hold=None):
    """the `big` dims of tests/host_dryrun.py (768 / 2048 / 2048, J = 512), q32b feature storage, the two groups"""
    from lirec_amd import model as M
    from lirec_amd.data import synthetic_batch, to_device_batch
    from oracle import lirec_oracle as O
    config.recipe('int_rel_ch', rels_n_clips=BR, dropout_seed=77, lr=WC.LR)
    opt.device = 'cuda'
    opt.adam_on_side_stream = side
    model, loss, _ = M.create_model(101, n_rels=15)
    optim = FusedAdam(model, lr=WC.LR, param_groups=WC.two_groups(model, lr_bias=3e-3))
    model.load_state_dict(O.fill_params(O.param_shapes(O.OracleCfg(), 101, 15), 5), strict=True)
    model.train()
    batch = to_device_batch(synthetic_batch(11, 'int_rel_ch', BB, T=BT, R=BR), 'cuda')
    batch['features'] = ops.to_q32b(batch['features'].float().contiguous())
    if hold is not None:
        lane = model._wgrad_lane()
        assert lane is not None
        with lane[1]:
            _lib.lib().lirec_debug_set(131072, -1)
        hold.append(lane)
    return model, loss, optim, batch


def _release(held):
    for lane in held:
        with lane[1]:
            _lib.lib().lirec_debug_set(0, -1)


def test_recorded_step_with_the_fold_armed_across_two_groups():
    """weights that decay and biases that do not split every first layer over two groups: the recorded step keeps the headline form
    (overwrite mode, the first-layer update folded in -- one row per parameter --, the side join deferred) and equals the eager
    loop bit for bit after three steps: parameters and both moments, and the gradients of the last step; the W1 shadow is the
    conversion of the weights"""
    grads = {}

    def make(side):
        return _big(side)
    eager = TG._route('side', make, steps=STEPS, check=False, between=lambda s, o: grads.__setitem__(('eager', s), o.model.flat_grads(attach=False).clone()))
    rec = TG._route('recorded', make, steps=STEPS, check=False, between=lambda s, o: grads.__setitem__(('rec', s), o.model.flat_grads(attach=False).clone()))
    assert rec['flags'] == (True, True, True), rec['flags']
    TG._agree(eager, rec, 'eager vs recorded, fold armed across two groups', range(2, STEPS + 1))
    assert rec['shadow_ok'] and rec['state'][1:] == [STEPS, STEPS]
    assert _same(grads[('eager', STEPS)], grads[('rec', STEPS)]), 'the gradients of the last step differ'


def test_lr_and_flag_change_in_front_of_every_replay_with_the_side_stream_held_back():
    """lr of both groups and the flag of one group change in front of EVERY replay while the side stream's share of each step --
    the heads' and the gate's update among it -- starts after the main stream has begun the next step: each update reads ITS
    step's table (one per issuing stream, written on that stream).  The eager loop's bits."""
    def between(s, optim):
        for grp in optim.param_groups:
            grp['lr'] = grp['lr'] * 0.8
        k = s % 2
        optim.param_groups[k]['decoupled_weight_decay'] = not optim.param_groups[k]['decoupled_weight_decay']
        if k == 1:
            optim.param_groups[1]['weight_decay'] = 1e-2 if optim.param_groups[1]['decoupled_weight_decay'] else 0.0
    steps = 6
    eager = TG._route('side', _big, steps=steps, check=False, between=between)
    held = []
    try:
        rec = TG._route('recorded', lambda side: _big(side, hold=held), steps=steps, check=False, between=between)
    finally:
        _release(held)
    assert rec['flags'] == (True, True, True), rec['flags']
    TG._agree(eager, rec, 'eager vs replays with the side stream held back', range(2, steps + 1))
    assert rec['shadow_ok']
