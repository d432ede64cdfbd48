"""Decoupled weight decay (AdamW) per parameter group without a GPU: the yardstick of tests/test_gpu_adamw.py against
torch.optim.AdamW and torch.optim.Adam(decoupled_weight_decay=True) in float64; the fp32 restatement under HALF of every bound on
every case the GPU file runs; an invisible decay gives the bits of wd = 0; the constructor, the groups and how device_hyper
resolves; checkpoints to a stock AdamW and back, flat checkpoints; lirec_set_adam_hyper_map's argument checks through the C ABI
(LIREC_EINVAL before any device call), with and without the library's host-side dry run; a recorded step with two groups whose
flag and learning rate change between replays, in the dry run; the ABI's numbers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_cases as AC
import adamw_cases as WC
import group_cases as GC
from lirec_amd import _lib, config, ops, util
from lirec_amd.config import opt
from lirec_amd.graph import RecordedTrainStep
from lirec_amd.optim import FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL


def _model(kind='int_rel_ch', **kw):
    from lirec_amd import model as M
    config.recipe(kind, joint_dim=GC.JOINT, rels_n_clips=GC.R, dropout=0.3, dropout_seed=7, **GC.DIMS, **kw)
    opt.device = 'cpu'
    torch.manual_seed(3)
    return M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)


@pytest.fixture(autouse=True)
def _reset():
    yield
    config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick is torch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stock', ['AdamW', 'Adam(decoupled_weight_decay=True)'])
def test_ref64w_is_torch_adamw_in_float64(stock):
    """six parameters in three groups of mixed flags (tables A and B of the kernel cases: groups 0 and 2 decoupled, group 1
    coupled), three steps, parameter 3 frozen for the second: the yardstick range by range against torch on float64 CPU tensors
    with the same groups, fed g * grad_scale (a power of two: exact), to 1e-12 relative -- the tolerance tests/test_host_groups.py
    uses for the coupled rule"""
    worst = 0.0
    for name, (rows5, flags) in WC.TABLES.items():
        sizes, group_of = [5, 7, 16, 3, 9, 4], [0, 1, 2, 0, 1, 2]
        rows = [AC.hyper32(tuple(r) + (1.0,))[:5] for r in rows5]
        r = np.random.default_rng(5)
        offs, at = [], 0
        for k in sizes:
            offs.append(at)
            at = (at + k + 3) // 4 * 4
        p = np.zeros(at, np.float32)
        for o, k in zip(offs, sizes):
            p[o:o + k] = (0.1 * r.standard_normal(k)).astype(np.float32)
        params = [torch.nn.Parameter(torch.from_numpy(p[o:o + k].astype(np.float64))) for o, k in zip(offs, sizes)]
        groups = [dict(params=[q for q, g in zip(params, group_of) if g == i], lr=rows[i][0], betas=rows[i][1:3], eps=rows[i][3],
                       weight_decay=rows[i][4], decoupled_weight_decay=flags[i]) for i in range(3)]
        if stock == 'AdamW':
            ref = torch.optim.AdamW(groups)
            for g, f in zip(ref.param_groups, flags):          # (AdamW's default is True; the groups say what they are)
                assert g['decoupled_weight_decay'] == f
        else:
            ref = torch.optim.Adam(groups, decoupled_weight_decay=True)
        P, M, V = p.astype(np.float64), np.zeros(at), np.zeros(at)
        lag = [0] * len(sizes)
        for step in (1, 2, 3):
            g = np.zeros(at, np.float32)
            for o, k in zip(offs, sizes):
                g[o:o + k] = r.standard_normal(k).astype(np.float32)
            frozen = {3} if step == 2 else set()
            for i, (q, o, k) in enumerate(zip(params, offs, sizes)):
                q.grad = None if i in frozen else torch.from_numpy(g[o:o + k].astype(np.float64) * GC.GRAD_SCALE)
            ref.step()
            rs = [(o, k, lag[i], group_of[i]) for i, (o, k) in enumerate(zip(offs, sizes)) if i not in frozen]
            before = P.copy()
            P, M, V = WC.ref64(P, g, M, V, rs, step, rows, flags, GC.GRAD_SCALE)[:3]
            for i in frozen:                                   # a frozen parameter gets no decay
                assert np.array_equal(P[offs[i]:offs[i] + sizes[i]], before[offs[i]:offs[i] + sizes[i]])
                lag[i] += 1
            for i, (q, o, k) in enumerate(zip(params, offs, sizes)):
                st = ref.state[q]
                assert int(st['step']) == step - lag[i]
                for got, want in ((P[o:o + k], q.detach().numpy()), (M[o:o + k], st['exp_avg'].numpy()), (V[o:o + k], st['exp_avg_sq'].numpy())):
                    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
                    worst = max(worst, float(err.max()))
                    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (name, step, i, float(err.max()))
    print('ref64w per group against torch.optim.%s (float64): worst relative difference %.3g' % (stock, worst))


@pytest.mark.parametrize('coef', [1.0, GC.COEF])
@pytest.mark.parametrize('table', sorted(WC.TABLES))
@pytest.mark.parametrize('step', GC.STEPS)
def test_fp32_restatement_stays_under_half_of_the_bounds(step, table, coef):
    """every kernel case of tests/test_gpu_adamw.py (three steps, both tables, unclipped and clipped): ref32 range by range uses less
    than HALF of every bound (the rule of tests/test_host_optim.py) -- on the decoupled ranges, where the rule is new, and on the
    whole buffer less than 1.0 as tests/test_host_groups.py has it for the coupled rule"""
    rows, flags = WC.TABLES[table]
    s, rs = GC.build(step)
    got = WC.ref32(*s, rs, step, rows, flags, GC.GRAD_SCALE, coef)
    dec = [r for r in rs if flags[r[3]]]
    use_w = WC.use_of_bounds(got, *s, dec, step, rows, flags, GC.GRAD_SCALE, coef)
    use = WC.use_of_bounds(got, *s, rs, step, rows, flags, GC.GRAD_SCALE, coef)
    print('step %d table %s coef %g: use of the bounds, decoupled ranges p %.3f m %.3f v %.3f; all ranges %.3f' % (step, table, coef, *use_w, max(use)))
    assert max(use_w) < 0.5, use_w
    assert max(use) < 1.0, use
    mask = GC.inside(rs, len(s[0]))
    for a, b in zip(got, (s[0], s[2], s[3])):
        assert np.array_equal(a[~mask], b[~mask])


@pytest.mark.parametrize('row', range(4))
@pytest.mark.parametrize('step', [1, 3, 1000])
def test_fp32_restatement_of_the_big_and_model_cases(row, step):
    """the rows on their own, at adam_cases.N_HOST elements and the magnitudes of adam_cases (the big range, and what a model's
    gradients may look like): under half of every bound"""
    h = AC.hyper32(tuple((WC.ROWS_W + [WC.ROW_INVISIBLE])[row]) + (GC.GRAD_SCALE,))
    for mag in (1.0, 1e-3):
        s = AC.make_state(AC.Case(0, step, mag), AC.N_HOST)
        got = WC.ref32w(*s, step, h)
        pn, mn, vn, G, A, V = WC.ref64w(*s, step, h)
        use = [float((np.abs(x.astype(np.float64) - r) / b).max()) for x, r, b in zip(got, (pn, mn, vn), AC.bounds(s[0], s[2], G, A, V))]
        assert max(use) < 0.5, (mag, use)


def test_an_invisible_decay_gives_the_bits_of_no_decay():
    """lr wd < 2^-25 (the reference's defaults, 3e-5 x 1e-5): d == 1.0f and the decoupled update is the update with wd = 0, bit
    for bit -- as torch's fp32 mul_ by 1 - lr wd leaves the parameter alone; a visible row moves it"""
    h = AC.hyper32(WC.ROW_INVISIBLE + (1.0,))
    assert WC.decay32(h) == np.float32(1.0) and 1.0 - h[0] * h[4] < 1.0
    h0 = h[:4] + (0.0,) + h[5:]
    for step in (1, 3, 1000):
        s = AC.make_state(AC.Case(0, step, 1.0), AC.N_HOST)
        a, b, c = WC.ref32w(*s, step, h), WC.ref32w(*s, step, h0), AC.ref32(*s, step, h0)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32))
        q = torch.from_numpy(s[0].copy())
        q.mul_(1 - h[0] * h[4])
        assert np.array_equal(q.numpy().view(np.uint32), s[0].view(np.uint32))
    for row in WC.ROWS_W:
        hv = AC.hyper32(tuple(row) + (1.0,))
        assert WC.decay32(hv) < np.float32(1.0) and hv[0] * hv[4] >= 0.99e-5
        s = AC.make_state(AC.Case(0, 3, 1.0), AC.N_HOST)
        assert not np.array_equal(WC.ref32w(*s, 3, hv)[0], WC.ref32w(*s, 3, hv[:4] + (0.0,) + hv[5:])[0])


# ---------------------------------------------------------------------------------------------------------------------------
# the constructor, the groups, device_hyper
# ---------------------------------------------------------------------------------------------------------------------------
def test_constructor_and_groups():
    model, _, plain = _model()
    assert plain.defaults['decoupled_weight_decay'] is False and not plain.device_hyper
    assert plain.hyper_rows() == ((3e-5, 0.9, 0.999, 1e-8, 1e-5, False),)
    # the global flag: one group, decoupled -- the table route switches on
    fo = FusedAdam(model, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True)
    assert fo.defaults['decoupled_weight_decay'] is True and fo.param_groups[0]['decoupled_weight_decay'] is True
    assert fo.device_hyper and fo.hyper_rows() == ((1e-3, 0.9, 0.999, 1e-8, 1e-2, True),)
    assert fo.trainable_ranges() == [(0, model.flat_params().numel(), 0, 0)]
    assert FusedAdam(model, decoupled_weight_decay=True, device_hyper=True).device_hyper
    with pytest.raises(ValueError, match='decoupled_weight_decay.*device_hyper'):
        FusedAdam(model, decoupled_weight_decay=True, device_hyper=False)
    # per group: the usual grouping
    two = FusedAdam(model, lr=1e-3, param_groups=WC.two_groups(model))
    assert two.device_hyper and [g['decoupled_weight_decay'] for g in two.param_groups] == [True, False]
    assert two.hyper_rows() == ((1e-3, 0.9, 0.999, 1e-8, 1e-2, True), (1e-3, 0.9, 0.999, 1e-8, 0.0, False))
    assert [r[:5] for r in two.hyper_rows()] == [tuple(r) for r in GC.rows_of(two)]          # (index-based reads keep working)
    # the global flag is the groups' default, a group may say otherwise
    mixed = FusedAdam(model, decoupled_weight_decay=True, param_groups=[dict(g, **({'decoupled_weight_decay': False} if i else {}))
                                                                       for i, g in enumerate(GC.three_groups(model))])
    assert [r[5] for r in mixed.hyper_rows()] == [True, False, False]
    # one explicit group, decoupled, with device_hyper=False: refused; a coupled one stays the by-value path
    names = [n for n, _ in model.named_parameters()]
    with pytest.raises(ValueError, match='device_hyper'):
        FusedAdam(model, param_groups=[dict(params=names, decoupled_weight_decay=True)], device_hyper=False)
    assert not FusedAdam(model, param_groups=[dict(params=names)]).device_hyper
    # a loop sets the key later: left to default the route switches on, an explicit False raises -- in hyper_rows() too
    late = FusedAdam(model)
    key = RecordedTrainStep.hyper_key(late)
    late.param_groups[0]['decoupled_weight_decay'] = True
    assert not late.device_hyper                       # (reading the attribute resolves nothing ...)
    assert late.hyper_rows()[0][5] is True and late.device_hyper                   # (... hyper_rows() / step() / the key do)
    assert late.trainable_ranges()[0] == (0, model.flat_params().numel(), 0, 0)
    assert RecordedTrainStep.hyper_key(late) != key and RecordedTrainStep.hyper_key(late)[0][0] == 'device_hyper'
    never = FusedAdam(model, device_hyper=False)
    never.param_groups[0]['decoupled_weight_decay'] = True
    with pytest.raises(ValueError, match='device_hyper=False'):
        never.hyper_rows()
    with pytest.raises(ValueError, match='device_hyper=False'):
        RecordedTrainStep.hyper_key(never)
    # the key of a recorded step under device_hyper keeps its shape: the flag is a table value
    k2 = RecordedTrainStep.hyper_key(two)
    assert k2 == (('device_hyper', two.group_membership()), 1.0)
    two.param_groups[1]['decoupled_weight_decay'] = True
    two.param_groups[0]['decoupled_weight_decay'] = False
    assert RecordedTrainStep.hyper_key(two) == k2 and [r[5] for r in two.hyper_rows()] == [False, True]
    with pytest.raises(ValueError, match='amsgrad'):
        FusedAdam(model, amsgrad=True, decoupled_weight_decay=True)


def test_create_model_passes_the_config_key():
    assert opt.decoupled_weight_decay is False
    _, _, optim = _model(decoupled_weight_decay=True, weight_decay=1e-2)
    assert optim.param_groups[0]['decoupled_weight_decay'] is True and optim.device_hyper and optim.hyper_rows()[0][4:] == (1e-2, True)
    _, _, optim = _model()
    assert optim.param_groups[0]['decoupled_weight_decay'] is False and not optim.device_hyper


def test_first_layer_fold_ranges():
    """weights that decay and biases that do not: the first layers span two groups, and the fold takes them as ranges with their
    groups, each a run of whole parameters; a frozen or lagging first-layer parameter declines"""
    model, _, _ = _model()
    two = FusedAdam(model, lr=1e-3, param_groups=WC.two_groups(model))
    lo, hi, n_params = model.first_layer_range()
    rs = two.first_layer_fold_ranges()
    assert rs is not None and 1 < len(rs) <= _lib.ADAM_MAP_MAX == 16
    mem = dict(zip(two._names, two.group_membership()))
    covered = 0
    for a, b, lag, grp in rs:
        inside = [n for n, (o, k) in model._offsets.items() if o >= a and o + k <= b]
        assert lag == 0 and inside and all(mem[n] == grp for n in inside) and a >= lo
        covered += sum(model._offsets[n][1] for n in inside)
    assert covered == n_params
    assert {grp for *_, grp in rs} == {0, 1}
    # the three groups of group_cases: armed now
    assert FusedAdam(model, param_groups=GC.three_groups(model)).first_layer_fold_ranges() is not None
    one = FusedAdam(model, device_hyper=True).first_layer_fold_ranges()
    assert len(one) == 1 and one[0][0] == lo and one[0][2:] == (0, 0)
    name = next(n for n, (o, k) in model._offsets.items() if o >= lo and n.endswith('.bias'))
    dict(model.named_parameters())[name].requires_grad_(False)
    assert two.first_layer_fold_ranges() is None
    dict(model.named_parameters())[name].requires_grad_(True)
    two._lag = {name: 1}
    two._ranges_key = None
    assert two.first_layer_fold_ranges() is None


def test_five_element_rows_are_still_accepted():
    """ops.adam_hyper_write: rows of five are coupled rows; a sixth element is the flag, stored as 1.0 / 0"""
    seen = []

    class Lib:
        def lirec_adam_hyper_write(self, table, arr, n, stream):
            seen.append([(a.lr, a.weight_decay, a.decoupled, tuple(a.reserved_)) for a in arr[:n]])
            return 0
    t = torch.zeros(64)
    saved = ops.lib, ops._p, ops._stream
    ops.lib, ops._p, ops._stream = (lambda: Lib()), (lambda x: None), (lambda: None)
    try:
        ops.adam_hyper_write(t, GC.ROWS_B)
        ops.adam_hyper_write(t, WC.rows6(*WC.TABLES['A']))
        ops.adam_hyper_write(t, [GC.ROWS_B[0] + (0,), GC.ROWS_B[1] + (7,)])
    finally:
        ops.lib, ops._p, ops._stream = saved
    f = lambda x: float(np.float32(x))
    assert seen[0] == [(f(r[0]), f(r[4]), 0.0, (0.0, 0.0)) for r in GC.ROWS_B]
    assert [x[2] for x in seen[1]] == [1.0, 0.0, 1.0] and [x[2] for x in seen[2]] == [0.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------------
def _stock(model, fo, cls):
    clone = {id(p): torch.nn.Parameter(p.detach().clone()) for p in model.parameters()}
    groups = [dict({k: v for k, v in g.items() if k in ('lr', 'betas', 'eps', 'weight_decay', 'decoupled_weight_decay')},
                   params=[clone[id(p)] for p in g['params']]) for g in fo.param_groups]
    return (torch.optim.AdamW(groups) if cls == 'AdamW' else torch.optim.Adam(groups, decoupled_weight_decay=True)), clone


def _fill_state(model, fo):
    """moments and steps as after a few updates, one parameter two behind (the update itself needs the GPU)"""
    fo._ensure_state()
    torch.manual_seed(11)
    live = torch.zeros(fo._m.numel(), dtype=torch.bool)
    for o, k in model._offsets.values():
        live[o:o + k] = True
    fo._m.copy_(torch.randn_like(fo._m) * live)
    fo._v.copy_(torch.rand_like(fo._v) * live)
    fo._step = 7
    fo._lag = {'vis2_ctx.weight': 2}


@pytest.mark.parametrize('cls', ['AdamW', 'Adam'])
def test_state_dict_to_a_stock_adamw_and_back(cls):
    model, _, _ = _model()
    fo = FusedAdam(model, lr=1e-3, param_groups=WC.two_groups(model, lr_bias=5e-3))
    _fill_state(model, fo)
    sd = fo.state_dict()
    assert [g['decoupled_weight_decay'] for g in sd['param_groups']] == [True, False]
    ref, clone = _stock(model, fo, cls)
    ref.load_state_dict(sd)
    for g, h in zip(ref.param_groups, fo.param_groups):
        for k in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad'):
            assert g[k] == h[k], k
        # (torch.optim.AdamW sets the key in EVERY group of a state it loads -- its __setstate__ --: the biases' group comes back
        #  decoupled, which with its weight_decay of 0 is the same update; torch.optim.Adam keeps the groups' own flags)
        assert g['decoupled_weight_decay'] == (True if cls == 'AdamW' else h['decoupled_weight_decay'])
        for q, p in zip(g['params'], h['params']):
            for k in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(ref.state[q][k], fo.state[p][k])
            assert float(ref.state[q]['step']) == float(fo.state[p]['step'])
    # ... and back, into an optimiser with the same groups built WITHOUT the flag and with device_hyper left to default
    model2, _, _ = _model()
    fo2 = FusedAdam(model2, lr=3e-5, param_groups=[dict(params=g['params']) for g in WC.two_groups(model2)])
    assert [r[5] for r in fo2.hyper_rows()] == [False, False]
    fo2.load_state_dict(ref.state_dict())
    assert [r[:5] for r in fo2.hyper_rows()] == [r[:5] for r in fo.hyper_rows()] and fo2.device_hyper
    assert [r[5] for r in fo2.hyper_rows()] == ([True, True] if cls == 'AdamW' else [True, False])
    assert fo2._step == 7 and fo2._lag == {'vis2_ctx.weight': 2}
    assert torch.equal(fo2._m, fo._m) and torch.equal(fo2._v, fo._v)


def test_a_stock_adamw_state_switches_the_table_route_on():
    """the silent error this closes: a checkpoint of a stock AdamW run loaded into a default-constructed FusedAdam continued with
    coupled decay; now the flag arrives, the table route is on -- and an optimiser that refused that route refuses the state"""
    model, _, fo = _model()
    assert not fo.device_hyper
    ref = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in model.parameters()], lr=2e-4, weight_decay=1e-2)
    for q in ref.param_groups[0]['params']:
        q.grad = torch.ones_like(q)
    ref.step()
    fo.load_state_dict(ref.state_dict())
    assert fo.device_hyper and fo.hyper_rows() == ((2e-4, 0.9, 0.999, 1e-8, 1e-2, True),) and fo._step == 1
    assert fo.trainable_ranges() == [(0, model.flat_params().numel(), 0, 0)]
    with pytest.raises(ValueError, match='device_hyper=False'):
        FusedAdam(model, device_hyper=False).load_state_dict(ref.state_dict())
    # a stock coupled Adam's state leaves the by-value path alone; a state from before the key existed reads as coupled
    model3, _, fo3 = _model()
    sd = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in model3.parameters()]).state_dict()
    fo3.load_state_dict(sd)
    assert not fo3.device_hyper
    for g in sd['param_groups']:
        del g['decoupled_weight_decay']
    fo3.load_state_dict(sd)
    assert not fo3.device_hyper and fo3.hyper_rows()[0][5] is False


def test_flat_checkpoints_keep_the_flag():
    # three groups (the flag travels inside 'groups')
    model, _, _ = _model()
    pg = [dict(g, decoupled_weight_decay=(i != 1)) for i, g in enumerate(GC.three_groups(model))]
    fo = FusedAdam(model, lr=3e-5, weight_decay=1e-2, param_groups=pg)
    _fill_state(model, fo)
    ck = {'epoch': 3, 'state_dict': model.state_dict(), 'optimizer': fo.state_dict(), 'param_group_names': fo.group_names()}
    flat = util.checkpoint_to_flat(ck, model)
    assert [g['decoupled_weight_decay'] for g in flat['groups']] == [True, False, True] and 'decoupled_weight_decay' not in flat
    back = util.flat_to_checkpoint(flat, model)
    assert [g['decoupled_weight_decay'] for g in back['optimizer']['param_groups']] == [True, False, True]
    fo_b = FusedAdam(_model()[0], param_groups=GC.three_groups(model))
    fo_b.load_state_dict(back['optimizer'])
    assert fo_b.hyper_rows() == fo.hyper_rows() and torch.equal(fo_b._m, fo._m) and fo_b._lag == fo._lag
    _stock(model, fo, 'AdamW')[0].load_state_dict(back['optimizer'])
    # one group: the key only when it is true
    one = FusedAdam(model, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True)
    _fill_state(model, one)
    flat1 = util.checkpoint_to_flat({'epoch': 0, 'state_dict': model.state_dict(), 'optimizer': one.state_dict()}, model)
    assert flat1['decoupled_weight_decay'] is True and 'groups' not in flat1
    back1 = util.flat_to_checkpoint(flat1, model, lr=1e-3, weight_decay=1e-2)
    assert back1['optimizer']['param_groups'][0]['decoupled_weight_decay'] is True
    again = FusedAdam(_model()[0])
    again.load_state_dict(back1['optimizer'])
    assert again.device_hyper and again.hyper_rows() == one.hyper_rows() and torch.equal(again._v, one._v) and again._step == 7
    plain = FusedAdam(model)
    flat0 = util.checkpoint_to_flat({'epoch': 0, 'state_dict': model.state_dict(), 'optimizer': plain.state_dict()}, model)
    assert 'decoupled_weight_decay' not in flat0
    assert 'decoupled_weight_decay' not in util.flat_to_checkpoint(flat0, model)['optimizer']['param_groups'][0]


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
A0 = 0x10000000
TABLE = A0 + 0x4000000 * 8


@pytest.fixture(params=['dry', 'no_dry_run'])
def lib(request):
    L = _lib.lib()
    if request.param == 'dry':
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_set_adam_hyper_map(None, None, 0) == 0
        assert L.lirec_debug_set(0, -1) == 0


def _map(L, rs, table=TABLE, count=None):
    arr = (_lib.AdamGroupRange * max(len(rs), 1))()
    for a, (o, k, lag, grp) in zip(arr, rs):
        a.offset, a.length, a.lag, a.group = o, k, lag, grp
    return L.lirec_set_adam_hyper_map(table, arr, len(rs) if count is None else count)


def test_abi_numbers_and_exports():
    L = _lib.lib()
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert L.lirec_abi_sizeof(11) == C.sizeof(_lib.AdamHyper) == 32
    assert [f[0] for f in _lib.AdamHyper._fields_] == ['lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'decoupled', 'reserved_']
    assert _lib.AdamHyper.decoupled.offset == 20 and _lib.AdamHyper.reserved_.offset == 24
    assert 'lirec_set_adam_hyper_map' in _lib.EXPORTS and hasattr(L, 'lirec_set_adam_hyper_map')
    header = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    assert 'int lirec_set_adam_hyper_map(const lirec_adam_hyper* table_dev, const lirec_adam_group_range* ranges, int32_t count);' in header
    assert 'float decoupled;' in header and 'float reserved_[2];' in header and '#define LIREC_ADAM_MAP_MAX 16' in header
    assert _lib.ADAM_MAP_MAX == 16


def test_set_adam_hyper_map_argument_checks(lib):
    L = lib
    good = [(0, 4096, 0, 0), (4096, 16, 0, 1), (4112, 100, 0, 7)]
    assert _map(L, good) == 0
    assert _map(L, [(4 * i, 4, 0, i % 8) for i in range(16)]) == 0                 # 16 entries
    assert _map(L, [(0, 5, 0, 0), (5, 3, 0, 1)]) == 0                              # (offsets need no alignment: they are looked up)
    for off in (4, 8, 12, 2):
        assert _map(L, good, table=TABLE + off) == EINVAL                          # a misaligned table
    assert _map(L, [(4 * i, 4, 0, 0) for i in range(17)]) == EINVAL                # count outside 0..16
    assert _map(L, good, count=-1) == EINVAL
    assert _map(L, [(0, 4096, 0, 0), (4095, 16, 0, 1)]) == EINVAL                  # overlapping
    assert _map(L, [(4096, 16, 0, 1), (0, 4096, 0, 0)]) == EINVAL                  # not ascending
    assert _map(L, [(-4, 16, 0, 0)]) == EINVAL and _map(L, [(0, 0, 0, 0)]) == EINVAL
    assert _map(L, [(0, 16, 0, 8)]) == EINVAL and _map(L, [(0, 16, 0, -1)]) == EINVAL          # a group outside 0..7
    assert _map(L, [(0, 16, 1, 0)]) == EINVAL                                      # a lag: the fold has the one global step
    big = 2 ** 63 - 1
    assert _map(L, [(8, big, 0, 0), (16, 4, 0, 1)]) == EINVAL and _map(L, [(8, big - 7, 0, 0)]) == EINVAL      # offset + length would wrap
    assert _map(L, [(8, big - 8, 0, 0)]) == 0
    assert L.lirec_set_adam_hyper_map(TABLE, None, 2) == EINVAL and _map(L, good, table=None) == EINVAL
    # off: count 0, or NULL
    assert _map(L, [], table=TABLE) == 0 and L.lirec_set_adam_hyper_map(None, None, 0) == 0
    # the single-row setting is independent of it
    assert L.lirec_set_adam_hyper_row(TABLE + 32) == 0 and L.lirec_set_adam_hyper_row(None) == 0


def test_a_recorded_step_follows_the_flag_and_the_learning_rate_in_the_dry_run():
    """two groups (decay / no decay) through the real Python host stack in the library's dry run, at the dimensions where the
    persistent kernels and the folded update are planned: the fold is armed with one row per parameter; the flag and lr change
    between replays -- the command list keeps its size, one table write per change (one table: no side stream here), the key is
    unchanged; under by-value recording, switching the flag on is the 'hyper-parameters changed' refusal"""
    code = ('import host_dryrun as H, torch, adamw_cases as WC\n'
            'from lirec_amd import _lib, ops, config, model as M\n'
            'from lirec_amd.config import opt\n'
            'from lirec_amd.optim import FusedAdam\n'
            'from lirec_amd.graph import RecordedTrainStep\n'
            'from lirec_amd.data import synthetic_batch\n'
            'L = _lib.lib(); assert L.lirec_debug_set(H.DRY, -1) == 0; H.patch()\n'
            'ops.set_gemm_mode(2)\n'
            'big = dict(text_dim=768, visual_dim=2048, track_dim=2048, joint_dim=512)\n'
            'config.recipe("int_rel_ch", dropout=0.3, dropout_seed=5, rels_n_clips=18, **big)\n'
            'opt.device = "cpu"; opt.wgrad_side_stream = False\n'
            'model, loss, _ = M.create_model(101, n_rels=15)\n'
            'model.train()\n'
            'hb = synthetic_batch(3, "int_rel_ch", 8, n_classes=101, n_rels=15, T=16, R=18, text_dim=768, visual_dim=2048, track_dim=2048)\n'
            'batch = {k: (v.float() if (torch.is_tensor(v) and k == "features") else v) for k, v in hb.items()}\n'
            'def run(optim):\n'
            '    for _ in range(2):\n'
            '        optim.zero_grad(); lv = loss(model(dict(batch)), batch); lv.backward(); optim.step()\n'
            '    return RecordedTrainStep(model, loss, optim, batch, warmup=1)\n'
            'optim = FusedAdam(model, lr=1e-3, param_groups=WC.two_groups(model))\n'
            'writes, maps = [], []\n'
            'w0 = ops.adam_hyper_write\n'
            'ops.adam_hyper_write = lambda t, rows: (writes.append(rows), w0(t, rows))[1]\n'
            'm0 = L.lirec_set_adam_hyper_map\n'
            'ops.lib = lambda: type("P", (), {"__getattr__": lambda s, n: (lambda *a: (maps.append(a[2]), m0(*a))[1]) if n == "lirec_set_adam_hyper_map" else getattr(L, n)})()\n'
            'g = run(optim)\n'
            'n, key = g.cmds.size, g._hyper\n'
            'assert g.fused, "the fold is not armed for weights / biases in two groups"\n'
            'assert n > 5 and len(writes) == 1 and key == (("device_hyper", optim.group_membership()), 1.0)\n'
            'assert maps and max(maps) > 1 and maps[-1] == 0, maps\n'
            'for i in range(3):\n'
            '    for grp in optim.param_groups: grp["lr"] = grp["lr"] * 0.5\n'
            '    optim.param_groups[i % 2]["decoupled_weight_decay"] = not optim.param_groups[i % 2]["decoupled_weight_decay"]\n'
            '    g.step()\n'
            '    assert g.cmds.size == n and len(writes) == 2 + i and g.hyper_key(optim) == key, (i, len(writes))\n'
            '    assert [r[5] for r in writes[-1]] == [bool(x["decoupled_weight_decay"]) for x in optim.param_groups]\n'
            'g.step(); assert len(writes) == 4\n'
            'g.release(); g.cmds.destroy()\n'
            'plain = FusedAdam(model, lr=1e-3)\n'
            'g = run(plain)\n'
            'assert g.fused and not plain.device_hyper and len(writes) == 4\n'
            'g.step()\n'
            'plain.param_groups[0]["decoupled_weight_decay"] = True\n'
            'try:\n'
            '    g.step(); raise SystemExit("switching the flag on under by-value recording did not raise")\n'
            'except RuntimeError as e:\n'
            '    assert "hyper-parameters changed" in str(e)\n'
            'g.release(); g.cmds.destroy()\n'
            'print("adamw dry run ok")\n')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'adamw dry run ok' in r.stdout, r.stdout[-4000:]
