"""Frozen parameters (``requires_grad_(False)``) without a GPU: the plan that decides which backward launches still run, against a
brute-force reachability over a dependency table written out here; the optimiser's trainable ranges against a per-element mask;
the per-parameter step bookkeeping (a lag behind the global step) against a stock ``torch.optim.Adam`` through ``state_dict`` /
``load_state_dict`` in both directions; and the argument checks of ``lirec_adam_step_ranges`` (LIREC_EINVAL before any device
call) under the library's host-side dry run."""
import ctypes as C

import numpy as np
import pytest
import torch

from lirec_amd import _lib, config
from lirec_amd.config import opt
from lirec_amd.optim import FusedAdam

DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)
DRY = 4194304                                  # lirec_debug_set: host-side dry run
A0 = 0x10000000                                # fake, aligned, never dereferenced device addresses


def _model(kind):
    from lirec_amd import model as M
    config.recipe(kind, joint_dim=16, rels_n_clips=3, dropout=0.3, dropout_seed=7, **DIMS)
    opt.device = 'cpu'
    torch.manual_seed(3)
    return M.create_model(11, n_rels=5)


# the frozen sets of the issue, as predicates on (parameter name, its group)
FROZEN_SETS = {
    'nothing': lambda n, g: False,
    'heads_only_trainable': lambda n, g: not g.startswith('out_'),
    'both_L1': lambda n, g: g.startswith('L1_'),
    'L1_c': lambda n, g: g == 'L1_c',
    'context_head': lambda n, g: g in ('L1_c', 'L2_c', 'out_ctx'),
    'gate': lambda n, g: g == 'gate',
    'all_biases': lambda n, g: n.endswith('.bias'),
    'txt_ctx_weight': lambda n, g: n == 'txt_ctx.weight',
    'embeddings': lambda n, g: g[:2] in ('L1', 'L2'),
    'everything': lambda n, g: True,
}
KINDS = ['modalties', 'int_ch', 'int_rels', 'int_rel_ch']          # Modalities, MaxTracks without context, MultiClip, MaxTracks


def _freeze(model, which):
    for n, p in model.named_parameters():
        p.requires_grad_(not FROZEN_SETS[which](n, model.param_group_of(n)))


# ---------------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------------
def _table(has_ctx, has_gate):
    """launch -> (groups whose gradients it forms, data it makes, [(made item that must be wanted or None, item it then reads)]).
    Written from the backward's data flow: loss -> heads' data gradients -> (gate) -> dEE halves -> per head second-layer weight
    gradient and the tail (hidden-layer gradient, un-pool, first-layer weight gradient, input gradient)."""
    t = {'out_ints_dW': (['out_ints'], [], []),
         'dW2_i': (['L2_i'], [], [(None, 'dEE_i')]),
         'tail_i': (['L1_i'], ['dX_i'], [(None, 'dEE_i')])}
    if has_ctx:
        t['out_ctx_dW'] = (['out_ctx'], [], [])
        t['dW2_c'] = (['L2_c'], [], [(None, 'dEE_c')])
        t['tail_c'] = (['L1_c'], ['dX_c'], [(None, 'dEE_c')])
    if has_gate:
        t['out_ints_dA'] = ([], ['dZg'], [])
        t['out_ctx_dA'] = ([], ['dEE_c_raw'], [])
        t['gate_stage'] = ([], ['dZg_rows'], [(None, 'dZg')])
        t['gate_dW'] = (['gate'], [], [(None, 'dZg_rows')])
        # one launch forms both halves; only the context half is built on the context head's raw data gradient
        t['gate_dEE'] = ([], ['dEE_i', 'dEE_c'], [(None, 'dZg_rows'), ('dEE_c', 'dEE_c_raw')])
    else:
        t['out_ints_dA'] = ([], ['dEE_i'], [])
        if has_ctx:
            t['out_ctx_dA'] = ([], ['dEE_c'], [])
    return t


def _brute(table, live, want_input):
    wanted = {'dX_i', 'dX_c'} if want_input else set()
    need = set()
    while True:
        before = (len(wanted), len(need))
        for name, (grads, makes, reads) in table.items():
            if any(live.get(g, False) for g in grads) or any(m in wanted for m in makes):
                need.add(name)
                for cond, item in reads:
                    if cond is None or cond in wanted:
                        wanted.add(item)
        if (len(wanted), len(need)) == before:
            return need


@pytest.mark.parametrize('which', sorted(FROZEN_SETS))
@pytest.mark.parametrize('kind', KINDS)
def test_plan_is_the_reachability_of_the_dependency_table(kind, which):
    model, _, _ = _model(kind)
    _freeze(model, which)
    plan = model.trainable_plan()
    table = _table(model._has_ctx, model._has_gate)
    for want_input in (False, True):
        assert set(plan.need(want_input)) == _brute(table, plan.live, want_input), (kind, which, want_input)
    assert set(plan.need()) <= set(type(plan).LAUNCHES)
    if which == 'nothing':
        assert set(plan.need()) == set(table) and plan.all_live
    if which == 'everything':
        assert not plan.need() and set(plan.need(True)) >= {'tail_i'}
    # partly frozen groups run as ever: freezing biases, or one weight, prunes nothing
    if which in ('all_biases', 'txt_ctx_weight'):
        assert set(plan.need()) == set(table)


def test_plan_is_cached_on_the_flags_and_follows_them():
    model, _, _ = _model('int_rel_ch')
    a = model.trainable_plan()
    assert model.trainable_plan() is a
    _freeze(model, 'both_L1')
    b = model.trainable_plan()
    assert b is not a and model.trainable_plan() is b
    assert not {'tail_i', 'tail_c'} & set(b.need()) and {'dW2_i', 'dW2_c', 'gate_dEE', 'gate_dW'} <= set(b.need())
    _freeze(model, 'heads_only_trainable')
    assert set(model.trainable_plan().need()) == {'out_ints_dW', 'out_ctx_dW'}
    _freeze(model, 'context_head')
    assert set(model.trainable_plan().need()) == {'out_ints_dW', 'out_ints_dA', 'gate_stage', 'gate_dW', 'gate_dEE', 'dW2_i', 'tail_i'}
    _freeze(model, 'nothing')
    assert model.trainable_plan().need() == a.need()


def test_frozen_parameters_have_no_gradient_view():
    """flat_grads(attach=True) on the CPU layout: views for trainable parameters only, an earlier view of a frozen one dropped"""
    model, _, _ = _model('int_rel_ch')
    g = model.flat_grads(attach=True)
    for n, p in model.named_parameters():
        o, k = model._offsets[n]
        assert p.grad is not None and p.grad.data_ptr() == g[o:o + k].data_ptr(), n
    _freeze(model, 'gate')
    model.flat_grads(attach=True)
    for n, p in model.named_parameters():
        assert (p.grad is None) == n.startswith('gates_'), n
    _freeze(model, 'nothing')
    g[:] = 7.0
    model.flat_grads(attach=True)
    for n, p in model.named_parameters():
        assert p.grad is not None
        assert float(p.grad.abs().max()) == (0.0 if n.startswith('gates_') else 7.0), n       # (unfrozen: starts from zero)


# ---------------------------------------------------------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------------------------------------------------------
def _check_ranges(rs, offsets, trainable, extent):
    mask = np.zeros(extent, bool)                 # True: a frozen parameter's element
    live = np.zeros(extent, bool)
    for n, (o, k) in offsets.items():
        (live if trainable[n] else mask)[o:o + k] = True
    covered = np.zeros(extent, bool)
    end = 0
    for a, b, lag in rs:
        assert 0 <= a < b <= extent and a % 4 == 0 and a >= end, (a, b)
        covered[a:b] = True
        end = b
    assert not (covered & mask).any(), 'a frozen element is updated'
    assert (covered | ~live).all(), 'a trainable element is not updated'


@pytest.mark.parametrize('kind', KINDS)
def test_trainable_ranges_against_an_element_mask(kind):
    model, _, optim = _model(kind)
    names = [n for n, _ in model.named_parameters()]
    r = np.random.default_rng(11)
    assert optim.trainable_ranges() == [(0, model.flat_params().numel(), 0)]
    for trial in range(40):
        frozen = r.random(len(names)) < r.choice([0.1, 0.5, 0.9])
        lags = {n: int(r.integers(0, 3)) for n in names if r.random() < 0.3}
        for (n, p), f in zip(model.named_parameters(), frozen):
            p.requires_grad_(not f)
        optim._lag = dict(lags)
        rs = optim.trainable_ranges()
        tr = {n: not f for n, f in zip(names, frozen)}
        _check_ranges(rs, model._offsets, tr, model.flat_params().numel())
        # every range carries the lag of the parameters in it
        for a, b, lag in rs:
            inside = [n for n, (o, k) in model._offsets.items() if tr[n] and o >= a and o + k <= b]
            assert inside and all(lags.get(n, 0) == lag for n in inside)
        # a stretch (a bucket, a rank's slice) is the intersection
        lo, hi = sorted(int(x) // 32 * 32 for x in r.integers(0, model.flat_params().numel(), 2))
        cut = optim.trainable_ranges(lo, hi)
        assert cut == [(max(a, lo), min(b, hi), lag) for a, b, lag in rs if min(b, hi) > max(a, lo)]
        assert all((a - lo) % 4 == 0 for a, _, _ in cut)
        assert all(len(c) <= _lib.ADAM_MAX_RANGES for c in FusedAdam._chunks(cut))


def test_many_ranges_are_cut_into_calls_of_64():
    offsets = {'p%d' % i: (8 * i, 5) for i in range(400)}                  # 400 parameters, 3 elements of gap after each
    tr = {n: i % 2 == 0 for i, n in enumerate(offsets)}
    rs = FusedAdam.merged_ranges(offsets, tr, {}, 3200)
    assert len(rs) == 200
    _check_ranges(rs, offsets, tr, 3200)
    ch = FusedAdam._chunks(rs)
    assert [len(c) for c in ch] == [64, 64, 64, 8] and sum(ch, []) == rs
    # neighbours merge across the gap only when both are trainable with one lag; the last one takes the buffer's tail
    tr = {n: True for n in offsets}
    assert FusedAdam.merged_ranges(offsets, tr, {}, 3232) == [(0, 3232, 0)]
    assert FusedAdam.merged_ranges(offsets, tr, {'p1': 2}, 3232) == [(0, 5, 0), (8, 13, 2), (16, 3232, 0)]
    tr['p399'] = False
    assert FusedAdam.merged_ranges(offsets, tr, {}, 3232) == [(0, 8 * 398 + 5, 0)]


# ---------------------------------------------------------------------------------------------------------------------------
# per-parameter steps
# ---------------------------------------------------------------------------------------------------------------------------
SCHEDULE = ['nothing', 'gate', 'gate', 'nothing', 'both_L1', 'heads_only_trainable', 'nothing', 'everything', 'gate']


def _steps_of(sd, n):
    return [int(float(sd['state'][i]['step'])) if i in sd['state'] else 0 for i in range(n)]


def test_per_parameter_steps_against_stock_adam_both_ways():
    model, _, fo = _model('int_rel_ch')
    params = list(model.parameters())
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.Adam(clones, lr=3e-5, weight_decay=1e-5)
    for which in SCHEDULE:
        _freeze(model, which)
        for p, c in zip(params, clones):                 # stock Adam is fed gradients on the trainable parameters only
            c.grad = torch.ones_like(c) if p.requires_grad else None
        ref.step()
        fo._step += 1                                    # the bookkeeping of FusedAdam.step() (the update itself needs the GPU)
        fo._advance_lags()
    want = _steps_of(ref.state_dict(), len(params))
    assert len(set(want)) > 2 and max(want) == len(SCHEDULE) - 1          # ('everything' is a step nobody took ... in torch)
    got = _steps_of(fo.state_dict(), len(params))
    # (the global step counts step() calls, the one nobody took part in included; a parameter's own is that minus its lag)
    assert fo._step == len(SCHEDULE) and got == want
    # torch -> here
    model2, _, fo2 = _model('int_rel_ch')
    fo2.load_state_dict(ref.state_dict())
    assert fo2._step == max(want) and _steps_of(fo2.state_dict(), len(params)) == want
    assert all(fo2._lag.get(n, 0) == max(want) - w for (n, _), w in zip(model2.named_parameters(), want))
    # here -> torch -> here
    ref2 = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=3e-5, weight_decay=1e-5)
    ref2.load_state_dict(fo2.state_dict())
    assert _steps_of(ref2.state_dict(), len(params)) == want
    model3, _, fo3 = _model('int_rel_ch')
    fo3.load_state_dict(ref2.state_dict())
    assert _steps_of(fo3.state_dict(), len(params)) == want
    # equal steps -- every checkpoint written before parameters could be frozen -- load as ever: no lag
    for st in ref2.state.values():
        st['step'] = torch.tensor(5.0)
    fo3.load_state_dict(ref2.state_dict())
    assert fo3._step == 5 and not fo3._lag and fo3.all_trainable()


def test_flat_checkpoints_keep_per_parameter_steps():
    from lirec_amd import util
    model, _, fo = _model('int_rel_ch')
    _freeze(model, 'gate')
    for _ in range(3):
        fo._step += 1
        fo._advance_lags()
    _freeze(model, 'nothing')
    fo._step += 1
    fo._advance_lags()
    ck = {'epoch': 2, 'state_dict': model.state_dict(), 'optimizer': fo.state_dict()}
    flat = util.checkpoint_to_flat(ck, model)
    assert flat['step'] == 4 and set(flat['lags']) == {n for n, _ in model.named_parameters() if n.startswith('gates_')}
    assert set(flat['lags'].values()) == {3}
    back = util.flat_to_checkpoint(flat, model)
    assert _steps_of(back['optimizer'], len(model._plist)) == _steps_of(ck['optimizer'], len(model._plist))


def test_frozen_signature_is_part_of_the_recorded_steps_key():
    from lirec_amd.graph import RecordedTrainStep
    model, _, fo = _model('int_rel_ch')
    k0 = RecordedTrainStep.hyper_key(fo)
    assert len(k0) == 5 and fo.frozen_key() == ()
    _freeze(model, 'gate')
    k1 = RecordedTrainStep.hyper_key(fo)
    assert k1 != k0 and k1[:5] == k0
    fo._step += 1
    fo._advance_lags()                                   # frozen parameters fall behind: not part of the key (they are not updated)
    assert RecordedTrainStep.hyper_key(fo) == k1
    _freeze(model, 'nothing')                            # ... but once trainable again their lag is
    k2 = RecordedTrainStep.hyper_key(fo)
    assert k2 not in (k0, k1) and 1 in k2[5][1]


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks of lirec_adam_step_ranges
# ---------------------------------------------------------------------------------------------------------------------------
HY = (3e-5, 0.9, 0.999, 1e-8, 1e-5, 1.0)


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


def _ranges(L, rs=((0, 1023, 0), (1024, 5, 2)), **kw):
    v = dict(p=_addr(0), g=_addr(1), m=_addr(2), v=_addr(3), step=3, step_dev=None, count=None, ticket=None, advance=0, n=None)
    v.update(kw)
    arr = (_lib.AdamRange * max(len(rs), 1))()
    for a, (o, k, lag) in zip(arr, rs):
        a.offset, a.length, a.lag = o, k, lag
    n = len(rs) if v['n'] is None else v['n']
    return L.lirec_adam_step_ranges(v['p'], v['g'], v['m'], v['v'], arr, n, v['step'], *HY, v['step_dev'], v['count'], v['ticket'],
                                    v['advance'], None)


def test_abi_of_the_new_call():
    L = _lib.lib()
    assert L.lirec_abi_sizeof(10) == C.sizeof(_lib.AdamRange) == 24
    assert 'lirec_adam_step_ranges' in _lib.EXPORTS and hasattr(L, 'lirec_adam_step_ranges')
    assert _lib.ADAM_MAX_RANGES == 64


BAD = {
    'count_negative': dict(n=-1),
    'count_65': dict(rs=tuple((16 * i, 8, 0) for i in range(65))),
    'negative_length': dict(rs=((0, -1, 0),)),
    'negative_length_second': dict(rs=((0, 8, 0), (16, -4, 0))),
    'offset_not_multiple_of_4': dict(rs=((0, 8, 0), (17, 4, 0))),
    'offset_2': dict(rs=((2, 8, 0),)),
    'negative_offset': dict(rs=((-4, 8, 0),)),
    'overlap': dict(rs=((0, 10, 0), (8, 4, 0))),
    'out_of_order': dict(rs=((64, 8, 0), (0, 8, 0))),
    'step_minus_lag_0': dict(rs=((0, 8, 3),)),
    'step_minus_lag_negative': dict(rs=((0, 8, 0), (8, 8, 5))),
    'negative_lag': dict(rs=((0, 8, -1),)),
    'step_0_by_value': dict(step=0),
    'p_null': dict(p=None), 'g_null': dict(g=None), 'm_null': dict(m=None), 'v_null': dict(v=None),
    'both_device_steps': dict(step_dev=_addr(6), count=_addr(4), ticket=_addr(5)),
    'count_without_ticket': dict(count=_addr(4)),
}
BAD.update({'%s_plus%d' % (k, off): {k: _addr(i) + off} for i, k in enumerate('pgmv') for off in (4, 8, 12)})


@pytest.mark.parametrize('what', sorted(BAD))
def test_adam_step_ranges_argument_checks(dry, what):
    assert _ranges(dry, **BAD[what]) == _lib.LIREC_EINVAL
    # the valid neighbours pass
    assert _ranges(dry) == 0
    assert _ranges(dry, rs=()) == 0                                          # count 0: a no-op
    assert _ranges(dry, rs=tuple((16 * i, 13, i % 3) for i in range(64)), step=3) == 0
    assert _ranges(dry, rs=((0, 8, 0), (8, 0, 0), (8, 8, 1))) == 0           # touching ranges, an empty one
    assert _ranges(dry, rs=((0, 8, 7),), step=0, step_dev=_addr(6)) == 0     # (the step is read on the device)
    assert _ranges(dry, rs=((0, 8, 7),), step=0, count=_addr(4), ticket=_addr(5), advance=1) == 0
    assert _ranges(dry, p=_addr(0) + 16, g=_addr(1) + 48, m=_addr(2) + 16, v=_addr(3) + 32) == 0
    if what.split('_plus')[0] in 'pgmv':
        assert _ranges(dry, rs=(), **BAD[what]) == _lib.LIREC_EINVAL        # (checked before the count = 0 shortcut)


def test_ranges_are_refused_without_the_dry_run_too():
    """the refusal comes before any device call: no dry run, no GPU"""
    L = _lib.lib()
    assert _ranges(L, rs=((2, 8, 0),)) == _lib.LIREC_EINVAL and _ranges(L, rs=((0, 8, 3),)) == _lib.LIREC_EINVAL
