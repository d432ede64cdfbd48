"""Frozen parameters on the GPU, through the model: ``p.requires_grad_(False)`` on any set of parameters.

After three eager steps with a frozen set: (a) every frozen parameter has its initial bits, its moments are untouched, its
``.grad`` is None; (b) the trainable gradients match the oracle's autograd gradients at the tolerances of the parity tests
(golden_util.grad_close); (c) the flat parameters and moments after each step are adam_cases.ref32 applied to the device's own
gradients with each parameter's OWN step, bit for bit, everything else unchanged; (d) the launches the plan drops were not issued
(the library's per-site profile); (e) with everything frozen ``loss.backward()`` raises nothing and issues nothing.  Then:
unfreezing (per-parameter steps, against a stock torch.optim.Adam fed the same gradients), the persistent layer-1 path at full
feature dimensions (a one-head dW1 launch, the fused update not armed, the shadow of W1 kept when nothing writes W1), the recorded
step against the eager loop bit for bit, and two data-parallel ranks.

Small shapes: the dims of tests/test_gpu_nonfinite.py (text 24, visual 32, track 32, joint_dim 16; B = 4, T = 6, R = 3), dropout on.
"""
import os
import socket

import numpy as np
import pytest
import torch

import adam_cases as AC
from golden_util import grad_close
from lirec_amd import config, ops
from lirec_amd.config import opt
from lirec_amd.data import synthetic_batch, to_device_batch
from oracle import lirec_oracle as O

pytestmark = pytest.mark.gpu
DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)
SEED = 7

FROZEN_SETS = {
    'nothing': lambda n, g: False,
    'heads_only_trainable': lambda n, g: not g.startswith('out_'),
    'both_L1': lambda n, g: g.startswith('L1_'),
    'L1_c': lambda n, g: g == 'L1_c',
    'context_head': lambda n, g: g in ('L1_c', 'L2_c', 'out_ctx'),
    'gate': lambda n, g: g == 'gate',
    'all_biases': lambda n, g: n.endswith('.bias'),
    'txt_ctx_weight': lambda n, g: n == 'txt_ctx.weight',
    'everything': lambda n, g: True,
}
BACKWARD_SITES = {'linear_dW', 'linear_dA', 'gate_stage', 'gate_dW', 'gate_dEE', 'embed_dW2', 'embed_dZ1', 'embed_dW1',
                  'embed_dW1_reduce', 'pool_bwd'}
# (d): the sites that must not appear (where the all-trainable step of the recipe has them)
DROPPED = {
    'both_L1': {'embed_dW1', 'embed_dW1_reduce', 'pool_bwd', 'embed_dZ1'},
    'heads_only_trainable': {'gate_stage', 'gate_dW', 'gate_dEE', 'embed_dW2', 'embed_dZ1', 'embed_dW1', 'embed_dW1_reduce',
                             'pool_bwd', 'linear_dA'},
    'everything': BACKWARD_SITES | {'adam'},
}


def _site_names():
    from lirec_amd import _lib
    L = _lib.lib()
    return {L.lirec_profile_site_name(s).decode() for s in range(L.lirec_profile_sites())}


def _freeze(model, which):
    for n, p in model.named_parameters():
        p.requires_grad_(not FROZEN_SETS[which](n, model.param_group_of(n)))


def _small(kind):
    from lirec_amd import model as M
    config.recipe(kind, joint_dim=16, rels_n_clips=3, dropout=0.3, dropout_seed=SEED, **DIMS)
    opt.device = 'cuda'
    torch.manual_seed(3)
    model, loss, optim = M.create_model(11, n_rels=5)
    model.train()
    kw = dict(n_classes=11, n_rels=5, **DIMS)
    if kind in ('int_rel_ch', 'int_rels'):
        kw['R'] = 3
    if kind in ('int_rel_ch', 'int_ch'):
        kw['T'] = 6
    if kind == 'modalties':
        kw['soft_gt'] = True
    hb = synthetic_batch(5, kind, 4, **kw)
    return model, loss, optim, hb


def _hyper(optim):
    g = optim.param_groups[0]
    return AC.hyper32((g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], optim.grad_scale))


def _np(t):
    return t.detach().cpu().numpy().copy()


def _expect_update(model, before, grads, steps, live, hyper):
    """ref32 on every trainable parameter with its own step; every other element of the flat buffers as it was"""
    want = [a.copy() for a in before]
    for n, (o, k) in model._offsets.items():
        if live[n]:
            got = AC.ref32(before[0][o:o + k], grads[o:o + k], before[1][o:o + k], before[2][o:o + k], steps[n], hyper)
            for w, x in zip(want, got):
                w[o:o + k] = x
    return want


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _eager_steps(model, loss, optim, batch, nsteps, steps=None, each=None):
    """`nsteps` eager steps; after each one check (c) and call each(i, grads, before, after).  `steps`: updates received so far per
    parameter (updated here)."""
    hyper = _hyper(optim)
    names = [n for n, _ in model.named_parameters()]
    steps = {n: 0 for n in names} if steps is None else steps
    optim._ensure_state()
    for i in range(nsteps):
        live = {n: p.requires_grad for n, p in model.named_parameters()}
        optim.zero_grad()
        lv = loss(model(dict(batch)), batch)
        lv.backward()
        torch.cuda.synchronize()
        grads = _np(model.flat_grads(attach=False))
        before = [_np(model.flat_params()), _np(optim._m), _np(optim._v)]
        optim.step()
        torch.cuda.synchronize()
        after = [_np(model.flat_params()), _np(optim._m), _np(optim._v)]
        for n in names:
            if live[n]:
                steps[n] += 1
        want = _expect_update(model, before, grads, steps, live, hyper)
        for w, a, what in zip(want, after, ('parameters', 'exp_avg', 'exp_avg_sq')):
            bad = [n for n, (o, k) in model._offsets.items() if not _bits_equal(w[o:o + k], a[o:o + k])]
            assert not bad, ('step %d: %s differ from ref32 with per-parameter steps (or a frozen one moved)' % (i + 1, what), bad)
            assert _bits_equal(w, a), 'step %d: %s: an element outside every parameter changed' % (i + 1, what)
        if each is not None:
            each(i, grads, before, after, live)
    return steps


_FULL_SITES = {}


def _sites_of_all_trainable(kind):
    if kind not in _FULL_SITES:
        model, loss, optim, hb = _small(kind)
        batch = to_device_batch(hb, 'cuda')
        ops.profile_enable(True)
        try:
            _eager_steps(model, loss, optim, batch, 1)
            _FULL_SITES[kind] = set(ops.profile_read())
        finally:
            ops.profile_enable(False)
    return _FULL_SITES[kind]


CASES = [('int_rel_ch', w) for w in sorted(FROZEN_SETS) if w != 'nothing'] + \
        [('int_rels', w) for w in ('heads_only_trainable', 'both_L1', 'gate', 'everything')] + \
        [('int_ch', w) for w in ('heads_only_trainable', 'both_L1', 'all_biases')] + \
        [('modalties', w) for w in ('heads_only_trainable', 'both_L1', 'everything')]


@pytest.mark.parametrize('kind,which', CASES, ids=['%s-%s' % c for c in CASES])
def test_three_eager_steps_with_a_frozen_set(kind, which):
    full = _sites_of_all_trainable(kind)
    assert BACKWARD_SITES & full and 'adam' in full and full <= _site_names()
    model, loss, optim, hb = _small(kind)
    batch = to_device_batch(hb, 'cuda')
    P0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    flat0 = _np(model.flat_params())
    _freeze(model, which)
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    live = [n for n, p in model.named_parameters() if p.requires_grad]
    assert frozen, 'the set freezes something in every recipe it is run on'
    # moments of the frozen parameters: a canary (their state is "untouched", not merely "still zero")
    optim._ensure_state()
    for n in frozen:
        o, k = model._offsets[n]
        optim._m[o:o + k] = 0.5
        optim._v[o:o + k] = 0.25

    def first_step_against_the_oracle(i, grads, before, after, live_now):
        if i != 0 or kind not in ('int_rel_ch', 'int_rels') or not live:
            return
        # (b) the oracle's autograd on the same parameters, batch and dropout masks
        cfg = O.OracleCfg(joint_dim=16, tr_maximize=(kind == 'int_rel_ch'), **DIMS)
        Pg = {k: v.clone().requires_grad_(k in live) for k, v in P0.items()}
        ob = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in hb.items()}
        ol = O.loss_forward(cfg, O.model_forward(Pg, cfg, ob, O.PhiloxDropout(SEED, 0.3)), ob, 5)
        ol.sum().backward()
        for n in live:
            o, k = model._offsets[n]
            grad_close(torch.from_numpy(grads[o:o + k]).view(Pg[n].shape), Pg[n].grad, 'grad %s (%s frozen)' % (n, which))
        assert all(Pg[n].grad is None for n in frozen)

    ops.profile_enable(True)
    try:
        steps = _eager_steps(model, loss, optim, batch, 3, each=first_step_against_the_oracle)     # (c) inside, (e): nothing raised
        torch.cuda.synchronize()
        sites = set(ops.profile_read())
    finally:
        ops.profile_enable(False)
    # (a)
    for n, p in model.named_parameters():
        o, k = model._offsets[n]
        if n in frozen:
            assert p.grad is None, n
            assert _bits_equal(_np(p).reshape(-1), flat0[o:o + k]), ('a frozen parameter moved', n)
            assert bool((optim._m[o:o + k] == 0.5).all()) and bool((optim._v[o:o + k] == 0.25).all()), ('moments of a frozen parameter', n)
            assert steps[n] == 0
        else:
            assert p.grad is not None and p.grad.data_ptr() == model.flat_grads(attach=False)[o:o + k].data_ptr(), n
            assert steps[n] == 3 and not _bits_equal(_np(p).reshape(-1), flat0[o:o + k]), n
    sd = optim.state_dict()
    assert [int(float(sd['state'][i]['step'])) for i in range(len(model._plist))] == [steps[n] for n, _ in model.named_parameters()]
    # (d)
    print('FROZEN-SITES %s %s: %s (all trainable: %s)' % (kind, which, sorted(sites), sorted(full)))
    assert sites <= full, ('a frozen set issues a subset of the all-trainable launches', sorted(sites - full))
    dropped = DROPPED.get(which, set()) & full
    assert not (dropped & sites), ('launches the plan drops were issued', sorted(dropped & sites))
    if which in DROPPED:
        assert dropped, 'the all-trainable step has the launches whose absence is checked'
    if which == 'everything':
        assert not (sites & (BACKWARD_SITES | {'adam'}))
    if which in ('all_biases', 'txt_ctx_weight'):
        assert sites == full                                   # a partly frozen group runs as ever


def test_backward_through_autograd_with_everything_frozen_and_with_wanted_inputs():
    """loss.sum().backward() -- the autograd engine's route -- with everything frozen: nothing raised, no library launch in backward;
    features that require grad still get their gradient, the same bits as with the parameters trainable"""
    model, loss, optim, hb = _small('int_rel_ch')
    opt.dropout = 0.0                                          # (two forwards, one input gradient)
    batch = to_device_batch(hb, 'cuda')
    x = batch['features'].detach().clone().float().requires_grad_(True)
    lv = loss(model(dict(batch, features=x)), batch)
    lv.sum().backward()
    want = x.grad.detach().clone()
    assert bool(want.abs().max() > 0)
    _freeze(model, 'everything')
    x.grad = None
    lv = loss(model(dict(batch, features=x)), batch)
    lv.sum().backward()
    assert torch.equal(x.grad, want) and all(p.grad is None for p in model.parameters())
    lv = loss(model(dict(batch)), batch)
    torch.cuda.synchronize()
    ops.profile_enable(True)
    try:
        lv.sum().backward()
        torch.cuda.synchronize()
        assert not set(ops.profile_read())
    finally:
        ops.profile_enable(False)


# ---------------------------------------------------------------------------------------------------------------------------
# unfreezing
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_gate_unfrozen_after_two_steps_starts_its_own_step_count():
    model, loss, optim, hb = _small('int_rel_ch')
    batch = to_device_batch(hb, 'cuda')
    hyper = _hyper(optim)
    names = [n for n, _ in model.named_parameters()]
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    use = [0.0, 0.0, 0.0]

    def against_stock_adam(i, grads, before, after, live):
        # a stock torch.optim.Adam on the host, given THIS step's state (values, moments, per-parameter steps) and the device's
        # gradients on the trainable parameters only: one step of it against the device's, within the bounds of the update
        ps = [torch.nn.Parameter(torch.from_numpy(before[0][o:o + k].copy()).view(shapes[n])) for n, (o, k) in
              ((n, model._offsets[n]) for n in names)]
        ref = torch.optim.Adam(ps, lr=hyper[0], betas=(hyper[1], hyper[2]), eps=hyper[3], weight_decay=hyper[4])
        sd = ref.state_dict()
        sd['state'] = {j: {'step': torch.tensor(float(counts[n])),
                           'exp_avg': torch.from_numpy(before[1][o:o + k].copy()).view(shapes[n]),
                           'exp_avg_sq': torch.from_numpy(before[2][o:o + k].copy()).view(shapes[n])}
                       for j, (n, (o, k)) in enumerate((n, model._offsets[n]) for n in names)}
        ref.load_state_dict(sd)
        for p, n in zip(ps, names):
            o, k = model._offsets[n]
            p.grad = torch.from_numpy(grads[o:o + k].copy()).view(shapes[n]) if live[n] else None
        ref.step()
        for j, (p, n) in enumerate(zip(ps, names)):
            o, k = model._offsets[n]
            if not live[n]:
                assert _bits_equal(_np(p).reshape(-1), after[0][o:o + k]), n          # torch leaves it alone, and so did the device
                continue
            counts[n] += 1
            assert int(float(ref.state[p]['step'])) == counts[n]
            sl = [a[o:o + k] for a in before]
            _, _, _, G, A, V = AC.ref64(sl[0], grads[o:o + k], sl[1], sl[2], counts[n], hyper)
            bp, bm, bv = AC.bounds(sl[0], sl[1], G, A, V)
            for x, (got, t, b) in enumerate(zip(after, (p, ref.state[p]['exp_avg'], ref.state[p]['exp_avg_sq']), (bp, bm, bv))):
                err = np.abs(got[o:o + k].astype(np.float64) - _np(t).reshape(-1).astype(np.float64))
                use[x] = max(use[x], float((err / b).max()))
                assert (err <= b).all(), ('step %d: %s against stock Adam' % (i + 1, n), 'pmv'[x], float((err / b).max()))

    counts = {n: 0 for n in names}
    _freeze(model, 'gate')
    steps = _eager_steps(model, loss, optim, batch, 2, each=against_stock_adam)
    _freeze(model, 'nothing')
    steps = _eager_steps(model, loss, optim, batch, 2, steps=steps, each=against_stock_adam)        # ref32 with each one's own step: inside
    print('FROZEN-FIGURE unfreeze: worst |device - stock Adam| / bound p=%.3f m=%.3f v=%.3f' % tuple(use))
    assert steps == counts
    sd = optim.state_dict()
    for j, n in enumerate(names):
        assert int(float(sd['state'][j]['step'])) == (2 if n.startswith('gates_') else 4), n
    assert optim._step == 4 and set(optim._lag) == {n for n in names if n.startswith('gates_')} and set(optim._lag.values()) == {2}
    # the gate's two updates were steps 1 and 2 of its own: one launch over ranges with a lag, not the whole-buffer call
    assert (0, model.flat_params().numel(), 0) not in optim.trainable_ranges() and len(optim.trainable_ranges()) >= 2


# ---------------------------------------------------------------------------------------------------------------------------
# the persistent layer-1 path: full feature dimensions, q32b storage (the smallest shape tests/test_gpu_planes.py runs it at)
# ---------------------------------------------------------------------------------------------------------------------------
PB, PT, PR = 4, 8, 18


def _persistent(which):
    from lirec_amd import model as M
    config.recipe('int_rel_ch', rels_n_clips=PR, dropout_seed=77)
    opt.device = 'cuda'
    opt.layer1_planes = True
    model, loss, optim = M.create_model(101, n_rels=15)
    model.load_state_dict(O.fill_params(O.param_shapes(O.OracleCfg(), 101, 15), 5), strict=True)
    model.train()
    _freeze(model, which)
    hb = synthetic_batch(11, 'int_rel_ch', PB, T=PT, R=PR)
    return model, loss, optim, to_device_batch(hb, 'cuda', feature_dtype='q32')


def _eager(model, loss, optim, batch):
    optim.zero_grad()
    out = model(dict(batch))
    lv = loss(out, batch)
    lv.backward()
    optim.step()
    return out


def test_persistent_path_with_the_context_first_layer_frozen_is_a_one_head_launch():
    """L1_c frozen: the interaction head's tail alone (single-head lirec_embed_bwd: a persistent dW1 launch with that head's
    problems only), no un-pool pass, the fused update not armed; the interaction head's first-layer gradients are the bits of the
    all-trainable run's where the launch is the same per-problem arithmetic -- compared at the parity tests' tolerance"""
    ref_m, ref_l, ref_o, ref_b = _persistent('nothing')
    ref_o.zero_grad()
    ref_l(ref_m(dict(ref_b)), ref_b).backward()
    torch.cuda.synchronize()
    g_ref = {n: p.grad.detach().clone() for n, p in ref_m.named_parameters()}
    model, loss, optim, batch = _persistent('L1_c')
    assert optim.arm_first_layer_update() is False and model.lanes.fold is None
    flat0 = model.flat_params().detach().clone()
    ops.profile_enable(True)
    try:
        _eager(model, loss, optim, batch)
        torch.cuda.synchronize()
        sites = ops.profile_read()
    finally:
        ops.profile_enable(False)
    assert model.last_layer1_planes and 'embed_dW1' in sites and 'embed_dW1_reduce' in sites and 'pool_bwd' not in sites, sorted(sites)
    assert sites['embed_dW1']['launches'] == 1 and not model.lanes.fold_applied
    for n, p in model.named_parameters():
        o, k = model._offsets[n]
        if model.param_group_of(n) == 'L1_c':
            assert p.grad is None and torch.equal(model.flat_params()[o:o + k], flat0[o:o + k]), n
        else:
            grad_close(p.grad, g_ref[n], 'grad ' + n)
            assert not torch.equal(model.flat_params()[o:o + k], flat0[o:o + k]), n


def test_persistent_path_with_both_first_layers_frozen_keeps_the_shadow_of_w1():
    """nothing writes W1: step() leaves the q32b shadow valid and the next forward reads it -- the logits of step 3 equal those of
    a run that stages the weights afresh each step (the shadow invalidated)"""
    outs = []
    for keep in (True, False):
        model, loss, optim, batch = _persistent('both_L1')
        assert model.refresh_w1q()
        for i in range(3):
            if not keep:
                model.invalidate_w1q()
            out = _eager(model, loss, optim, batch)
            assert bool(getattr(model, '_w1q_valid', False)) == keep, (keep, i)
        torch.cuda.synchronize()
        outs.append({k: v.detach().clone() for k, v in out.items() if v is not None})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    # with a trainable first layer the same step does invalidate it
    model, loss, optim, batch = _persistent('L1_c')
    assert model.refresh_w1q()
    _eager(model, loss, optim, batch)
    assert not model._w1q_valid


@pytest.mark.parametrize('which', ['L1_c', 'both_L1', 'heads_only_trainable'])
def test_recorded_step_with_a_frozen_set_equals_the_eager_loop_bitwise(which):
    from lirec_amd.graph import RecordedTrainStep
    NSTEP = 6                                                   # 2 warm-up steps, the recording, 3 replays
    m1, l1, o1, b1 = _persistent(which)
    for _ in range(NSTEP):
        _eager(m1, l1, o1, b1)
    torch.cuda.synchronize()
    m2, l2, o2, b2 = _persistent(which)
    g = RecordedTrainStep(m2, l2, o2, b2, warmup=2)
    try:
        for _ in range(3):
            g.step()
        g.flush()
        torch.cuda.synchronize()
        assert o2._step == NSTEP == o1._step and o1._lag == o2._lag and set(o2._lag.values()) == {NSTEP}
        assert torch.equal(m2.flat_params(), m1.flat_params()), 'parameters differ'
        o1._ensure_state(); o2._ensure_state()
        assert torch.equal(o2._m, o1._m) and torch.equal(o2._v, o1._v), 'moments differ'
        ga, gb = m1.flat_grads(attach=False), m2.flat_grads(attach=False)
        for n, p in m2.named_parameters():
            o, k = m2._offsets[n]
            if p.requires_grad:
                assert torch.equal(ga[o:o + k], gb[o:o + k]), ('gradients differ', n)
        # a requires_grad_ flip after recording: the recorded launches are another set's
        flip = next(p for p in m2.parameters() if not p.requires_grad)
        flip.requires_grad_(True)
        with pytest.raises(RuntimeError):
            g.step()
        flip.requires_grad_(False)
        g.step()
    finally:
        g.release()


# ---------------------------------------------------------------------------------------------------------------------------
# two data-parallel ranks sharing the GPU (gloo, as tests/test_gpu_parallel.py)
# ---------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_make(seed=11):
    from lirec_amd import model as M
    config.recipe('int_rel_ch', joint_dim=16, rels_n_clips=3, dropout=0.0, dropout_seed=77, **DIMS)
    opt.device = 'cuda'
    torch.manual_seed(seed)
    model, loss, optim = M.create_model(11, n_rels=5)
    optim.param_groups[0]['lr'] = 1e-3
    model.train()
    _freeze(model, 'both_L1')
    return model, loss, optim


def _dp_batch(lo, hi):
    b = synthetic_batch(21, 'int_rel_ch', 8, T=6, R=3, n_classes=11, n_rels=5, **DIMS)
    return to_device_batch({k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in b.items()}, 'cuda')


def _dp_steps(model, loss, optim, batch, n=2):
    for _ in range(n):
        optim.zero_grad()
        loss(model(dict(batch)), batch).backward()
        optim.step()
    torch.cuda.synchronize()
    return model.flat_params().detach().cpu().numpy().copy()


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from lirec_amd.parallel import DataParallel
        per = 8 // world
        model, loss, optim = _dp_make(seed=11)
        DataParallel(model, optim, sharded=True)
        # the check opt.strict makes in step(): the same frozen set on every rank passes, one that differs is refused on all
        flags = optim._flags()
        model.grad_sync.check_frozen_set(flags)
        model.grad_sync._frozen_checked = None          # (checked once per set: make both ranks check again)
        try:
            model.grad_sync.check_frozen_set(flags[:-1] + (bool(rank),))
            refused = False
        except RuntimeError:
            refused = True
        assert refused
        q.put((rank, _dp_steps(model, loss, optim, _dp_batch(rank * per, (rank + 1) * per))))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_both_first_layers_frozen():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    model, loss, optim = _dp_make(seed=11)
    p0 = model.flat_params().detach().cpu().numpy().copy()
    p_ref = _dp_steps(model, loss, optim, _dp_batch(0, 8))
    assert _bits_equal(res[0][1], res[1][1]), 'the ranks\' parameters differ'
    for n, p in model.named_parameters():
        o, k = model._offsets[n]
        if not p.requires_grad:
            assert _bits_equal(res[0][1][o:o + k], p0[o:o + k]) and _bits_equal(p_ref[o:o + k], p0[o:o + k]), ('a frozen parameter moved', n)
        else:
            assert not _bits_equal(p_ref[o:o + k], p0[o:o + k]), n
    # (tests/test_gpu_parallel.py: the drift bounded by 10 % of the two steps' maximum travel, 2 lr)
    assert float(np.abs(res[0][1] - p_ref).max()) <= 2e-4
