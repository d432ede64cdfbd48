"""The model's wiring under its own switches (tests/flag_matrix_cases.py) against the float64 oracle.

Every kernel family has a test of its own; which of them a train step takes, on which stream, from which kept buffer and behind
which wait is decided by about ten flags in ``_run_forward`` / ``_run_backward``, ``StepLanes``, ``FusedAdam.step`` and
``RecordedTrainStep``.  Here every row of the matrix is run through the model at full dimensions (J = 512, 6912-d) and the
smallest row counts at which each tier engages, and for every (shape, row):

  (a) one train step in the production state (``debug_keep_state`` off): logits, loss, every gradient;
  (b) the same step with the state kept: bit for bit (a) -- and from the kept state, the profile sites and the lanes a WITNESS
      that the row's flags took effect, checked against ``effective(row)``;
  (c) the first row of every numeric class: held to ``oracle.lirec_oracle`` in DOUBLE (same Philox masks, the device's relu
      decisions of (b)) with ``compare``'s tolerances -- the project's bounds against the fp32 oracle, unchanged;
  (d) every other row of the class: bit for bit the class's first row;
  (e) four eager steps: parameters, both Adam moments and the last gradients bit for bit across the class;
  (f) S1, S5 and S4: the recorded step replayed to the same step count: bit for bit (e), with the recording's own witnesses.

A row the code refuses asserts the refusal by its message (flag_matrix_cases.REFUSALS); nothing is skipped.
"""
from types import SimpleNamespace

import pytest
import torch

import flag_matrix_cases as FM
from lirec_amd import config
from lirec_amd.config import opt
from lirec_amd.data import to_device_batch
from oracle import lirec_oracle as O
from test_gpu_bench_shape import (DeviceReluDecisions, N_CLASSES, N_RELS, PARAM_SEED, SEED, compare, device_relu_decisions,
                                  make_batch, oracle_cfg)
from test_gpu_recorded_bench_shape import _shadow_is_current

pytestmark = pytest.mark.gpu
NSTEP = 4

# per shape, what its rows share: the host batch, the parameters, each class's first row (results on the device) and its oracle
# result.  One shape at a time: a class's results are ~0.4 GB at these dimensions.
_SHARED = {'shape': None}


def _shared(shape):
    if _SHARED['shape'] != shape:
        _SHARED.clear()
        torch.cuda.empty_cache()
        recipe, B, T, R = FM.SHAPES[shape][:4]
        cfg = oracle_cfg(recipe)
        _SHARED.update(shape=shape, cfg=cfg, hb=make_batch(B, T, R, 'survey', recipe),
                       params=O.fill_params(O.param_shapes(cfg, N_CLASSES, N_RELS), PARAM_SEED), runs={}, oracle={})
    return _SHARED


def _representative(shape, cls):
    """the first row of the shape's list in numeric class ``cls`` that is not refused"""
    return next(rid for rid in FM.SHAPES[shape][4] if FM.refusal(FM.row(rid)) is None and FM.numeric_class(FM.row(rid)) == cls)


def _fresh(shape, r):
    """model, loss, optimiser under row ``r``'s flags (left in force: the step reads them as it runs)"""
    from lirec_amd import model as M
    recipe, B, T, R = FM.SHAPES[shape][:4]
    config.recipe(recipe, dropout_seed=SEED, **({} if recipe == 'int_ch' else {'rels_n_clips': R}))
    opt.device = 'cuda'
    assert float(opt.dropout) == 0.3
    for f in FM.FLAGS:
        setattr(opt, f, r[f])
    model, loss, optim = M.create_model(N_CLASSES, n_rels=N_RELS)
    model.load_state_dict(_shared(shape)['params'], strict=True)
    model.train()
    return model, loss, optim


def _step(model, loss, optim, batch, update=True):
    """one eager step; returns (logits before the loss masks them in place, loss, flat gradient buffer) of it"""
    optim.zero_grad()
    out = model(dict(batch))
    pre = {k: v.detach().clone() for k, v in out.items() if v is not None}
    lv = loss(out, batch)
    lv.backward()
    torch.cuda.synchronize()
    res = (pre, lv.detach().clone().reshape(-1), model.flat_grads(attach=False).detach().clone())
    if update:
        optim.step()
    return res


def _differ(a, b, model=None):
    """{name: (elements that differ, of how many, largest difference)} between two {name: tensor} -- empty when bit-identical;
    a flat buffer is reported per parameter"""
    out = {}
    for k in a:
        x, y = a[k], b[k]
        if x.shape != y.shape:
            out[k] = ('shape', tuple(x.shape), tuple(y.shape))
        elif not torch.equal(x, y):
            if model is not None and x.dim() == 1 and x.numel() == model._n_flat:
                for n, (off, cnt) in model._offsets.items():
                    d = x[off:off + cnt] != y[off:off + cnt]
                    if bool(d.any()):
                        out['%s[%s]' % (k, n)] = (int(d.sum()), cnt, float((x[off:off + cnt] - y[off:off + cnt]).abs().max()))
            else:
                out[k] = (int((x != y).sum()), x.numel(), float((x.double() - y.double()).abs().max()))
    return out


def _step_dict(s):
    pre, lv, g = s
    return dict({'logits ' + k: v for k, v in pre.items()}, loss=lv, grads=g)


def _witnesses(shape, e, model, sites):
    """what run (b) left behind against what the row's flags, as they take effect, ask for"""
    recipe, B, T, R = FM.SHAPES[shape][:4]
    n = B * T
    has_c = has_g = recipe != 'int_ch'
    st = model.last_state
    # (more than 64 context clips per candidate: the library's q32b path declines both heads, and the model asks for none)
    planes = bool(e['layer1_planes'] and not (has_c and R > 64))
    took = 'stage' in sites and 'embed_dW1_reduce' in sites
    assert bool(model.last_layer1_planes) == planes == took, ('layer-1 kernels', model.last_layer1_planes, sorted(sites))
    if has_c:
        assert (st['cmp'] is not None) == e['compact_ctx_rows'], 'row compaction'
        assert (st['hbits_c'] is not None) == (e['h1_sign_bits'] and R <= 64), 'sign bits of the context head\'s H1'
        assert st['H1_c'] is not None, 'H1_c kept for the relu decisions'
    else:
        assert st.get('cmp') is None and st.get('hbits_c') is None and 'H1_c' not in st
    if has_g:
        staged_gate = bool(e['gate_q32'] and n % 32 == 0)
        assert (st['gate_ws'] is not None) == staged_gate, 'the gate\'s workspace'
        assert st['w_side_staged'] == bool(staged_gate and e['gate_stage_on_side']), 'the gate\'s weights staged on lane 0'
    else:
        assert 'gate_ws' not in st
    assert (0 in model.lanes.sides) == (1 in model.lanes.sides) == e['wgrad_side_stream'], ('side lanes', sorted(model.lanes.sides))
    return has_g, planes


def _run(shape, rid):
    """(a), (b), (e) and (f) of one row; the comparisons inside a row are asserted here"""
    from lirec_amd import _lib, ops
    from lirec_amd.graph import RecordedTrainStep
    sh = _shared(shape)
    if rid in sh['runs']:
        return sh['runs'][rid]
    r = FM.row(rid)
    e = FM.effective(r)
    recorded = FM.SHAPES[shape][5]
    ops.set_gemm_mode(_lib.default_gemm_mode())
    g = None
    try:
        # ---- (a) + (e): production state, four eager steps
        model, loss, optim = _fresh(shape, r)
        batch = to_device_batch(sh['hb'], 'cuda', feature_dtype='q32' if r[FM.STORAGE] == 'q32' else torch.float32)
        first = _step(model, loss, optim, batch)
        assert model.last_state is None
        for _ in range(NSTEP - 1):
            last = _step(model, loss, optim, batch)
        torch.cuda.synchronize()
        final = {'params': model.flat_params().detach().clone(), 'exp_avg': optim._m.detach().clone(),
                 'exp_avg_sq': optim._v.detach().clone(), 'grads': last[2]}
        offsets, shapes = dict(model._offsets), {k: tuple(p.shape) for k, p in model.named_parameters()}
        layout = SimpleNamespace(_offsets=offsets, _n_flat=model._n_flat)       # (what _differ reads of a model)
        assert model._fwd_train_calls == NSTEP == optim._step
        # ---- (b): the same first step with the state kept; witnesses
        m2, l2, o2 = _fresh(shape, r)
        m2.debug_keep_state = True
        ops.profile_enable(True)
        try:
            kept = _step(m2, l2, o2, batch, update=False)
            sites = ops.profile_read()
        finally:
            ops.profile_enable(False)
        d = _differ(_step_dict(first), _step_dict(kept), m2)
        assert not d, ('keeping the forward state changed the step', d)
        has_g, planes = _witnesses(shape, e, m2, sites)
        o2.step()
        assert m2.lanes.bucket0_on_side == bool(e['adam_on_side_stream'] and has_g), 'who updated the first gradient bucket'
        torch.cuda.synchronize()
        masks = device_relu_decisions(m2, SEED, sh['cfg'].dropout)
        m2.last_state = None
        del m2, l2, o2
        # ---- (f): the recorded step, replayed to the same step count
        if recorded:
            m3, l3, o3 = _fresh(shape, r)
            g = RecordedTrainStep(m3, l3, o3, batch, warmup=2)
            fused = bool(e['fuse_dw1_adam'] and planes)
            assert g.overwrite, 'single GPU, no accumulation: the recorded step overwrites its gradients'
            assert g.defer == e['defer_side_join'] and m3.lanes.defer_join == g.defer, 'deferred side join'
            assert g.fused == fused and bool(m3._w1q_valid) == fused, ('folded first-layer update', g.fused, m3._w1q_valid)
            while m3._fwd_train_calls < NSTEP:
                g.step()
            g.flush()
            torch.cuda.synchronize()
            assert m3._fwd_train_calls == NSTEP == o3._step
            rec = {'params': m3.flat_params().detach().clone(), 'exp_avg': o3._m.detach().clone(),
                   'exp_avg_sq': o3._v.detach().clone(), 'grads': m3.flat_grads(attach=False).detach().clone()}
            d = _differ(final, rec, m3)
            assert not d, ('the recorded step left other bits than the eager loop', d)
            if fused:
                _shadow_is_current(m3)
            g.release()
            g = None
            assert not m3._w1q_valid
    finally:
        if g is not None:
            g.release()
        config.reset()
        ops.set_gemm_mode(_lib.default_gemm_mode())
    res = {'first': first, 'final': final, 'masks': masks, 'offsets': offsets, 'shapes': shapes, 'layout': layout}
    if rid == _representative(shape, FM.numeric_class(r)):
        sh['runs'][rid] = res
    return res


def _oracle(shape, cls, masks):
    """forward, loss and backward of the oracle in double: parameters as float64, the features as the float64 values of what
    the device reads (the reference's `.float()`, mlp/model.py:279), the step's own Philox masks, the device's relu decisions"""
    sh = _shared(shape)
    if cls not in sh['oracle']:
        cfg, hb = sh['cfg'], dict(sh['hb'])
        hb['features'] = hb['features'].float().double()
        P = {k: v.detach().double().requires_grad_(True) for k, v in sh['params'].items()}
        relu = DeviceReluDecisions(masks)
        oo = O.model_forward(P, cfg, hb, O.PhiloxDropout(SEED, cfg.dropout), relu)
        pre = {k: v.detach().clone() for k, v in oo.items() if v is not None}
        lv = O.loss_forward(cfg, oo, hb, N_RELS)
        lv.sum().backward()
        assert lv.dtype == torch.float64 and all(v.grad.dtype == torch.float64 for v in P.values())
        sh['oracle'][cls] = (pre, lv.detach().reshape(-1).clone(), {k: v.grad.detach().clone() for k, v in P.items()})
        print('%s class %s: relu decisions taken from the device (site: differing, max |x|, elements): %s' % (shape, cls, relu.flips))
    return sh['oracle'][cls]


@pytest.mark.parametrize('shape,rid', FM.CASES, ids=['%s-%s' % c for c in FM.CASES])
def test_flag_row(shape, rid):
    from lirec_amd._lib import LirecError
    r = FM.row(rid)
    if FM.refusal(r) is not None:
        # the row cannot be built: the model says so, in these words, before anything runs
        assert rid in FM.REFUSALS
        try:
            model, loss, optim = _fresh(shape, r)
            batch = to_device_batch(_shared(shape)['hb'], 'cuda', feature_dtype='q32')
            with pytest.raises(LirecError) as err:
                model(dict(batch))
            assert str(err.value) == FM.REFUSALS[rid]
        finally:
            config.reset()
        return
    assert rid not in FM.REFUSALS
    cls = FM.numeric_class(r)
    rep_id = _representative(shape, cls)
    res = _run(shape, rid)
    if rid == rep_id:
        # (c) the class's first row against the oracle in double
        pre, lv, g = res['first']
        hip = ({k: v.cpu() for k, v in pre.items()}, lv.cpu(),
               {n: g[off:off + k].view(res['shapes'][n]).cpu() for n, (off, k) in res['offsets'].items()})
        ref = _oracle(shape, cls, res['masks'])
        assert set(hip[0]) == set(ref[0])
        compare(hip, ref, '%s class %s' % (shape, ''.join('01'[int(c)] for c in cls)))
    else:
        # (d), (e) bit identity inside the class
        rep = _run(shape, rep_id)
        d = _differ(_step_dict(rep['first']), _step_dict(res['first']), res['layout'])
        assert not d, ('first step differs from row %s of the same numeric class' % rep_id, d)
        d = _differ(rep['final'], res['final'], res['layout'])
        assert not d, ('after %d steps: differs from row %s of the same numeric class' % (NSTEP, rep_id), d)


def test_q32_storage_with_more_than_64_context_clips_is_refused_in_words():
    """S4 again: the q32b layer-1 kernels decline R = 65 and nothing else reads q32b storage -- the model says so itself (the
    library's answer was a bare 'invalid argument' from lirec_embed_fwd2)."""
    from lirec_amd._lib import LirecError
    try:
        model, loss, optim = _fresh('S4', FM.row('feature_storage'))
        batch = to_device_batch(_shared('S4')['hb'], 'cuda', feature_dtype='q32')
        with pytest.raises(LirecError, match='at most 64 context clips per candidate .this batch: 65.'):
            model(dict(batch))
    finally:
        config.reset()
