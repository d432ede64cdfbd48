"""Per-clip weights and per-clip loss values of the fused losses on the GPU: lirec_margin_loss_weighted in its four forms,
lirec_ce_loss_weighted and lirec_heads_loss_fwd_bwd_weighted against float64.

Yardstick: the float64 oracle composed from one-clip slices (tests/weight_cases.py; tests/test_host_clip_weights.py pins the
composition to the oracle of the whole batch at 1e-12 and asserts the caps for every case here); for the CE loss
``F.cross_entropy`` in float64 restated with per-row weights.

Bounds: those of tests/test_gpu_losses.py -- loss rtol 1e-5 / atol 1e-6, gradients rtol 1e-4 / atol 1e-7; bit-identity claims
compare with ``torch.equal``.  The gradient elements whose float64 hinge decision lies within rounding are left out exactly as
there (loss_cases.restate: they do not depend on the weights).  Weights given as float32 are the float32 values in the reference
too (the input IS float32); float64 weights enter the reference unrounded -- the kernel's conversion to float32 is 6e-8 relative.
"""
import dataclasses

import numpy as np
import pytest
import torch

import loss_cases as LC
import weight_cases as WC
from golden_util import assert_close
from lirec_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS_TOL = (1e-5, 1e-6)
GRAD_TOL = (1e-4, 1e-7)


def _ids(cases):
    return [LC.case_id(c) for c in cases]


def _dev_w(w, f64):
    return None if w is None else (w.double() if f64 else w.float()).to(DEV).contiguous()


def _ref_w(w, f64):
    """the weights as the reference takes them: the values the kernel is GIVEN (float32 input: the float32 values)"""
    return None if w is None else (w.double() if f64 else w.float().double())


def run_kernel(case, inp, w=None, f64=False, norm='sum', clip_loss=False, loader=False, sel=None, sample=0, divisors=None,
               want_probs=False):
    """One lirec_margin_loss[_weighted] call for the case (tests/test_gpu_losses.py:run_kernel with the clip-weight arguments).
    Host copies: loss (0-dim), d_ints [B,T,C], d_rels [B,T,NR] | None, sel_out [B], probs | None, the logits after the call, the
    per-clip values [B,2] | None."""
    B, T, C, NR = case.B, case.T, case.C, case.NR
    tracks = case.form in ('margin', 'mtr')
    lab = lambda t: (t.long() if loader else t.int()).to(DEV).contiguous()
    msk = lambda t: (t.double() if loader else t.float()).to(DEV).contiguous()
    ints = inp['ints'].reshape(B * T, C).to(DEV).contiguous()
    rels = inp['rels'].reshape(B * T, NR).to(DEV).contiguous() if case.rels else None
    r = inp['r'] if tracks else inp['r'][:, 0]
    cl = torch.full((B, 2), float('nan'), device=DEV) if clip_loss else None
    kw = {}
    if w is not None or cl is not None:
        kw = dict(clip_weight=_dev_w(w, f64), clip_weight_norm=norm, clip_loss=cl)
    loss, d_i, d_r, sel_out, probs = ops.margin_loss(
        ints, rels, msk(inp['mem']) if tracks and not case.mem_null else None, msk(inp['w']) if not case.w_null else None,
        lab(inp['y']), lab(r) if case.rels else None, lab(inp['gt']) if tracks else None,
        sel.int().to(DEV) if sel is not None else None, B, T, C, NR if case.rels else 0, LC.MARGIN, case.lym, case.max_neg,
        case.tr_correct, tracks, case.form == 'mtmm', loader_types=loader, sample=sample, sample_seed=LC.SAMPLE_SEED,
        want_probs=want_probs, divisors=divisors, **kw)
    torch.cuda.synchronize()
    cpu = lambda t, *s: None if t is None else t.cpu().reshape(s)
    return dict(loss=cpu(loss), d_ints=cpu(d_i, B, T, C), d_rels=cpu(d_r, B, T, NR), sel=sel_out.cpu().long(), probs=cpu(probs, B, T),
                ints=ints.cpu().view(B, T, C), clip=cpu(cl, B, 2))


def compare(case, inp, got, ref, k=None):
    """loss, gradients (without the elements whose float64 decision is within rounding), the chosen track and the masked logits
    against ``ref`` = weight_cases.weighted64(...)"""
    rs = LC.restate(case, inp, k)
    assert LC.caps_hold(case, rs, forced=k is not None), ('float64 decisions within rounding', rs['share'])
    loss, d_i, d_r, clip, xm = ref
    print('loss %.9g want %.9g' % (float(got['loss']), float(loss)))
    assert bool(torch.isfinite(got['loss']).all()) and bool(torch.isfinite(got['d_ints']).all())
    assert_close(got['loss'], loss, *LOSS_TOL, 'loss')
    keep = ~rs['ex_ints']
    assert_close(got['d_ints'][keep], d_i[keep], *GRAD_TOL, 'd_ints')
    if case.rels:
        keep = ~rs['ex_rels']
        assert bool(torch.isfinite(got['d_rels']).all())
        assert_close(got['d_rels'][keep], d_r[keep], *GRAD_TOL, 'd_rels')
    if case.form in ('margin', 'mtr'):
        assert torch.equal(got['sel'], rs['k'])
        assert torch.equal(got['ints'], xm.float().view_as(got['ints'])), 'logits after the call'
    else:
        assert torch.equal(got['ints'], inp['ints'].view_as(got['ints']))
    if got['clip'] is not None:
        assert bool(torch.isfinite(got['clip']).all()), 'a per-clip value was not written'
        assert_close(got['clip'], clip, *LOSS_TOL, 'clip_loss')


def same_bits(a, b, keys=('loss', 'd_ints', 'd_rels', 'sel', 'ints')):
    for key in keys:
        assert (a[key] is None and b[key] is None) or torch.equal(a[key], b[key]), key


# ---------------------------------------------------------------------------------------------------------------------------
# the four forms, both max_neg variants, both norms, both weight dtypes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', [False, True], ids=['w32', 'w64'])
@pytest.mark.parametrize('norm', WC.NORMS)
@pytest.mark.parametrize('case', WC.FORMS, ids=_ids(WC.FORMS))
def test_weighted_forms_against_float64(case, norm, f64):
    """weights log-uniform in [1e-3, 1e3] with two clips at exactly 0, loader-typed labels and masks; B = 300: more clips than
    the 256 threads that sum the weights; T = 65: the positive track beyond one 64-lane step"""
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    w = WC.draw_weights(case.B, case.seed)
    assert int((w == 0).sum()) == 2
    got = run_kernel(case, inp, w, f64, norm, clip_loss=True, loader=True)
    compare(case, inp, got, WC.weighted64(case, inp, _ref_w(w, f64), norm))
    zero = w == 0
    assert not got['d_ints'][zero].any() and (got['d_rels'] is None or not got['d_rels'][zero].any())


# ---------------------------------------------------------------------------------------------------------------------------
# zero denominators
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', WC.NORMS)
@pytest.mark.parametrize('case', WC.ZERO_DEN, ids=_ids(WC.ZERO_DEN))
def test_all_weights_zero_is_loss_zero_without_nan(case, norm):
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    for f64 in (False, True):
        got = run_kernel(case, inp, torch.zeros(case.B, dtype=torch.float64), f64, norm, clip_loss=True)
        assert float(got['loss']) == 0.0 and not got['d_ints'].any() and (got['d_rels'] is None or not got['d_rels'].any())
        assert bool(torch.isfinite(got['clip']).all())
        assert_close(got['clip'], WC.weighted64(case, inp, None, norm)[3], *LOSS_TOL, 'clip_loss')


@pytest.mark.parametrize('norm', WC.NORMS)
def test_zero_relationship_denominator_leaves_the_interaction_half(norm):
    """mtmm with every labelled clip at weight 0, and mtmm without a labelled clip: the relationship half is 0 (loss and
    gradients), the interaction half is the float64 composition's"""
    for case in WC.ZERO_DEN[:2]:
        case = LC.seeded(case)
        inp = LC.make_inputs(case)
        lab = WC.labelled(case, inp)
        assert bool(lab.any()) == (case.r_mode != 'none')
        w = torch.where(lab, torch.zeros(case.B, dtype=torch.float64), WC.draw_weights(case.B, 7, zeros=0))
        got = run_kernel(case, inp, w, True, norm)
        ref = WC.weighted64(case, inp, w, norm)
        compare(case, inp, got, ref)
        assert not got['d_rels'].any() and float(got['loss']) > 0
        assert not ref[2].any()


# ---------------------------------------------------------------------------------------------------------------------------
# bit identity with the unweighted call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', WC.IDENTITY, ids=_ids(WC.IDENTITY))
def test_unit_weights_and_clip_loss_only_are_the_unweighted_bits(case):
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    for loader in (False, True):
        base = run_kernel(case, inp, loader=loader)
        for norm in WC.NORMS:
            for f64 in (False, True):
                same_bits(base, run_kernel(case, inp, torch.ones(case.B), f64, norm, loader=loader))
                same_bits(base, run_kernel(case, inp, torch.ones(case.B), f64, norm, clip_loss=True, loader=loader))
        only = run_kernel(case, inp, clip_loss=True, loader=loader)
        same_bits(base, only)
        assert_close(only['clip'], WC.weighted64(case, inp, None)[3], *LOSS_TOL, 'clip_loss')
    compare(case, inp, base, WC.weighted64(case, inp, None))


# ---------------------------------------------------------------------------------------------------------------------------
# the per-clip values
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', WC.NORMS)
@pytest.mark.parametrize('case', WC.CLIP_LOSS, ids=_ids(WC.CLIP_LOSS))
def test_clip_loss_values(case, norm, monkeypatch):
    """against the float64 per-clip terms; sum_b w_b clip_loss / D reproduces the returned loss; identical between the two-launch
    finalize (arrive == NULL) and the in-launch one; independent of the weights"""
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    w = WC.draw_weights(case.B, case.seed + 1)
    got = run_kernel(case, inp, w, True, norm, clip_loss=True)
    ref = WC.weighted64(case, inp, w, norm)
    compare(case, inp, got, ref)
    (den_i, den_r), _ = WC.denominators(case, inp, w, norm)
    clip = got['clip'].double()
    total = (w * clip[:, 0]).sum() / den_i + ((w * clip[:, 1]).sum() / den_r if den_r > 0 else 0.0)
    assert_close(got['loss'], total, *LOSS_TOL, 'loss from clip_loss')
    if case.form == 'mtmm':
        assert not got['clip'][~WC.labelled(case, inp), 1].any()                 # no relationship term: column 1 is 0
    monkeypatch.setattr(ops, '_arrive_counter', lambda dev: None)                # -> a.arrive = NULL
    two = run_kernel(case, inp, w, True, norm, clip_loss=True)
    assert torch.equal(two['clip'], got['clip']) and torch.equal(two['d_ints'], got['d_ints'])
    assert_close(two['loss'], ref[0], *LOSS_TOL, 'loss (two launches)')
    monkeypatch.undo()
    assert torch.equal(run_kernel(case, inp, clip_loss=True)['clip'], got['clip'])


# ---------------------------------------------------------------------------------------------------------------------------
# tr_cat_distr with an injected pick
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', WC.NORMS)
def test_sampled_form_with_an_injected_pick(norm):
    """sample = 1 with `sel`: the probabilities and the pick do not depend on the weights; loss and gradients are the float64
    composition's given the pick"""
    case = LC.seeded(WC.SAMPLED, 'sel')
    inp = LC.make_inputs(case)
    sel = LC.forced_tracks(case, inp)
    k = LC.positive(case, inp, 'sel')
    w = WC.draw_weights(case.B, 11)
    plain = run_kernel(case, inp, sel=sel, sample=1, want_probs=True)
    got = run_kernel(case, inp, w, True, norm, sel=sel, sample=1, want_probs=True, clip_loss=True)
    assert torch.equal(got['probs'], plain['probs']) and torch.equal(got['sel'], plain['sel']) and torch.equal(got['sel'], k)
    assert_close(got['probs'], LC.probs64(case, inp), 1e-4, 1e-6, 'probs_out')
    compare(case, inp, got, WC.weighted64(case, inp, w, norm, k=k), k=k)


# ---------------------------------------------------------------------------------------------------------------------------
# data-parallel divisors: two unequal halves with the global weight sums over 2
# ---------------------------------------------------------------------------------------------------------------------------
def _part(case, inp, a, b):
    return dataclasses.replace(case, B=b - a), {key: (None if v is None else v[a:b]) for key, v in inp.items()}


@pytest.mark.parametrize('norm', WC.NORMS)
@pytest.mark.parametrize('case', WC.DIVISORS, ids=_ids(WC.DIVISORS))
def test_halves_with_global_divisors_average_to_the_whole_batch(case, norm):
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    B = case.B
    cut = B // 2 - 1                                                     # unequal halves
    w = WC.draw_weights(B, case.seed + 2)
    whole = WC.weighted64(case, inp, w, norm)
    (den_i, den_r), _ = WC.denominators(case, inp, w, norm)
    div = (den_i / 2, den_r / 2)
    rs = LC.restate(case, inp)
    for as_device in (False, True):
        d = torch.tensor(div, dtype=torch.float32, device=DEV) if as_device else div
        parts = [run_kernel(*_part(case, inp, a, b), w[a:b], True, norm, divisors=d, clip_loss=True) for a, b in ((0, cut), (cut, B))]
        loss = (parts[0]['loss'].double() + parts[1]['loss'].double()) / 2
        assert_close(loss, whole[0], *LOSS_TOL, 'mean of the halves\' losses')
        # (averaged over the two ranks, the gradient of a clip is half its rank's: the kernel's own is twice the whole batch's)
        d_i = torch.cat([p['d_ints'] for p in parts]) / 2
        keep = ~rs['ex_ints']
        assert_close(d_i[keep], whole[1][keep], *GRAD_TOL, 'd_ints')
        d_r = torch.cat([p['d_rels'] for p in parts]) / 2
        keep = ~rs['ex_rels']
        assert_close(d_r[keep], whole[2][keep], *GRAD_TOL, 'd_rels')
        assert_close(torch.cat([p['clip'] for p in parts]), whole[3], *LOSS_TOL, 'clip_loss')


# ---------------------------------------------------------------------------------------------------------------------------
# heads forward + weighted loss + heads' data gradients in one call
# ---------------------------------------------------------------------------------------------------------------------------
def _P(t):
    return t.data_ptr()


@pytest.mark.parametrize('with_rels', [True, False], ids=['rels', 'ints'])
def test_fused_weighted_call_equals_the_three_calls(with_rels):
    """tests/test_gpu_losses.py:test_fused_heads_loss_call_equals_the_three_calls at T = 65 with clip weights and the per-clip
    values: bit for bit"""
    T = 65
    assert (T, with_rels) in LC.FUSED
    g = torch.Generator().manual_seed(77 + T)
    B, C_, NR, KG, KC = 3, 101, 15, 512, 256
    n = B * T
    G = torch.randn(n, KG, generator=g).to(DEV)
    E = torch.randn(n, KC, generator=g).to(DEV)
    Wi, bi = (torch.randn(C_, KG, generator=g) / KG ** 0.5).to(DEV), torch.randn(C_, generator=g).to(DEV)
    Wc, bc = (torch.randn(NR, KC, generator=g) / KC ** 0.5).to(DEV), torch.randn(NR, generator=g).to(DEV)
    nb = torch.tensor([T, 64 + 1, 7])
    mem = (torch.arange(T)[None, :] < nb[:, None]).float().to(DEV)
    w = (torch.rand(B, C_, generator=g) < 0.95).float().to(DEV)
    y = torch.randint(0, C_, (B,), generator=g, dtype=torch.int32).to(DEV)
    r = torch.randint(0, NR + 1, (B, T), generator=g, dtype=torch.int32).to(DEV)
    gt = torch.zeros(B, 2, dtype=torch.int32, device=DEV)
    cwt = torch.tensor([0.25, 3.0, 0.0], dtype=torch.float64, device=DEV)
    res = []
    for fused in (False, True):
        Yi, Yc = torch.empty(n, C_, device=DEV), torch.zeros(n, NR, device=DEV)
        dG, dE = torch.full((n, KG), 3.0, device=DEV), torch.full((n, KC), 3.0, device=DEV)
        dWi, dbi = torch.zeros_like(Wi), torch.zeros_like(bi)
        dWc, dbc = torch.zeros_like(Wc), torch.zeros_like(bc)
        cl = torch.full((B, 2), float('nan'), device=DEV)
        heads = [(_P(G), KG, Wi, bi, n, KG, C_, Yi, C_)] + ([(_P(E), KC, Wc, bc, n, KC, NR, Yc, NR)] if with_rels else [])
        drop = ops.make_dropout(0, 0.0)
        back = lambda di, dc: [(di, C_, _P(G), KG, Wi, n, KG, C_, dWi, dbi, _P(dG), KG, 0, None, KG, 0, drop)] + \
            ([(dc, NR, _P(E), KC, Wc, n, KC, NR, dWc, dbc, _P(dE), KC, 0, None, KC, 0, drop)] if with_rels else [])
        kw = dict(mem=mem, w=w, y=y, r=r if with_rels else None, g=gt, sel=None, B=B, T=T, Cc=C_, NR=NR if with_rels else 0,
                  margin=0.101, lymbda=0.7, max_neg=False, tr_correct=False, mask_inplace=True, rels_mean_valid=False,
                  clip_weight=cwt, clip_weight_norm='sum', clip_loss=cl)
        if fused:
            loss, d_i, d_c, sel, _ = ops.margin_loss(Yi, Yc if with_rels else None, heads=heads, back=back('ints', 'rels'), **kw)
        else:
            ops.linear_fwd_group(heads)
            loss, d_i, d_c, sel, _ = ops.margin_loss(Yi, Yc if with_rels else None, **kw)
            ops.linear_bwd_group(back(d_i, d_c), parts=2)
        torch.cuda.synchronize()
        res.append([t.clone() for t in (Yi, Yc, loss, d_i, dG, dE, sel, cl)] + ([d_c.clone()] if with_rels else []))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    loss, d_i, cl = res[0][2], res[0][3], res[0][7]
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(cl).all()) and float(res[0][4].abs().sum()) > 0
    assert not d_i.view(B, T, C_)[2].any() and d_i.view(B, T, C_)[1].any()                # (the clip at weight 0; a weighted one)
    wsum = float(cwt.sum())
    total = float(((cwt * cl[:, 0].double()).sum() + (cwt * cl[:, 1].double()).sum()) / wsum)
    assert abs(total - float(loss)) <= 1e-5 * abs(total) + 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# lirec_ce_loss_weighted
# ---------------------------------------------------------------------------------------------------------------------------
def _ce_inputs(B, C, NR, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    ints = torch.from_numpy(g.standard_normal((B, C)).astype(np.float32)) * 2
    rels = torch.from_numpy(g.standard_normal((B, NR)).astype(np.float32)) * 2
    y = torch.from_numpy(g.integers(0, C, B))
    r = torch.from_numpy(g.integers(0, NR + 1, B))
    r[0], r[B - 1] = NR, 0
    cw = torch.from_numpy(g.uniform(0.25, 4.0, C).astype(np.float32))
    return ints, rels, y, r, cw


def _ce_ref(ints, rels, y, r, cw, NR, w, norm):
    """F.cross_entropy in float64 with per-row weights: loss, gradients, per-clip values"""
    F = torch.nn.functional
    oi, orl = ints.double().requires_grad_(True), rels.double().requires_grad_(True)
    lab = (r != NR)
    ci = F.cross_entropy(oi, y, reduction='none') * (cw.double()[y] if cw is not None else 1.0)
    cr = torch.where(lab, F.cross_entropy(orl, torch.where(lab, r, torch.zeros_like(r)), reduction='none'), torch.zeros(len(r), dtype=torch.float64))
    cwy = cw.double()[y] if cw is not None else torch.ones(len(y), dtype=torch.float64)
    if norm == 'sum':
        di, dr = (w * cwy).sum(), (w * lab).sum()
    else:
        di, dr = cwy.sum(), lab.double().sum()
    loss = (w * ci).sum() / di if float(di) > 0 else torch.zeros((), dtype=torch.float64)
    if float(dr) > 0:
        loss = loss + (w * cr).sum() / dr
    loss = loss + 0.0 * (oi.sum() + orl.sum())
    loss.backward()
    return loss.detach(), oi.grad, orl.grad, torch.stack([ci.detach(), cr.detach()], 1), (float(di), float(dr))


@pytest.mark.parametrize('norm', WC.NORMS)
@pytest.mark.parametrize('class_w', [False, True], ids=['plain', 'class_w'])
@pytest.mark.parametrize('C', [7, 101])
def test_ce_loss_weighted(C, class_w, norm):
    B, NR = 9, 15
    ints, rels, y, r, cw = _ce_inputs(B, C, NR, 2700 + C)
    cw = cw if class_w else None
    dv = lambda t: None if t is None else t.to(DEV)
    args = (dv(ints), dv(rels), dv(y.int()), dv(r.int()), dv(cw), B, C, NR)
    base = [t.cpu() for t in ops.ce_loss(*args)]
    for f64 in (False, True):
        w = WC.draw_weights(B, 2800 + C)
        cl = torch.full((B, 2), float('nan'), device=DEV)
        got = ops.ce_loss(*args, clip_weight=_dev_w(w, f64), clip_weight_norm=norm, clip_loss=cl)
        torch.cuda.synchronize()
        loss, d_i, d_r, clip, (di, dr) = _ce_ref(ints, rels, y, r, cw, NR, _ref_w(w, f64), norm)
        print('ce loss %.9g want %.9g' % (float(got[0]), float(loss)))
        assert_close(got[0].cpu().reshape(()), loss, *LOSS_TOL, 'ce loss')
        assert_close(got[1].cpu(), d_i, *GRAD_TOL, 'd_ints')
        assert_close(got[2].cpu(), d_r, *GRAD_TOL, 'd_rels')
        assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[1], got[2], cl))
        assert_close(cl.cpu(), clip, *LOSS_TOL, 'clip_loss')
        rw = _ref_w(w, f64)
        total = (rw * cl.cpu().double()[:, 0]).sum() / di + (rw * cl.cpu().double()[:, 1]).sum() / dr
        assert_close(got[0].cpu().reshape(()), total, *LOSS_TOL, 'loss from clip_loss')
        # unit weights (either dtype, with and without the per-clip values): the bits of lirec_ce_loss
        ones = torch.ones(B, dtype=torch.float64 if f64 else torch.float32, device=DEV)
        for keep in (None, torch.empty((B, 2), device=DEV)):
            unit = ops.ce_loss(*args, clip_weight=ones, clip_weight_norm=norm, clip_loss=keep)
            assert all(torch.equal(a.cpu(), b) for a, b in zip(unit, base))
        only = ops.ce_loss(*args, clip_loss=cl)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(only, base))
        assert_close(cl.cpu(), clip, *LOSS_TOL, 'clip_loss (no weights)')
    # every weight 0: loss 0, zero gradients, no NaN
    zero = ops.ce_loss(*args, clip_weight=torch.zeros(B, device=DEV), clip_weight_norm=norm)
    assert float(zero[0]) == 0.0 and not zero[1].any() and not zero[2].any()


# ---------------------------------------------------------------------------------------------------------------------------
# through the model: batch['clip_weight'], keep_clip_losses, clip_losses(), the recorded step
# ---------------------------------------------------------------------------------------------------------------------------
DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)
SHAPE = dict(T=6, R=3, n_classes=11, n_rels=5, **DIMS)


def _small(norm='sum', kind='int_rel_ch'):
    """the reduced recipe of tests/test_gpu_loops.py / tests/test_gpu_parallel.py, dropout off"""
    from lirec_amd import config, model as M
    from lirec_amd.config import opt
    config.recipe(kind, joint_dim=16, rels_n_clips=3, dropout=0.0, dropout_seed=77, clip_weight_norm=norm, **DIMS)
    opt.device = 'cuda'
    torch.manual_seed(11)
    model, loss, optim = M.create_model(11, n_rels=5)
    model.train()
    return model, loss, optim


def _grads(model, loss, optim, batch):
    optim.zero_grad()
    lv = loss(model(dict(batch)), batch)
    lv.backward()
    torch.cuda.synchronize()
    return model.flat_grads(attach=False).detach().clone().cpu().double(), float(lv.detach().sum())


@pytest.mark.parametrize('norm', WC.NORMS)
def test_eager_step_with_clip_weight_in_the_batch(norm):
    """B = 8: the parameter gradients of one step with ``batch['clip_weight']`` equal the weight-combined gradients of eight
    one-clip steps (the bound of tests/test_gpu_parallel.py on averaged parameter gradients), and the per-clip values the loss
    kept are the one-clip losses"""
    from lirec_amd import config
    from lirec_amd.data import synthetic_batch, to_device_batch
    try:
        model, loss, optim = _small(norm)
        host = synthetic_batch(21, 'int_rel_ch', 8, **SHAPE)
        w = WC.draw_weights(8, 3)
        loss.keep_clip_losses = True
        g_w, l_w = _grads(model, loss, optim, dict(to_device_batch(host, 'cuda'), clip_weight=w))        # (a host tensor: checked, copied)
        clip = loss.last_clip_losses.cpu().double()
        assert clip.shape == (8, 2) and bool(torch.isfinite(clip).all())
        g_plain, _ = _grads(model, loss, optim, to_device_batch(host, 'cuda'))
        loss.keep_clip_losses = False
        den = float(w.sum()) if norm == 'sum' else 8.0
        g_ref, l_ref = torch.zeros_like(g_w), 0.0
        for b in range(8):
            one = to_device_batch({k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in host.items()}, 'cuda')
            g_b, l_b = _grads(model, loss, optim, one)
            assert loss.last_clip_losses is None
            g_ref += float(w[b]) * g_b / den
            l_ref += float(w[b]) * l_b / den
            assert abs(float(clip[b].sum()) - l_b) <= 1e-5 * abs(l_b) + 1e-6, (b, clip[b], l_b)
        scale = float(g_ref.abs().max())
        tol = 1e-6 + 1e-4 * g_ref.abs() + 6e-5 * scale
        assert ((g_w - g_ref).abs() <= tol).all(), ('weighted gradients differ', float((g_w - g_ref).abs().max()), scale)
        assert abs(l_w - l_ref) <= 1e-5 * abs(l_ref) + 1e-6
        assert float((g_plain - g_ref).abs().max()) > 1e-2 * scale, 'the weights were meant to matter'
        with pytest.raises(Exception, match='finite and non-negative'):
            loss(model(to_device_batch(host, 'cuda')), dict(to_device_batch(host, 'cuda'), clip_weight=-w))
    finally:
        config.reset()


def test_clip_losses_over_a_dataset_in_order():
    """40 clips in batches of 16 (the last one short): float32 [40, 2] in dataset order, equal to the per-batch
    ``last_clip_losses``; the model's mode and the loss's flag are as they were"""
    from lirec_amd import config
    from lirec_amd.data import SyntheticMixedFeaturesDataset, collate
    from lirec_amd.test import clip_losses
    try:
        model, loss, optim = _small()
        ds = SyntheticMixedFeaturesDataset('int_rel_ch', 40, seed=5, **SHAPE)
        got = clip_losses(ds, model, loss, batch_size=16)
        assert got.dtype == np.float32 and got.shape == (40, 2) and np.isfinite(got).all() and (got >= 0).all()
        assert model.training and loss.keep_clip_losses is False and loss.last_clip_losses is None
        model.eval()
        loss.keep_clip_losses = True
        with torch.no_grad():
            for lo in (0, 16, 32):
                ids = range(lo, min(lo + 16, 40))
                batch = collate([ds[i] for i in ids])
                lv = loss(model(batch), batch)
                part = loss.last_clip_losses.cpu().numpy()
                assert part.shape == (len(ids), 2) and np.array_equal(part, got[lo:lo + len(ids)]), lo
                mean = float(part.astype(np.float64).sum() / len(ids))
                assert abs(mean - float(lv)) <= 1e-5 * abs(mean) + 1e-6                   # (unweighted: the batch's loss is their mean)
        assert len({float(v) for v in got[:, 0]}) > 30                                    # (clips differ: an order can be told)
    finally:
        config.reset()


def test_recorded_step_reads_refilled_weights_in_place():
    """a resident store whose dataset carries weights: the batch buffer holds ``clip_weight`` as its tenth field, the step is
    recorded on one batch, the buffer is refilled with a batch of OTHER weights, and the replay equals the eager step on that batch
    bit for bit (parameters after the update)"""
    from lirec_amd import config, features as F
    from lirec_amd.graph import RecordedTrainStep
    from lirec_amd.loader import device_collate_in_force
    from lirec_amd.config import opt
    from test_pieces_entry import R, _fresh, _world
    world = _world(21, n_scenes=5, per_scene=5)                                # 25 clips
    try:
        w = WC.draw_weights(25, 9).numpy()
        res = {}
        for how in ('eager', 'recorded', 'recorded-unweighted'):
            model, loss, optim = _fresh(world)
            model.train()
            optim.param_groups[0]['lr'] = 1e-3
            ds = F.PiecesDataset(world, R, resident=True, clip_weight=None if how.endswith('unweighted') else w)
            opt.device_collate = True
            assert device_collate_in_force(ds) == how.endswith('unweighted')      # (weights: the threaded host collate)
            host = [ds.collate_fn([ds[i] for i in ids]) for ids in (list(range(8)), list(range(12, 20)))]
            assert tuple(host[0]['_layout']) == tuple(host[1]['_layout'])                 # (the static layout of a resident store)
            assert (host[0]['_layout'][-1][0] == 'clip_weight') == (not how.endswith('unweighted'))
            a, b = ds.to_device(host[0]), ds.to_device(host[1])
            assert ('clip_weight' in a) == (not how.endswith('unweighted'))
            if 'clip_weight' in a:
                assert a['clip_weight'].is_cuda and a['clip_weight'].dtype == torch.float64
                assert not torch.equal(a['clip_weight'], b['clip_weight'])
            def eager(batch):
                optim.zero_grad()
                lv = loss(model(dict(batch)), batch)
                lv.backward()
                optim.step()
                return lv
            eager(a)
            eager(a)
            if how == 'eager':
                eager(a)
                lv = eager(b)
            else:
                rec = RecordedTrainStep(model, loss, optim, a, warmup=0)       # the third step on `a`, recorded
                a['_dev_blob'].copy_(b['_dev_blob'])
                lv = rec.step()
                torch.cuda.synchronize()
                rec.release()
            torch.cuda.synchronize()
            res[how] = (model.flat_params().detach().clone(), float(lv.detach().reshape(-1)[0]))
        assert torch.equal(res['eager'][0], res['recorded'][0]), float((res['eager'][0] - res['recorded'][0]).abs().max())
        assert res['eager'][1] == res['recorded'][1]
        assert not torch.equal(res['recorded'][0], res['recorded-unweighted'][0])
    finally:
        config.reset()
