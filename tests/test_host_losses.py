"""The loss and evaluation calls without a GPU: their argument checks through the C ABI (LIREC_EINVAL before any device call), the
dynamic-LDS limit of both launchers, and the yardstick of tests/test_gpu_losses.py -- the float64 oracle -- checked on its own:
its gradients equal a central finite difference of its loss, the float64 restatement of its hinge terms (tests/loss_cases.py)
gives its loss, and the caps on what the GPU file leaves out of a gradient comparison hold for every case and seed used there."""
import ctypes as C
import dataclasses

import pytest
import torch

import loss_cases as LC
from lirec_amd import _lib

DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
A0 = 0x10000000                                # fake, aligned, never dereferenced device addresses


def _addr(i):
    return A0 + 0x1000000 * i


def _loss_args(B=4, T=20, Cc=101, NR=15, rels=True):
    a = _lib.MarginLossArgs()
    a.ints, a.ld_ints = _addr(0), Cc
    if rels:
        a.rels, a.ld_rels, a.r, a.d_rels, a.ld_drels = _addr(1), NR, _addr(5), _addr(9), NR
    a.mem, a.w, a.y, a.g = _addr(2), _addr(3), _addr(4), _addr(6)
    a.d_ints, a.ld_dints = _addr(8), Cc
    a.loss, a.partial, a.sel_out, a.arrive = _addr(10), _addr(11), _addr(12), _addr(13)
    a.B, a.T, a.C, a.NR = B, T, Cc, NR if rels else 0
    a.margin, a.lymbda = 0.101, 1.0
    return a


def _eval_args(B=4, T=20, Cc=101, NR=15, rels=True):
    a = _lib.EvalArgs()
    a.ints, a.ld_ints = _addr(0), Cc
    if rels:
        a.rels, a.ld_rels, a.r = _addr(1), NR, _addr(5)
    a.mem, a.y, a.g, a.counters = _addr(2), _addr(4), _addr(6), _addr(7)
    a.B, a.T, a.C, a.NR = B, T, Cc, NR if rels else 0
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


LOSS_BREAKS = {
    'rels_mean_valid_T2': _set(rels_mean_valid=1, T=2),
    'sample_with_tr_correct': _set(sample=1, tr_correct=1),
    'sample_3': _set(sample=3),
    'sample_negative': _set(sample=-1),
    'batch_divisor_negative': _set(batch_divisor=-1.0),
    'rels_divisor_negative': _set(rels_divisor=-0.5),
    'rels_without_r': _set(r=None),
    'rels_without_d_rels': _set(d_rels=None),
    'rels_NR0': _set(NR=0),
    'sample2_without_outputs': _set(sample=2, probs_out=None, sel_out=None),
    'no_ints': _set(ints=None),
    'no_y': _set(y=None),
    'no_d_ints': _set(d_ints=None),
    'no_loss': _set(loss=None),
    'no_partial': _set(partial=None),
    'B0': _set(B=0),
    'T0': _set(T=0),
    'C0': _set(C=0),
    'lds_T_one_too_many': _set(T=LC.T_MAX + 1),
    'lds_C_too_large': _set(T=64, C=1000),
}


@pytest.mark.parametrize('what', sorted(LOSS_BREAKS))
def test_margin_loss_argument_checks(what):
    L = _lib.lib()
    a = _loss_args()
    LOSS_BREAKS[what](a)
    assert L.lirec_margin_loss(C.byref(a), None) == _lib.LIREC_EINVAL
    assert L.lirec_margin_loss(None, None) == _lib.LIREC_EINVAL


EVAL_BREAKS = {
    'no_ints': _set(ints=None), 'no_y': _set(y=None), 'no_g': _set(g=None), 'no_counters': _set(counters=None),
    'rels_without_r': _set(r=None), 'rels_NR0': _set(NR=0), 'B0': _set(B=0), 'T0': _set(T=0), 'C0': _set(C=0),
    'lds_T_one_too_many': _set(T=LC.largest_T(LC.lds_eval, 101, 15) + 1),
}


@pytest.mark.parametrize('what', sorted(EVAL_BREAKS))
def test_eval_argument_checks(what):
    L = _lib.lib()
    a = _eval_args()
    EVAL_BREAKS[what](a)
    assert L.lirec_eval_max_tracks(C.byref(a), None) == _lib.LIREC_EINVAL
    assert L.lirec_eval_max_tracks(None, None) == _lib.LIREC_EINVAL


def _ce(L, **kw):
    v = dict(ints=_addr(0), ld_ints=101, rels=_addr(1), ld_rels=15, y=_addr(2), r=_addr(3), class_w=None, B=4, C=101, NR=15,
             d_ints=_addr(4), ld_dints=101, d_rels=_addr(5), ld_drels=15, loss=_addr(6), partial=_addr(7), den_ints=0.0,
             den_rels=0.0, dens_dev=None)
    v.update(kw)
    return L.lirec_ce_loss(*v.values(), None)


@pytest.mark.parametrize('kw', [dict(den_ints=-1.0), dict(den_rels=-0.25), dict(ints=None), dict(y=None), dict(d_ints=None),
                                dict(loss=None), dict(partial=None), dict(B=0), dict(C=0), dict(r=None), dict(d_rels=None),
                                dict(NR=0)], ids=lambda kw: '-'.join(kw))
def test_ce_loss_argument_checks(kw):
    assert _ce(_lib.lib(), **kw) == _lib.LIREC_EINVAL


def test_lds_limit_is_the_header_formula():
    """The largest track counts the launchers admit, derived from their formulas: one track more is LIREC_EINVAL before any device
    call; the largest passes the check (under the library's host dry run, which hands nothing to the HIP runtime)."""
    L = _lib.lib()
    t_loss, t_eval = LC.largest_T(LC.lds_loss, 101, 15), LC.largest_T(LC.lds_eval, 101, 15)
    assert (t_loss, t_eval) == (343, 173)                                      # (what the formulas give today)
    assert LC.lds_loss(t_loss, 101, 15) <= LC.LDS_LIMIT < LC.lds_loss(t_loss + 1, 101, 15)
    assert LC.lds_eval(t_eval, 101, 15) <= LC.LDS_LIMIT < LC.lds_eval(t_eval + 1, 101, 15)
    assert LC.lds_loss(129, 101, 15) <= 64 * 1024 < LC.lds_loss(200, 101, 15) and LC.lds_loss(17, 1000, 15) > 64 * 1024
    a, e = _loss_args(T=t_loss + 1), _eval_args(T=t_eval + 1)
    assert L.lirec_margin_loss(C.byref(a), None) == _lib.LIREC_EINVAL
    assert L.lirec_eval_max_tracks(C.byref(e), None) == _lib.LIREC_EINVAL
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        a, e = _loss_args(T=t_loss), _eval_args(T=t_eval)
        assert L.lirec_margin_loss(C.byref(a), None) == 0
        assert L.lirec_eval_max_tracks(C.byref(e), None) == 0
        # without rels the tables are smaller: more tracks fit
        t2 = LC.largest_T(LC.lds_loss, 101, 15, rels=False)
        assert t2 > t_loss
        assert L.lirec_margin_loss(C.byref(_loss_args(T=t2, rels=False)), None) == 0
        # ... and the argument checks hold with the launches "succeeding"
        assert L.lirec_margin_loss(C.byref(_loss_args(T=t2 + 1, rels=False)), None) == _lib.LIREC_EINVAL
        a = _loss_args(T=2)
        a.rels_mean_valid = 1
        assert L.lirec_margin_loss(C.byref(a), None) == _lib.LIREC_EINVAL
    finally:
        assert L.lirec_debug_set(0, -1) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick on its own
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_loss_follows_the_logits_dtype():
    """float64 logits give a float64 loss (the accumulator once was a float32 zero, which kept the sum float32); float32 logits
    give the float32 loss they always gave (tests/test_oracle_golden.py pins those bits)."""
    for c in (LC.Case('mtmm', 5, 1, 11, 5, seed=1), LC.Case('mtr', 4, 6, 11, 5, seed=2), LC.Case('mtr', 4, 6, 11, 5, max_neg=True, seed=2)):
        inp = LC.make_inputs(c)
        l64 = LC.oracle64(c, inp)[0]
        assert l64.dtype == torch.float64
        from oracle import lirec_oracle as O
        batch = {'labels': inp['y'].view(-1, 1, 1).expand(-1, 2, 1) if c.form == 'mtmm' else inp['y'], 'mem_mask': inp['mem'].double(),
                 'rels_label': inp['r'][:, 0] if c.form == 'mtmm' else inp['r'], 'gt_tracks': inp['gt'], 'multilab_weights': inp['w'].double()}
        if c.form == 'mtmm':
            l32 = O.multitask_maxmargin_loss(c.cfg(), {'inters': inp['ints'][:, 0].clone(), 'rels': inp['rels'][:, 0]}, batch, c.NR)
        else:
            l32 = O.margin_track_rels_loss(c.cfg(), {'inters': inp['ints'].clone(), 'rels': inp['rels']}, batch, c.NR)
        assert l32.dtype == torch.float32 and l32.shape == (1,)
        assert abs(float(l32) - float(l64)) <= 1e-6 * abs(float(l64))
        assert float(l64) != float(l64.float())                 # (it carries more than float32 holds)


FD_CASES = [LC.Case('mmce', 4, 1, 9, 3, seed=3), LC.Case('mtmm', 5, 1, 9, 4, seed=4),
            LC.Case('margin', 3, 5, 7, 3, seed=5), LC.Case('margin', 3, 5, 7, 3, seed=5, max_neg=True),
            LC.Case('mtr', 3, 5, 7, 3, seed=6), LC.Case('mtr', 3, 5, 7, 3, seed=6, max_neg=True),
            LC.Case('mtr', 3, 5, 7, 3, seed=7, tr_correct=True, g_mode='rand'),
            LC.Case('mtr', 3, 5, 7, 3, seed=7, tr_correct=True, g_mode='rand', max_neg=True)]


@pytest.mark.parametrize('case', FD_CASES, ids=[LC.case_id(c) for c in FD_CASES])
def test_oracle_gradients_are_the_finite_difference_of_its_loss(case):
    """The GPU file compares kernels with the oracle's autograd gradients: here those equal a central difference of the oracle's
    float64 loss, element by element -- two copies of one mistake would not.  (Step 1e-6: every hinge term, column gap and
    track gap of the seeds chosen is at least 1e-5 from its kink.)"""
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    rs = LC.restate(case, inp)
    assert rs['share'] == 0.0
    _, d_i, d_r, _ = LC.oracle64(case, inp)
    h = 1e-6
    for key, grad in (('ints', d_i), ('rels', d_r)):
        if grad is None:
            continue
        assert float(grad.abs().sum()) > 0
        base = inp[key].double()
        valid = inp['mem'].bool().unsqueeze(2).expand_as(base)
        fd = torch.zeros_like(base)
        for i in torch.nonzero(valid.reshape(-1)).view(-1).tolist():
            vals = []
            for sgn in (1.0, -1.0):
                x = base.clone().view(-1)
                x[i] += sgn * h
                vals.append(float(_loss64_of(case, inp, key, x.view_as(base))))
            fd.view(-1)[i] = (vals[0] - vals[1]) / (2 * h)
        assert float((fd - grad).abs().max()) <= 1e-8 + 1e-6 * float(grad.abs().max()), (key, float((fd - grad).abs().max()))
        assert float(grad[~valid].abs().sum()) == 0.0


def _loss64_of(case, inp, key, value):
    """the oracle's float64 loss with one input replaced by a float64 tensor (LC.oracle64 converts the float32 inputs itself)"""
    class _Keep(dict):
        pass
    inp2 = _Keep(inp)
    inp2[key] = _F64(value)
    return LC.oracle64(case, inp2)[0]


class _F64:
    """a stand-in for a float32 input tensor whose .double() is the given float64 tensor"""

    def __init__(self, v):
        self.v = v

    def double(self):
        return self.v


ALL = LC.all_margin_cases()


@pytest.mark.parametrize('group,case,how', ALL, ids=['%s-%s-%s' % (g, LC.case_id(c), h) for g, c, h in ALL])
def test_caps_of_every_gpu_case(group, case, how):
    """For the seed the GPU file uses: the restated loss is the oracle's (1e-12), the restated positive track reproduces the
    oracle's loss when injected, no clip's positive-track argmax is within 1e-5 (wanted ties excepted), and at most 1e-4 of the
    gradient elements (rows, max variant) depend on a decision within 1e-5 of its kink."""
    c = LC.seeded(case, how)
    assert c.seed - case.seed < 50
    inp = LC.make_inputs(c)
    k = LC.positive(c, inp, how)
    rs = LC.restate(c, inp, k)
    loss = LC.oracle64(c, inp, k)[0]
    assert abs(float(rs['loss']) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert rs['share'] <= LC.EXCL_CAP
    if c.form in ('margin', 'mtr') and not c.tr_correct:
        # the argmax the restatement finds IS the oracle's: injected as the pick, it gives the oracle's own loss
        k_arg = rs['k_arg']
        same = LC.oracle64(c, inp, k_arg)[0]
        if how is None:
            assert float(same) == float(loss)
        if how in (None, 'sel_mixed'):
            gap = rs['gap'].clone()
            if c.tie_clip is not None:
                assert float(gap[c.tie_clip]) == 0.0 and int(k_arg[c.tie_clip]) == 0
                gap[c.tie_clip] = 1.0
            assert float(gap.min()) >= LC.GAP_EPS or c.T == 1
        assert bool((inp['mem'][torch.arange(c.B), rs['k']] == 1).all())
    if c.ends:
        nv = inp['mem'].sum(1).long().tolist()
        assert 1 in nv and c.T in nv                                  # one valid track; every track valid


def test_case_list_covers_what_it_claims():
    Ts = {c.T for _, c, _ in ALL}
    assert {1, 2, 63, 64, 65, 128, 129, 200, LC.T_MAX} <= Ts
    assert {1, 7, 64, 65, 257, 1000} <= {c.C for c in LC.CLASSES} and {1, 15, 40, 70} <= {c.NR for c in LC.CLASSES}
    assert all(LC.lds_loss(c.T, c.C, c.NR, c.rels) > 64 * 1024 for c in LC.BIG_LDS)
    assert all(LC.lds_loss(c.T, c.C, c.NR, c.rels) <= LC.LDS_LIMIT for _, c, _ in ALL)
    assert {c.form for c in LC.FORMS} == {'mmce', 'mtmm', 'margin', 'mtr'}
    for c in LC.SAMPLER:
        if c.rels:
            inp = LC.make_inputs(LC.seeded(dataclasses.replace(c), 'sample'))
            b = c.r0_none[0]
            assert int(inp['r'][b, inp['gt'][b, 0]]) == c.NR
            p = LC.probs64(c, inp)
            assert bool(torch.isfinite(p).all()) and abs(float(p[b].sum()) - 0.5) < 1e-12      # (the rels half vanished: NaN -> 0)
            assert float((p * (1 - inp['mem'])).abs().sum()) == 0.0
