"""The weighted reference of the clip-weight tests (tests/test_gpu_clip_weights.py, tests/test_host_clip_weights.py) -- not a
test module.

The yardstick is the float64 oracle of tests/loss_cases.py (``oracle64``), composed, not restated: the oracle has no clip weights,
so a case is cut into one-clip slices (``dataclasses.replace(case, B=1)`` and the ``[b:b+1]`` slice of the inputs) and

    oracle64 with lymbda = 0            gives lr_b, the clip's relationship term, and its gradient,
    oracle64 with lymbda = 1, less lr_b gives li_b, the clip's interaction term, and its gradient

(a slice with no labelled relationship has no relationship term: NaN / no gradient count as 0).  The weighted loss and gradients
are then formed in float64 by the formula of include/lirec_hip.h (lirec_clip_weights):

    loss = lymbda * sum_b w_b li_b / D_i + sum_b w_b lr_b / D_r

tests/test_host_clip_weights.py pins the composition to ``oracle64`` of the whole batch at unit weights (1e-12).  The near-zero
hinge and near-tie exclusions do not depend on the weights: they are ``loss_cases.restate`` / ``caps_hold`` / ``seeded`` of the
whole case, unchanged.
"""
import dataclasses

import numpy as np
import torch

import loss_cases as LC

NORMS = ('sum', 'count')


def clip_slice(inp, b):
    return {key: (None if v is None else v[b:b + 1]) for key, v in inp.items()}


def clip_terms64(case: LC.Case, inp, k=None):
    """Per clip, from one-clip oracle calls: li [B], lr [B] (both before lymbda and the means), their gradients gi [B,T,C] and
    gr [B,T,NR] | None, and the logits after the loss's in-place masking [B,T,C]."""
    B = case.B
    li, lr = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    gi, gr, xm = [], [], []
    for b in range(B):
        one, sl = dataclasses.replace(case, B=1), clip_slice(inp, b)
        kb = None if k is None else torch.as_tensor(k)[b:b + 1]
        if case.rels:
            l0, _, g0, _ = LC.oracle64(dataclasses.replace(one, lymbda=0.0), sl, kb)
            if not bool(torch.isfinite(l0)):
                l0, g0 = torch.zeros((), dtype=torch.float64), torch.zeros_like(g0)
            g0 = torch.where(torch.isfinite(g0), g0, torch.zeros_like(g0))
            l1, g1, _, x = LC.oracle64(dataclasses.replace(one, lymbda=1.0), sl, kb)
            assert bool(torch.isfinite(l1)), 'the interaction term of a one-clip slice is always defined'
            lr[b], li[b] = l0, l1 - l0
            gr.append(g0)
        else:
            l1, g1, _, x = LC.oracle64(one, sl, kb)
            li[b] = l1
        gi.append(g1)
        xm.append(x)
    return dict(li=li, lr=lr, gi=torch.cat(gi), gr=torch.cat(gr) if case.rels else None, xm=torch.cat(xm))


def labelled(case: LC.Case, inp):
    """[B] bool: the clips the relationship mean runs over (the multitask clip loss: label != NR; every other loss: all)"""
    if case.form == 'mtmm':
        return inp['r'][:, 0] != case.NR
    return torch.ones(case.B, dtype=torch.bool)


def denominators(case: LC.Case, inp, w, norm, divisors=None):
    """(D_i, D_r) in float64: this batch's own by ``norm``, an entry of ``divisors`` > 0 in its place"""
    lab = labelled(case, inp).double()
    w = torch.ones(case.B, dtype=torch.float64) if w is None else w.double()
    if norm == 'sum':
        own = (float(w.sum()), float((w * lab).sum()))
    else:
        own = (float(case.B), float(lab.sum()))
    if divisors is None:
        return own, own
    given = tuple(float(d) if float(d) > 0 else o for d, o in zip(divisors, own))
    return own, given


def weighted64(case: LC.Case, inp, w, norm='sum', k=None, divisors=None, terms=None):
    """loss (0-dim float64), d_ints [B,T,C], d_rels [B,T,NR] | None, per-clip values [B,2] = (lymbda * li_b, lr_b), masked logits.
    A denominator of 0 (this batch's own) leaves its half at 0."""
    t = terms if terms is not None else clip_terms64(case, inp, k)
    wd = torch.ones(case.B, dtype=torch.float64) if w is None else w.double()
    (own_i, own_r), (di, dr) = denominators(case, inp, w, norm, divisors)
    ci = case.lym * wd / di if own_i > 0 else torch.zeros_like(wd)
    cr = wd / dr if own_r > 0 else torch.zeros_like(wd)
    if not case.rels:
        cr = torch.zeros_like(wd)
    loss = (ci * t['li']).sum() + (cr * t['lr']).sum()
    d_i = ci.view(-1, 1, 1) * t['gi']
    d_r = cr.view(-1, 1, 1) * t['gr'] if case.rels else None
    clip = torch.stack([case.lym * t['li'], t['lr']], 1)
    return loss, d_i, d_r, clip, t['xm']


def draw_weights(B, seed, zeros=2):
    """[B] float64 weights, log-uniform in [1e-3, 1e3], ``zeros`` clips at exactly 0 (never the first or the last clip, which the
    multitask cases keep unlabelled / labelled)."""
    g = np.random.Generator(np.random.PCG64(seed))
    w = 10.0 ** g.uniform(-3.0, 3.0, B)
    if zeros and B > 2:
        w[g.choice(np.arange(1, B - 1), size=min(zeros, B - 2), replace=False)] = 0.0
    return torch.from_numpy(w)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_clip_weights.py
# ---------------------------------------------------------------------------------------------------------------------------
def _both(form, B, T, C, NR, **kw):
    return [LC.Case(form, B, T, C, NR, max_neg=mx, **kw) for mx in (False, True)]


# mmce / mtmm at B = 9, T = 1; margin at B = 6, T = 20 and B = 5, T = 65 (crosses the 64-lane step); mtr at B = 16, T = 20 and at
# B = 300, T = 3, C = 11, NR = 5 (more clips than the 256 threads that sum the weights)
# (the max-over-classes variant belongs to the two track losses, mlp/model.py:483-486, :557-562: the clip losses have none, and
#  neither their modules nor the oracle take the flag)
FORMS = ([LC.Case('mmce', 9, 1, 101, 15, seed=2100), LC.Case('mtmm', 9, 1, 101, 15, seed=2101)]
         + _both('margin', 6, 20, 101, 15, seed=2102) + _both('margin', 5, 65, 101, 15, seed=2103, ends=(1, 37, 65, 65, 65))
         + _both('mtr', 16, 20, 101, 15, seed=2104) + _both('mtr', 300, 3, 11, 5, seed=2105))

ZERO_DEN = [LC.Case('mtmm', 9, 1, 101, 15, seed=2200), LC.Case('mtmm', 7, 1, 101, 15, seed=2201, r_mode='none'),
            LC.Case('mtr', 6, 20, 101, 15, seed=2202), LC.Case('mmce', 9, 1, 101, 15, seed=2203)]

IDENTITY = [LC.Case('mmce', 9, 1, 101, 15, seed=2300), LC.Case('mtmm', 9, 1, 101, 15, seed=2301),
            LC.Case('margin', 5, 65, 101, 15, seed=2302, max_neg=True), LC.Case('mtr', 16, 20, 101, 15, seed=2303),
            LC.Case('mtr', 300, 3, 11, 5, seed=2304)]

CLIP_LOSS = [LC.Case('mtmm', 9, 1, 101, 15, seed=2400), LC.Case('mtr', 16, 20, 101, 15, seed=2401),
             LC.Case('mtr', 300, 3, 11, 5, seed=2402, max_neg=True), LC.Case('margin', 5, 65, 101, 15, seed=2403)]

SAMPLED = LC.Case('mtr', 8, 20, 101, 15, seed=2500)

DIVISORS = [LC.Case('mtr', 16, 20, 101, 15, seed=2600), LC.Case('mtmm', 9, 1, 101, 15, seed=2601)]


def all_cases():
    """(case, how) of every margin case of the GPU file whose gradients are compared with float64"""
    out = [(c, None) for c in FORMS + ZERO_DEN + IDENTITY + CLIP_LOSS + DIVISORS]
    return out + [(SAMPLED, 'sel')]
