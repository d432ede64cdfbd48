"""Cases of the loss / evaluation kernel tests (tests/test_gpu_losses.py, tests/test_host_losses.py) -- not a test module.

The yardstick of both files is the oracle's own loss functions on FLOAT64 logits with autograd (``oracle64``).  Next to it stands a
short float64 restatement of the hinge terms (``restate``): the oracle returns a loss and gradients, not the per-term values, and
the discrete decisions the float32 kernel may take the other way -- a hinge term within rounding of 0, two tracks or two columns
whose scores tie within rounding -- are found from those terms.  tests/test_host_losses.py pins the restatement to the oracle
(its loss equals the oracle's to 1e-12, its positive track reproduces the oracle's loss when injected) and asserts the caps on
what may be left out, for every case and seed the GPU file uses.
"""
import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import lirec_oracle as O

MARGIN = 0.101
HINGE_EPS = 1e-5          # a float64 hinge term this close to 0 may be active on one side and not on the other
GAP_EPS = 1e-5            # ... and two scores this close may change places
EXCL_CAP = 1e-4           # largest share of gradient elements (sum variant) / rows (max variant) a case may leave out
LDS_LIMIT = 160 * 1024    # bytes of dynamic LDS the launchers admit (lirec_amd/csrc/lirec_hip.hip)


def lds_loss(T, C, NR, rels=True):
    """lirec_margin_loss's LDS need in bytes (the launcher's formula)."""
    NR1 = NR + 1 if rels else 0
    return (T * C + T * NR1 + 16 + 4 + 2 * T + C) * 4


def lds_eval(T, C, NR, rels=True):
    """lirec_eval_max_tracks's LDS need in bytes (the launcher's formula)."""
    nr, NR1 = (NR, NR + 1) if rels else (0, 0)
    return (2 * T * C + T * (nr + NR1) + 512) * 4


def largest_T(need, C, NR, rels=True):
    T = 1
    while need(T + 1, C, NR, rels) <= LDS_LIMIT:
        T += 1
    return T


@dataclasses.dataclass(frozen=True)
class Case:
    """One call of lirec_margin_loss.  form: 'mmce' MaxMarginCrossEntropyLoss (T = 1, no rels), 'mtmm' MultiTaskMaxMargin (T = 1,
    rels_mean_valid), 'margin' MarginLoss (rels NULL), 'mtr' MarginTrackRelsLoss."""
    form: str
    B: int
    T: int
    C: int
    NR: int
    max_neg: bool = False
    tr_correct: bool = False
    seed: int = 0
    lymbda: float = 0.7
    ends: Tuple[int, ...] = ()        # valid-prefix lengths of the first clips (the others keep the generator's)
    g_mode: str = 'zero'              # gt_tracks[:, 0]: 'zero' | 'rand' (any valid track) | 'equal' (== gt_tracks[:, 1])
    r_mode: str = 'rand'              # relationship labels: 'rand' | 'none' (all None) | 'one' (exactly one clip labelled; mtmm)
    r0_none: Tuple[int, ...] = ()     # clips whose ground-truth pair carries the label None
    mem_null: bool = False
    w_null: bool = False
    tie_clip: Optional[int] = None    # a clip whose tracks all carry the same logits (every track valid): the first index must win

    @property
    def rels(self):
        return self.form in ('mtmm', 'mtr')

    @property
    def lym(self):
        return self.lymbda if self.rels else 1.0          # (the two single-task losses have no lymbda)

    def cfg(self, sampled=False):
        return O.OracleCfg(margin=MARGIN, tr_margin=MARGIN, lymbda=self.lym, tr_correct=self.tr_correct, tr_max_neg=self.max_neg,
                           tr_cat_distr=sampled, tr_maximize=self.form in ('margin', 'mtr'))


def make_inputs(case: Case, seed=None):
    """The generator of tests/test_gpu_ops.py:_margin_inputs (standard-normal logits, a random valid prefix, two zeroed multilab
    columns per clip), then the case's own settings on top (drawn AFTER the base draws, which therefore stay what they were)."""
    B, T, C, NR = case.B, case.T, case.C, case.NR
    g = np.random.Generator(np.random.PCG64(case.seed if seed is None else seed))
    ints = torch.from_numpy(g.standard_normal((B, T, C)).astype(np.float32))
    rels = torch.from_numpy(g.standard_normal((B, T, NR)).astype(np.float32))
    mem = torch.zeros(B, T)
    for b in range(B):
        mem[b, :int(g.integers(1, T + 1))] = 1
    y = torch.from_numpy(g.integers(0, C, B))
    r = torch.from_numpy(g.integers(0, NR + 1, (B, T)))
    gt1 = [int(g.integers(0, int(mem[b].sum()))) for b in range(B)]
    w = torch.ones(B, C)
    for b in range(B):
        w[b, g.integers(0, C, 2)] = 0
    # --- the case's settings
    for b, n in enumerate(case.ends[:B]):
        mem[b] = 0
        mem[b, :n] = 1
    if case.tie_clip is not None:                          # every track a copy of the first: the track scores tie EXACTLY
        tb = case.tie_clip
        ints[tb] = ints[tb, 0].clone()
        rels[tb] = rels[tb, 0].clone()
        r[tb] = int(r[tb, 0]) % NR
        mem[tb] = 1
    if case.mem_null:
        mem[:] = 1
    nv = mem.sum(1).long()
    gt1 = [min(gt1[b], int(nv[b]) - 1) for b in range(B)]
    if case.g_mode == 'zero':
        gt0 = [0] * B
    elif case.g_mode == 'rand':
        gt0 = [int(g.integers(0, int(nv[b]))) for b in range(B)]
        if T > 1 and int(nv[0]) > 1:
            gt0[0] = max(gt0[0], 1)                         # at least one clip with g[:, 0] != 0
    else:
        gt0 = list(gt1)
    gt = torch.tensor([gt0, gt1], dtype=torch.long).t().contiguous()
    if case.r_mode == 'none':
        r[:] = NR
    elif case.r_mode == 'one':
        r[:] = NR
        r[B // 2] = int(g.integers(0, NR))
    elif case.form == 'mtmm':                               # labelled and None clips mixed, whatever the draw gave
        r[0], r[B - 1] = NR, int(g.integers(0, NR))
    for b in case.r0_none:
        r[b, gt[b, 0]] = NR
    if case.w_null:
        w[:] = 1
    return dict(ints=ints, rels=rels if case.rels else None, mem=mem, y=y, r=r, gt=gt, w=w)


def oracle64(case: Case, inp, k=None, dp=None):
    """The oracle's loss function of the case on float64 logits.  ``k``: an injected positive track per clip (the oracle's
    tr_cat_distr path with a sampler that returns it).  Returns loss (float64, 0-dim), d_ints [B,T,C], d_rels [B,T,NR] | None and
    the logits after the loss's in-place masking."""
    B, T, C, NR = case.B, case.T, case.C, case.NR
    x = inp['ints'].double().clone().requires_grad_(True)
    q = inp['rels'].double().clone().requires_grad_(True) if case.rels else None
    x2 = x * 1.0
    sampler = (lambda p: torch.as_tensor(k).long()) if k is not None else None
    cfg = case.cfg(sampled=k is not None)
    wts = inp['w'].double()
    if case.form == 'mmce':
        assert T == 1 and k is None and dp is None
        loss = O.maxmargin_ce_loss(cfg, {'inters': x2[:, 0]}, {'labels': inp['y'], 'multilab_weights': wts})
    elif case.form == 'mtmm':
        assert T == 1 and k is None
        batch = {'labels': inp['y'].view(B, 1, 1).expand(B, 2, 1), 'rels_label': inp['r'][:, 0], 'multilab_weights': wts}
        loss = O.multitask_maxmargin_loss(cfg, {'inters': x2[:, 0], 'rels': q[:, 0]}, batch, NR, dp=dp)
    else:
        assert dp is None
        batch = {'labels': inp['y'], 'mem_mask': inp['mem'].double(), 'rels_label': inp['r'], 'gt_tracks': inp['gt'],
                 'multilab_weights': wts}
        if case.form == 'margin':
            loss = O.margin_loss(cfg, {'inters': x2}, batch, sampler)
        else:
            loss = O.margin_track_rels_loss(cfg, {'inters': x2, 'rels': q}, batch, NR, sampler)
    loss = loss.sum()
    assert loss.dtype == torch.float64
    loss.backward()
    d_rels = None if not case.rels else (q.grad if q.grad is not None else torch.zeros_like(q))      # (every label None: no rels term)
    return loss.detach(), x.grad, d_rels, x2.detach()


def _top2_gap(v, dim):
    if v.shape[dim] < 2:
        return torch.full(v.shape[:dim] + v.shape[dim + 1:], float('inf'), dtype=v.dtype)
    t = torch.topk(v, 2, dim=dim)[0]
    return t.select(dim, 0) - t.select(dim, 1)


def restate(case: Case, inp, k=None):
    """Float64 restatement of the hinge terms (include/lirec_hip.h, lirec_margin_loss): the positive track and its top-two gap,
    the loss, and which gradient elements depend on a decision float32 may take the other way."""
    B, T, C, NR = case.B, case.T, case.C, case.NR
    idx = torch.arange(B)
    mem = inp['mem'].double()
    y, gt = inp['y'].long(), inp['gt'].long()
    x = inp['ints'].double().masked_fill((mem == 0).unsqueeze(2), float('-inf'))
    s = torch.sigmoid(x)
    score = s[idx, :, y]
    if case.rels:
        r = inp['r'].long()
        valid = (mem != 0) & (r != NR)
        q = torch.cat([torch.sigmoid(inp['rels'].double()) * valid.unsqueeze(2), torch.zeros(B, T, 1, dtype=torch.float64)], 2)
        r0, r1 = r[idx, gt[:, 0]], r[idx, gt[:, 1]]
        score = score + q[idx, :, r0]
    score = score * mem
    k_arg = torch.argmax(score, dim=1)
    if k is None:
        k = torch.zeros(B, dtype=torch.long) if case.tr_correct else k_arg
    k = torch.as_tensor(k).long()
    pos = s[idx, k, y]
    mi = ((mem != 0).unsqueeze(2) & (inp['w'] != 0).unsqueeze(1)).clone()
    if case.tr_correct:
        mi[idx, gt[:, 0], y] = False
        mi[idx, gt[:, 1], y] = False
    else:
        mi[idx, :, y] = False
    out = dict(k=k, k_arg=k_arg, gap=_top2_gap(score, 1))
    ex_i = torch.zeros(B, T, C, dtype=torch.bool)

    def part(sg, p, mask, ex, cols):
        """(per-clip loss, elements left out) of one head: sg [B,T,n] sigmoids, p [B] positive score, mask [B,T,n]"""
        if not case.max_neg:
            term = (MARGIN - p).view(B, 1, 1) + sg
            near = mask & (term.abs() <= HINGE_EPS)
            ex |= near
            ex[idx, k, cols] |= near.view(B, -1).any(1)
            return (torch.relu(term) * mask).sum((1, 2)), int(near.sum())
        best = (sg * mask).max(2)[0]
        term = (MARGIN - p).view(B, 1) + best
        near = term.abs() <= HINGE_EPS
        rows = near | ((best > 0) & (term > 0) & (_top2_gap(sg * mask, 2) < GAP_EPS))
        ex |= rows.unsqueeze(2)
        ex[idx, k, cols] |= near.any(1)
        return torch.relu(term).sum(1), int(rows.sum())

    li, n_i = part(s, pos, mi, ex_i, y)
    out.update(ex_ints=ex_i, near_ints=n_i)
    nvalid = B
    if case.rels:
        mr = torch.cat([valid.unsqueeze(2).expand(B, T, NR), torch.zeros(B, T, 1, dtype=torch.bool)], 2).clone()
        if case.tr_correct:
            mr.view(B * T, NR + 1)[torch.arange(B * T), r.view(-1)] = False
        else:
            mr[idx, :, r0] = False
            mr[idx, :, r1] = False
        ex_r = torch.zeros(B, T, NR + 1, dtype=torch.bool)
        lr, n_r = part(q, q[idx, k, r0], mr, ex_r, r0)
        out.update(ex_rels=ex_r[:, :, :NR], near_rels=n_r)
        if case.form == 'mtmm':
            nvalid = int((r[:, 0] != NR).sum())
            lr = lr * (r[:, 0] != NR)
    loss = case.lym * li.sum() / B
    if case.rels and nvalid:
        loss = loss + lr.sum() / nvalid
    out.update(loss=loss, nvalid=nvalid)
    # share left out: gradient elements (sum variant) or gradient rows (max variant), both heads together
    if case.max_neg:
        n_ex = int(ex_i.any(2).sum()) + (int(out['ex_rels'].any(2).sum()) if case.rels else 0)
        out['share'] = n_ex / (B * T * (2 if case.rels else 1))
    else:
        n_ex = int(ex_i.sum()) + (int(out['ex_rels'].sum()) if case.rels else 0)
        out['share'] = n_ex / (B * T * (C + (NR if case.rels else 0)))
    return out


def caps_hold(case: Case, rs, forced=False):
    """The caps of the decisions that may flip: no clip's positive-track argmax within GAP_EPS (a wanted tie excepted, and not
    asked of a forced track), at most EXCL_CAP of the gradient left out."""
    if rs['share'] > EXCL_CAP:
        return False
    if forced or case.tr_correct or case.T == 1:
        return True
    gap = rs['gap'].clone()
    if case.tie_clip is not None:
        gap[case.tie_clip] = float('inf')
    return bool((gap >= GAP_EPS).all())


SAMPLE_SEED = 0x5eed00000007          # Philox key of the in-kernel draw (both halves of the key in use)


def probs64(case: Case, inp):
    """The distribution the positive track is drawn from (mlp/model.py:470, :540-542) in float64: softmax over the tracks of the
    -inf-masked logits of the label's column; with rels the mean of that and the same over the relationship logits of the
    ground-truth pair's label, NaN -> 0 (a pair labelled None leaves no track to normalise over)."""
    B, NR = case.B, case.NR
    idx = torch.arange(B)
    mem = inp['mem'].double()
    x = inp['ints'].double().masked_fill((mem == 0).unsqueeze(2), float('-inf'))
    p = torch.softmax(x[idx, :, inp['y'].long()], dim=1)
    if case.rels:
        r, gt = inp['r'].long(), inp['gt'].long()
        valid = (mem != 0) & (r != NR)
        z = torch.cat([inp['rels'].double(), torch.zeros(B, case.T, 1, dtype=torch.float64)], 2)
        z = z.masked_fill(~valid.unsqueeze(2), float('-inf'))
        z[:, :, NR] = float('-inf')
        pr = torch.softmax(z[idx, :, r[idx, gt[:, 0]]], dim=1)
        p = (p + torch.where(pr != pr, torch.zeros_like(pr), pr)) / 2
    return p


def positive(case: Case, inp, how):
    """The injected positive track of a case: None (the loss's own argmax / track 0), 'sel' / 'sel_mixed' (forced_tracks), or
    'sample' -- the oracle's sampler on the float64 probabilities (the GPU test uses the kernel's own probabilities; a pick that
    differs there is caught by its own check of the caps)."""
    if how is None:
        return None
    if how == 'sample':
        return O.PhiloxTrackSampler(SAMPLE_SEED)(probs64(case, inp))
    sel = forced_tracks(case, inp, mixed=how == 'sel_mixed')
    return torch.where(sel >= 0, sel, restate(case, inp)['k_arg'])


def seeded(case: Case, how=None):
    """The case with the first seed (from its own upward) whose float64 decisions stand clear of rounding: chosen from the float64
    restatement alone.  tests/test_host_losses.py asserts the caps for every seed that comes out of here."""
    for seed in range(case.seed, case.seed + 50):
        c = dataclasses.replace(case, seed=seed)
        inp = make_inputs(c)
        # (a fallback clip of 'sel_mixed' takes the argmax: the gap is asked of every clip there)
        if caps_hold(c, restate(c, inp, positive(c, inp, how)), forced=how in ('sel', 'sample')):
            return c
    raise AssertionError('no seed within 50 of %r keeps the float64 decisions clear of rounding' % (case,))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_losses.py
# ---------------------------------------------------------------------------------------------------------------------------
T_MAX = largest_T(lds_loss, 101, 15)              # 343


def _both(form, B, T, C, NR, **kw):
    return [Case(form, B, T, C, NR, max_neg=mx, **kw) for mx in (False, True)]


def _ends(T):
    """valid prefixes that end inside the first, the second and the last 64-lane step, and one clip with one valid track"""
    last = ((T - 1) // 64) * 64
    return tuple(min(T, n) for n in (1, min(T, 37), min(T, 64 + 9) if T > 64 else T, last + 1 if last else T, T))


FORMS = ([Case('mmce', 9, 1, 101, 15, seed=11), Case('mmce', 5, 1, 1000, 15, seed=12),
          Case('mtmm', 9, 1, 101, 15, seed=13), Case('mtmm', 7, 1, 101, 15, seed=14, r_mode='none'),
          Case('mtmm', 7, 1, 101, 15, seed=15, r_mode='one')]
         + _both('margin', 6, 20, 101, 15, seed=16) + _both('mtr', 16, 20, 101, 15, seed=17))

TRACKS = [c for T in (1, 2, 63, 64, 65, 128, 129) for c in _both('mtr', 6, T, 101, 15, seed=100 + T, ends=_ends(T))]
TRACKS += [c for T in (65, 129) for c in _both('margin', 5, T, 101, 15, seed=300 + T, ends=_ends(T))]
# LDS above 64 KB (T >= 138 at C = 101, NR = 15; T >= 17 at C = 1000)
BIG_LDS = [c for T in (200, T_MAX) for c in _both('mtr', 5, T, 101, 15, seed=100 + T, ends=_ends(T))]
BIG_LDS += _both('margin', 5, 200, 101, 15, seed=500, ends=_ends(200)) + _both('mtr', 3, 20, 1000, 40, seed=501)

CLASSES = [c for C_ in (1, 7, 64, 65, 257, 1000) for c in _both('mtr', 3, 7, C_, 15, seed=600 + C_)]
CLASSES += [c for NR_ in (1, 15, 40, 70) for c in _both('mtr', 4, 9, 33, NR_, seed=700 + NR_)]

POSITIVE = ([c for gm in ('rand', 'equal') for c in _both('mtr', 8, 20, 101, 15, seed=800, tr_correct=True, g_mode=gm)]
            + _both('margin', 6, 65, 101, 15, seed=801, tr_correct=True, g_mode='rand', ends=_ends(65))
            + _both('mtr', 5, 129, 101, 15, seed=802, tr_correct=True, g_mode='rand', ends=_ends(129)))

OPTIONAL = [c for mn, wn in ((True, False), (False, True), (True, True))
            for c in _both('mtr', 6, 20, 101, 15, seed=900, mem_null=mn, w_null=wn) + _both('margin', 4, 65, 33, 5, seed=901, mem_null=mn, w_null=wn)]

SEL_CASES = _both('mtr', 8, 20, 101, 15, seed=1000) + _both('mtr', 5, 129, 101, 15, seed=1001, ends=_ends(129)) + \
    _both('margin', 6, 65, 101, 15, seed=1002, ends=_ends(65))

STRIDES = _both('mtr', 6, 20, 101, 15, seed=1100) + _both('mtr', 4, 65, 33, 5, seed=1101, ends=_ends(65)) + \
    [Case('mtmm', 9, 1, 101, 15, seed=1102)]

DTYPES = _both('mtr', 6, 65, 101, 15, seed=1200, ends=_ends(65)) + [Case('mtmm', 9, 1, 101, 15, seed=1201)]

DIVISORS = [Case('mtmm', 9, 1, 101, 15, seed=1300), Case('mtmm', 7, 1, 101, 15, seed=1301, r_mode='one')] + \
    _both('mtr', 6, 20, 101, 15, seed=1302) + _both('margin', 4, 65, 33, 5, seed=1303)

TIES = _both('mtr', 4, 65, 33, 5, seed=1400, tie_clip=1) + _both('margin', 4, 130, 17, 5, seed=1401, tie_clip=2)

SAMPLER = [Case(f, 8, T, 101, 15, seed=1500 + T, ends=_ends(T), r0_none=(2,) if f == 'mtr' else ())
           for T in (20, 65, 200) for f in ('mtr', 'margin')]

FINALIZE = [Case('mtr', 16, 20, 101, 15, seed=1600), Case('mtr', 300, 3, 11, 5, seed=1601)]

FUSED = [(T, rels) for T in (65, 200) for rels in (True, False)]


def all_margin_cases():
    """(group, case, how) of every lirec_margin_loss case whose gradients are compared with float64 (``how``: see ``positive``)"""
    groups = (('forms', FORMS), ('tracks', TRACKS), ('big_lds', BIG_LDS), ('classes', CLASSES), ('positive', POSITIVE),
              ('optional', OPTIONAL), ('strides', STRIDES), ('dtypes', DTYPES), ('divisors', DIVISORS), ('ties', TIES),
              ('finalize', FINALIZE))
    out = [(g, c, None) for g, cs in groups for c in cs]
    out += [('sel', c, how) for c in SEL_CASES for how in ('sel', 'sel_mixed')]
    out += [('sampler', dataclasses.replace(c, max_neg=mx), 'sample') for c in SAMPLER for mx in (False, True)]
    return out


def forced_tracks(case: Case, inp, mixed=False):
    """sel for the forced-track cases: for every clip a valid track OTHER than the float64 argmax where the clip has one (else the
    argmax); ``mixed``: every second clip -1 (falls back to the argmax)."""
    rs = restate(case, inp)
    nv = inp['mem'].sum(1).long()
    sel = torch.where(nv > 1, (rs['k_arg'] + 1 + torch.arange(case.B) % 3) % nv.clamp(min=1), rs['k_arg'])
    sel = torch.where((sel == rs['k_arg']) & (nv > 1), (sel + 1) % nv, sel)
    if mixed:
        sel[1::2] = -1
    return sel


def case_id(c: Case):
    flags = ''.join(s for s, on in (('-max', c.max_neg), ('-trc', c.tr_correct), ('-nomem', c.mem_null), ('-now', c.w_null)) if on)
    extra = ''.join('-' + v for v, d in ((c.g_mode, 'zero'), (c.r_mode, 'rand')) if v != d)
    return '%s-B%d-T%d-C%d-NR%d%s%s' % (c.form, c.B, c.T, c.C, c.NR, flags, extra)
