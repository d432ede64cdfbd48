"""The rank rule of lirec_eval_clip_topk (include/lirec_hip.h) restated in numpy WITHOUT a sort, the host side it is held to
(lirec_amd.metrics.Precision fed the stable descending order), and the adversarial rows -- shared by
tests/test_host_eval_topk.py and tests/test_gpu_eval_topk.py; not a test module."""
import numpy as np

from lirec_amd.metrics import Precision

COUNTERS = ('total', '_top1', '_top3', '_top5', '_top1_sf', '_top5_sf')


def ranks(x):
    """rank[b, c] = the number of classes that come before class c in row b: j is before c when x[j] > x[c], or x[j] == x[c]
    and j < c; a NaN after every number, among NaNs the lower index first."""
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape
    lower = np.arange(C)[:, None] < np.arange(C)[None, :]                  # [j, c]: j < c
    out = np.empty((B, C), dtype=np.int64)
    for lo in range(0, B, 64):
        xb = x[lo:lo + 64]
        nan = np.isnan(xb)
        xj, xc, nj, nc = xb[:, :, None], xb[:, None, :], nan[:, :, None], nan[:, None, :]
        with np.errstate(invalid='ignore'):
            numbers = (xj > xc) | ((xj == xc) & lower)                       # (false wherever a NaN takes part)
        before = numbers | (~nj & nc) | (nj & nc & lower)
        out[lo:lo + 64] = before.sum(1)
    return out


def rank_counters(x, y, soft=None, conf=None):
    """[total, top1, top3, top5, top1_sf, top5_sf] of one batch by the rank rule; ``conf[y, class of rank 0] += 1`` in place.
    A label outside [0, C) counts in total only."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y).reshape(-1).astype(np.int64)
    B, C = x.shape
    r = ranks(x)
    ok = (y >= 0) & (y < C)
    ry = np.where(ok, r[np.arange(B), np.where(ok, y, 0)], C + 5)
    c = [B, int((ry < 1).sum()), int((ry < 3).sum()), int((ry < 5).sum()), 0, 0]
    if conf is not None:
        np.add.at(conf, (y[ok], np.argmin(r, axis=1)[ok]), 1)
    if soft is not None:
        soft = np.asarray(soft, dtype=np.float64)
        for b in range(B):
            s = soft[b]
            with np.errstate(invalid='ignore'):
                s = s[(s >= 0) & (s < C) & (s == np.floor(s))].astype(np.int64)
            if len(s):
                best = int(r[b, s].min())
                c[4] += best == 0
                c[5] += best < 5
    return c


def stable_order(x):
    return np.argsort(-np.asarray(x, dtype=np.float32), axis=1, kind='stable')


def host_counters(x, y, soft=None, conf=None, prec=None):
    """The expected side: the host Precision (pinned to the reference by tests/golden) on the stable descending order.  Labels
    outside [0, C) are left out of the confusion matrix only (Precision would index it with them); they hit nothing."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y).reshape(-1).astype(np.int64)
    order = stable_order(x)
    p = prec if prec is not None else Precision(soft_gt=soft is not None)
    if soft is not None:
        p.update_probs(gt=y, pr_classes=order, soft_labels=np.asarray(soft))
    else:
        p.update_probs(gt=y, pr_classes=order)
    if conf is not None:
        ok = (y >= 0) & (y < x.shape[1])
        Precision().update_probs(gt=y[ok], pr_classes=order[ok], conf_mat=conf)
    return [int(getattr(p, k)) for k in COUNTERS]


def tie_free(x):
    """no two entries of a row compare equal and none is a NaN: every argsort agrees on such a row"""
    x = np.asarray(x, dtype=np.float32)
    s = np.sort(x, axis=1)
    return not np.isnan(x).any() and bool((s[:, 1:] != s[:, :-1]).all())


def adversarial(C=11):
    """(x [B, C] float32, y [B], soft [B, 4] float64): exact ties (at the top, at the top-5 boundary, the label tied with the
    winner), all-equal rows, NaN at the label, an all-NaN row, a -inf row, +-0, +-inf, labels of -1 and C, soft rows without a
    valid entry / with a duplicate / with the label / with a fraction, a NaN and an entry >= C."""
    assert C >= 8
    nan, inf = np.float32('nan'), np.float32('inf')
    base = np.linspace(-1.0, 1.0, C).astype(np.float32)                    # ascending: class C-1 wins, tie-free
    rows, ys, softs = [], [], []

    def add(x, y, soft=(-1, -1, -1, -1)):
        rows.append(np.asarray(x, dtype=np.float32)); ys.append(y); softs.append(np.asarray(soft, dtype=np.float64))
    add(base, C - 1, (C - 1, -1, -1, -1))                                  # plain hit, soft == label
    add(base, 0)                                                           # plain miss, no valid soft entry
    x = base.copy(); x[2] = x[C - 1]
    add(x, C - 1, (C - 1, C - 1, -1, -1))                                  # the label tied with the winner, label has the higher index
    add(x, 2, (2, -1, 2, -1))                                              # ... and the lower one; duplicate soft entries
    x = base.copy(); x[C - 6] = x[C - 5]
    add(x, C - 5, (C - 5, -1, -1, -1))                                     # a tie at the top-5 boundary: ranks 4 and 5
    add(x, C - 6, (C - 6, -1, -1, -1))
    x = base.copy(); x[C - 4] = x[C - 3]
    add(x, C - 3, (0.5, C - 3, -1, -1))                                    # a tie at the top-3 boundary; a fractional soft entry
    add(x, C - 4, (nan, C - 4, C, 1e9))                                    # NaN / out-of-range soft entries
    for y in (0, 4, 5, C - 1):
        add(np.zeros(C), y, (y, -1, -1, -1))                               # all equal: the order is the index order
    add(np.full(C, 3.25), 2, (7, 6, 5, -1))
    x = np.zeros(C); x[1::2] = -0.0
    add(x, 1, (1, -1, -1, -1))                                             # +-0 tie
    x = base.copy(); x[3] = 0.0; x[4] = -0.0; x[5:] = -1.0 - base[5:]
    add(x, 4, (4, 3, -1, -1))
    x = base.copy(); x[C - 1] = nan
    add(x, C - 1, (C - 1, -1, -1, -1))                                     # NaN at the label: it ranks last
    add(x, C - 2, (C - 2, -1, -1, -1))
    x = base.copy(); x[0] = nan; x[3] = nan
    add(x, 3, (0, 3, -1, -1))                                              # two NaNs: the lower index first
    add(np.full(C, nan), 0, (0, -1, -1, -1))                               # all NaN: index order
    add(np.full(C, nan), 6, (6, 5, -1, -1))
    add(np.full(C, -inf), 0, (4, -1, -1, -1))                              # a -inf row
    add(np.full(C, -inf), 5)
    x = base.copy(); x[1] = inf; x[2] = inf; x[0] = -inf
    add(x, 2, (2, 0, -1, -1))                                              # +inf twice, -inf once
    x = np.full(C, -inf); x[4] = nan
    add(x, 4, (4, -1, -1, -1))                                             # NaN under -inf
    add(base, -1, (C - 1, -1, -1, -1))                                     # labels outside [0, C): total only
    add(base, C, (-1, -1, -1, -1))
    add(base, -5)
    return np.stack(rows), np.asarray(ys, dtype=np.int64), np.stack(softs)


def random_case(seed, B, C, n_soft=3):
    """tie-free random rows (asserted by the callers), labels in range, soft rows padded with -1"""
    rng = np.random.default_rng(seed)
    # a permutation of 0..C-1 per row plus less than a quarter step of noise: distinct by construction (independent normal
    # float32 draws do collide now and then at 513 x 324), both signs
    x = rng.permuted(np.tile(np.arange(C, dtype=np.float64), (B, 1)), axis=1) + 0.25 * rng.random((B, C))
    x = ((x - 0.5 * C) * 0.01).astype(np.float32)
    y = rng.integers(0, C, size=B).astype(np.int64)
    soft = -np.ones((B, n_soft), dtype=np.float64)
    soft[:, 0] = rng.integers(0, C, size=B)
    two = rng.random(B) < 0.5
    soft[two, 1] = rng.integers(0, C, size=int(two.sum()))
    soft[rng.random(B) < 0.1] = -1
    return x, y, soft
