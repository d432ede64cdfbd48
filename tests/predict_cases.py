"""Inputs and expected sides for lirec_predict_clips (include/lirec_hip.h) -- shared by tests/test_host_predict.py and
tests/test_gpu_predict.py; not a test module.

Two generators.  MARGIN-SAFE: random logits, redrawn per clip until the best and the second-best value of the fp64 joint score
differ by more than 1e-5 (far above what two float sigmoid implementations can disagree by, 2^-23 per term) and no two logits
of a row are equal -- the integer outputs then do not depend on the sigmoid's last bit.  EXACT-TIE: logits drawn from
{-2, 0.5, 1, 3}.  Equal logits give equal probabilities under any sigmoid, S(a) + Q(b) and S(b) + Q(a) are the same double, and
the sums of DISTINCT value multisets (pairs, single values beside the "None" column's 0, and the 0 + 0 of a padded track) are at
least 1.06e-2 apart under the three sigmoid implementations below (tests/test_host_predict.py checks it): those are the only
ties, and every implementation has them -- the first-index rule decides, and it is exact.
"""
import numpy as np
from scipy.special import expit

import topk_cases as TC
from lirec_amd.metrics import joint_predictions, top_lists

TIE_VALUES = np.array([-2.0, 0.5, 1.0, 3.0], dtype=np.float32)
MARGIN = 1e-5


def _f32_formula(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over='ignore'):
        return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


# float32 in, float32 out: scipy's float32 expit; 1 / (1 + exp(-x)) evaluated in float32; the float64 sigmoid rounded to float32
SIGMOIDS = {
    'expit_f32': lambda x: expit(np.asarray(x, dtype=np.float32)),
    'formula_f32': _f32_formula,
    'f64_rounded': lambda x: expit(np.asarray(x, dtype=np.float64)).astype(np.float32),
}


def masked(ints, rels, mem):
    """copies of the logits with the padded tracks at -inf (float32)"""
    ints = np.array(ints, dtype=np.float32)
    rels = np.array(rels, dtype=np.float32) if rels is not None else None
    if mem is not None:
        pad = np.asarray(mem) == 0
        ints[pad] = -np.inf
        if rels is not None:
            rels[pad] = -np.inf
    return ints, rels


def joint_under(sigmoid, ints, rels, mem):
    """(trk, cls, rel) by the rules of the header with ``sigmoid`` for the probabilities: sums in double, first flat argmax"""
    ints, rels = masked(ints, rels, mem)
    n, T, C = ints.shape
    pc = sigmoid(ints)
    assert pc.dtype == np.float32
    if rels is None:
        flat = np.argmax(pc.reshape(n, -1), axis=1)
        return flat // C, flat % C, np.full(n, -1)
    pr = np.concatenate((sigmoid(rels).astype(np.float64), np.zeros((n, T, 1))), axis=2)
    NR1 = pr.shape[2]
    flat = np.argmax((pc.astype(np.float64)[:, :, :, None] + pr[:, :, None, :]).reshape(n, -1), axis=1)
    return flat // (C * NR1), (flat % (C * NR1)) // NR1, flat % NR1


def sigmoids_agree(ints, rels, mem):
    """per clip: the three host sigmoids all give the same joint prediction"""
    preds = [joint_under(s, ints, rels, mem) for s in SIGMOIDS.values()]
    same = np.ones(len(ints), dtype=bool)
    for p in preds[1:]:
        for a, b in zip(preds[0], p):
            same &= a == b
    return same


def joint_margin(ints, rels, mem):
    """per clip, best minus second-best value of the joint score with fp64 sigmoids (inf for a single candidate)"""
    ints, rels = masked(ints, rels, mem)
    n = ints.shape[0]
    s = expit(ints.astype(np.float64))
    if rels is not None:
        q = np.concatenate((expit(rels.astype(np.float64)), np.zeros(rels.shape[:2] + (1,))), axis=2)
        s = s[:, :, :, None] + q[:, :, None, :]
    s = np.sort(s.reshape(n, -1), axis=1)
    return s[:, -1] - s[:, -2] if s.shape[1] > 1 else np.full(n, np.inf)


def random_mem(rng, B, T):
    """0/1 [B, T] float32, the valid tracks anywhere, at least one per clip"""
    mem = (rng.random((B, T)) < 0.7).astype(np.float32)
    mem[np.arange(B), rng.integers(0, T, size=B)] = 1
    return mem


def margin_case(seed, B, T, C, NR, mem='random', **kw):
    rng = np.random.default_rng(seed)
    m = random_mem(rng, B, T) if isinstance(mem, str) else mem
    ints = np.empty((B, T, C), dtype=np.float32)
    rels = np.empty((B, T, NR), dtype=np.float32) if NR else None
    for b in range(B):
        for _ in range(1000):
            x = (2.0 * rng.standard_normal((1, T, C))).astype(np.float32)
            r = (2.0 * rng.standard_normal((1, T, NR))).astype(np.float32) if NR else None
            mb = m[b:b + 1] if m is not None else None
            # (a clip without a valid track has one value everywhere: nothing to redraw for)
            if (mb is not None and not mb.any() or joint_margin(x, r, mb)[0] > MARGIN) and TC.tie_free(x[0]) and (r is None or NR < 2 or TC.tie_free(r[0])):
                break
        else:
            raise AssertionError('no margin-safe draw')
        ints[b] = x[0]
        if NR:
            rels[b] = r[0]
    return dict(ints=ints, rels=rels, mem=m, K=5, exact=False, **kw)


def tie_case(seed, B, T, C, NR, mem='random', **kw):
    rng = np.random.default_rng(seed)
    m = random_mem(rng, B, T) if isinstance(mem, str) else mem
    ints = TIE_VALUES[rng.integers(0, 4, size=(B, T, C))]
    rels = TIE_VALUES[rng.integers(0, 4, size=(B, T, NR))] if NR else None
    return dict(ints=ints, rels=rels, mem=m, K=5, exact=True, **kw)


def named_cases():
    """name -> dict(ints [B, T, C] f32, rels [B, T, NR] f32 or None, mem [B, T] f32 or None, K; optional: ld_ints, ld_rels,
    mem_f64 (hand ``mem`` over as float64 with loader_types))"""
    nan = np.float32('nan')
    cases = {
        'a': tie_case(1, 3, 1, 1, 0, mem=None),
        'b': tie_case(2, 9, 1, 2, 1, mem=None),
        'c': tie_case(3, 37, 7, 13, 5),
        'c_no_rels': tie_case(4, 37, 7, 13, 0),
        'd': margin_case(5, 5, 65, 3, 2),                              # the flat joint path above 64 tracks
        'd_ties': tie_case(6, 5, 65, 3, 2),
        'd_no_rels': margin_case(7, 5, 65, 3, 0),
        'e': margin_case(8, 3, 2, 300, 15),                            # more than one class per thread
        'e_ties': tie_case(9, 3, 2, 300, 15),
        'f': dict(margin_case(10, 6, 4, 3, 2), K=5),                   # K above C and NR: the -1 / 0 tail
        'f_K16': dict(tie_case(11, 6, 4, 3, 2), K=16),
        'f_K1': dict(margin_case(12, 6, 4, 3, 2), K=1),
        'g': margin_case(13, 9, 3, 13, 5, ld_ints=13 + 3, ld_rels=5 + 1),
        'h': margin_case(14, 9, 5, 11, 5, mem=None),
        'i': margin_case(15, 9, 5, 11, 5, mem_f64=True),
        'clip_level': margin_case(16, 70, 1, 101, 15, mem=None),       # T = 1, mem NULL: modalties / int_rels
        'clip_level_no_rels': margin_case(17, 70, 1, 101, 0, mem=None),
        'bench_shape': margin_case(18, 8, 16, 101, 15),
    }
    mem_j = random_mem(np.random.default_rng(19), 4, 5)
    mem_j[2] = 0                                                       # one clip with every track padded
    cases['j'] = margin_case(19, 4, 5, 11, 5, mem=mem_j)
    cases['j_no_rels'] = margin_case(22, 4, 5, 11, 0, mem=mem_j)
    k = margin_case(20, 4, 3, 13, 5, mem=np.array([[1, 1, 1], [1, 0, 1], [1, 0, 1], [0, 1, 1]], dtype=np.float32))
    k['ints'][1, 2, 4] = nan                                          # a NaN in an unmasked logit: flagged
    k['ints'][2, 1, 0] = nan                                           # NaNs in a padded row only: not flagged
    k['rels'][2, 1, 3] = nan
    cases['k'] = k
    k1 = margin_case(21, 4, 1, 11, 5, mem=None)                        # the clip-level form: the ranked row is the one with the NaNs
    k1['ints'][0, 0, [2, 7]] = nan
    k1['rels'][3, 0, 0] = nan
    cases['k_clip_level'] = k1
    return cases


def flags_of(ints, rels, mem):
    ints = np.asarray(ints)
    valid = np.ones(ints.shape[:2], dtype=bool) if mem is None else np.asarray(mem) != 0
    nan = (np.isnan(ints).any(axis=2) & valid).any(axis=1)
    if rels is not None:
        nan |= (np.isnan(np.asarray(rels)).any(axis=2) & valid).any(axis=1)
    return nan.astype(np.int32) | (2 * (~valid.any(axis=1))).astype(np.int32)


def expected(case, trk=None):
    """The host side of one case: the integer outputs by lirec_amd.metrics (joint_predictions / top_lists), the real-valued ones
    from fp64 sigmoids.  ``trk``: rank the rows of these tracks instead of the predicted ones (the NaN-flagged clips, whose joint
    prediction is not pinned)."""
    ints, rels = masked(case['ints'], case['rels'], case['mem'])
    B, T, C = ints.shape
    K = case['K']
    with np.errstate(invalid='ignore'):
        j_trk, j_cls, j_rel, _, _ = joint_predictions(ints.copy(), rels.copy() if rels is not None else None, None)
    rows = np.arange(B)
    s64 = expit(ints.astype(np.float64))
    exp = {'trk': j_trk.astype(np.int32), 'cls': j_cls.astype(np.int32), 'rel': j_rel.astype(np.int32),
           'flags': flags_of(case['ints'], case['rels'], case['mem'])}
    exp['trk_score'] = s64.max(axis=2)
    exp['score'] = s64[rows, j_trk, j_cls]
    if rels is not None:
        q64 = np.concatenate((expit(rels.astype(np.float64)), np.zeros((B, T, 1))), axis=2)
        exp['trk_score'] = exp['trk_score'] + q64.max(axis=2)
        exp['score'] = exp['score'] + q64[rows, j_trk, j_rel]
    at = j_trk if trk is None else np.where(exp['flags'] & 1, trk, j_trk)
    exp['top_cls'], _ = top_lists(ints[rows, at], K)
    exp['top_cls_p'] = _probs64(ints[rows, at], exp['top_cls'])
    if rels is not None:
        exp['top_rel'], _ = top_lists(rels[rows, at], K)
        exp['top_rel_p'] = _probs64(rels[rows, at], exp['top_rel'])
    return exp


def _probs64(x, idx):
    p = np.take_along_axis(expit(x.astype(np.float64)), np.maximum(idx, 0), axis=1)
    return np.where(idx < 0, 0.0, p)


def brute_force(ints, rels, mem):
    """(trk, cls, rel, score, trk_score) by a plain loop over (t, c, r): float32 expit, the sums as Python doubles, the first
    strictly larger value wins"""
    ints, rels = masked(ints, rels, mem)
    B, T, C = ints.shape
    NR = rels.shape[2] if rels is not None else 0
    out = [np.zeros(B, dtype=np.int64) for _ in range(3)] + [np.zeros(B), np.zeros((B, T))]
    S = expit(ints).tolist()                                             # float32 values as Python doubles
    Q = expit(rels).tolist() if rels is not None else None
    for b in range(B):
        best = None
        for t in range(T):
            tbest = None
            for c in range(C):
                s = S[b][t][c]
                for r in (range(NR + 1) if rels is not None else [-1]):
                    v = s + (0.0 if r == NR else Q[b][t][r]) if r >= 0 else s
                    if best is None or v > best[0]:
                        best = (v, t, c, r)
                    if tbest is None or v > tbest:
                        tbest = v
            out[4][b, t] = tbest
        out[3][b], out[0][b], out[1][b], out[2][b] = best
    return tuple(out)
