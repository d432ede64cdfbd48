"""Cases and yardsticks of the decoupled-weight-decay (AdamW) tests (tests/test_host_adamw.py, tests/test_gpu_adamw.py) -- not a
test module.

The decoupled update (include/lirec_hip.h, "DECOUPLED WEIGHT DECAY"), for a group whose row of the table has the flag set:

    d  = (float)(1.0 - (double)lr * (double)wd)             once per range / launch, in double like the bias corrections
    g' = g gs                                               (gs: grad_scale, times the clip coefficient; NO wd term)
    m' = m + (1 - b1)(g' - m);  v' = v b2 + ((1 - b2) g') g'
    p' = p d - step_size (m' / (sqrt(v') / bc2_sqrt + eps))

torch's single-tensor order: param.mul_(1 - lr wd), the moments, addcdiv_.  Two restatements, in the style of adam_cases:

  ref64w   the definition in float64 (p (1 - lr wd), no intermediate rounding of the factor) on the fp32 state and the float32
           hyper-parameters: tests/test_host_adamw.py shows it equal to torch.optim.AdamW and
           torch.optim.Adam(decoupled_weight_decay=True) in float64;
  ref32w   operation by operation in float32 in the order of `adam1<true>` / `adam4<true>` (lirec_amd/csrc/gemm.hpp).

Bounds: adam_cases.bounds with G = |g gs| -- the project's own 16 u rule; the decay is one more rounding relative to |p| (two,
with the factor's own), which the |p| term of the bound on p' covers.

Rows (lr, beta1, beta2, eps, weight_decay): three whose decay is visible in fp32 (lr wd >= 1e-5) and one where it is not
(3e-5 x 1e-5 < 2^-25: d == 1.0f, the update has the bits of wd = 0).

The grouped forms take ranges (offset, length, lag, group) as group_cases does, rows of FIVE values and one flag per group: a
group with flag 0 is adam_cases' coupled update, a launch may mix the two."""
import numpy as np

import adam_cases as AC
import clip_cases as CC
import group_cases as GC

ROWS_W = [(1e-3, .9, .999, 1e-8, 1e-2), (1e-2, 0.0, .99, 1e-3, 1e-1), (3e-4, .5, .9, 1e-8, 5e-2)]
ROW_INVISIBLE = (3e-5, .9, .999, 1e-8, 1e-5)
ROW_COUPLED = GC.ROWS[2]                       # (1e-2, 0, .99, 1e-3, 1e-2): a coupled group whose decay is visible too

# the tables of the kernel cases: groups 0 and 2 decoupled, group 1 coupled
TABLES = {'A': ([ROWS_W[0], ROW_COUPLED, ROWS_W[2]], [True, False, True]),
          'B': ([ROWS_W[1], ROW_COUPLED, ROW_INVISIBLE], [True, False, True])}


def rows6(rows, flags):
    """the rows as ops.adam_hyper_write takes them with the flag: (lr, beta1, beta2, eps, weight_decay, decoupled)"""
    return [tuple(r[:5]) + (bool(f),) for r, f in zip(rows, flags)]


def decay32(hyper):
    """d as the kernels form it: the float32 lr and wd multiplied in double, 1 - that, rounded to float32"""
    return np.float32(1.0 - float(np.float32(hyper[0])) * float(np.float32(hyper[4])))


def ref64w(p, g, m, v, step, hyper):
    """(p', m', v', G, A, V) in float64; `hyper`: six float32 values as Python floats (adam_cases.hyper32); numpy or torch"""
    lr, b1, b2, eps, wd, gs = hyper
    assert all(float(np.float32(x)) == x for x in hyper), 'ref64w wants the float32 hyper-parameters'
    xp, f64 = AC._xp(p)
    p, g, m, v = (f64(a) for a in (p, g, m, v))
    step_size, bc2_sqrt = AC.bias_corrections(step, hyper)
    gg = g * gs
    mn = m + (1.0 - b1) * (gg - m)
    vn = b2 * v + (1.0 - b2) * gg * gg
    denom = xp.sqrt(vn) / bc2_sqrt + eps
    pn = p * (1.0 - lr * wd) - step_size * mn / denom
    G = xp.abs(gg)
    A = step_size * xp.maximum(xp.abs(m), G) / denom
    V = b2 * v + (1.0 - b2) * G * G
    return pn, mn, vn, G, A, V


def ref32w(p, g, m, v, step, hyper):
    """(p', m', v') in float32, operation by operation in the kernels' order (no contraction); numpy (IEEE division and square
    root, as the kernels' -- a device library's own need not be), fast enough for the 4 M elements of adam_cases.N_BIG"""
    f = np.float32
    lr, b1, b2, eps, wd, gs = (f(x) for x in hyper)
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    ss, bc = AC.bias_corrections(step, hyper)
    step_size, bc2_sqrt, d, one = f(ss), f(bc), decay32(hyper), f(1.0)
    with np.errstate(all='ignore'):
        gg = g * gs
        mn = m + (one - b1) * (gg - m)
        vn = v * b2 + ((one - b2) * gg) * gg
        denom = np.sqrt(vn) / bc2_sqrt + eps
        pn = p * d - step_size * (mn / denom)
    assert pn.dtype == f and mn.dtype == f and vn.dtype == f
    return pn, mn, vn


def ref64(p, g, m, v, rs, step, rows, flags, grad_scale, coef=1.0):
    """group_cases.ref64 with a flag per group: (p', m', v', bound_p, bound_m, bound_v) over the buffers' length"""
    f = lambda a: np.asarray(a, np.float64).copy()
    pn, mn, vn = f(p), f(m), f(v)
    bp, bm, bv = (np.zeros(len(pn)) for _ in range(3))
    for o, k, lag, grp in rs:
        sl = slice(o, o + k)
        gg = g[sl] if coef == 1.0 else CC.scaled_g(np.asarray(g[sl]), coef)
        fn = ref64w if flags[grp] else AC.ref64
        a, b_, c, G, A, V = fn(p[sl], gg, m[sl], v[sl], GC.effective_step(step, lag), GC.hyper_of(rows[grp][:5], grad_scale))
        pn[sl], mn[sl], vn[sl] = a, b_, c
        bp[sl], bm[sl], bv[sl] = AC.bounds(p[sl], m[sl], G, A, V)
    return pn, mn, vn, bp, bm, bv


def ref32(p, g, m, v, rs, step, rows, flags, grad_scale, coef=1.0):
    """the fp32 restatement range by range (the scale gs32 * coef32 rounded to fp32 once, as the clipped kernels form it)"""
    pn, mn, vn = (np.asarray(a, np.float32).copy() for a in (p, m, v))
    for o, k, lag, grp in rs:
        sl = slice(o, o + k)
        h = list(GC.hyper_of(rows[grp][:5], grad_scale))
        if coef != 1.0:
            h[5] = float(np.float32(h[5]) * np.float32(coef))
        fn = ref32w if flags[grp] else AC.ref32
        a, b_, c = fn(p[sl], g[sl], m[sl], v[sl], GC.effective_step(step, lag), tuple(h))
        pn[sl], mn[sl], vn[sl] = a, b_, c
    return pn, mn, vn


def use_of_bounds(got, p, g, m, v, rs, step, rows, flags, grad_scale, coef=1.0):
    """[worst |got - ref64| / bound for p', m', v'] over the elements of the ranges"""
    ref = ref64(p, g, m, v, rs, step, rows, flags, grad_scale, coef)
    mask = GC.inside(rs, len(ref[0]))
    return [float((np.abs(np.asarray(x, np.float64) - r)[mask] / b[mask]).max()) for x, r, b in zip(got, ref[:3], ref[3:])]


# -- FusedAdam: the two groups of the issue -- the weights decay (decoupled, 1e-2), the biases do not ---------------------------
LR = 1e-3


def two_groups(model, lr_bias=None):
    names = [n for n, _ in model.named_parameters()]
    w, b = [n for n in names if not n.endswith('.bias')], [n for n in names if n.endswith('.bias')]
    assert w and b
    bias = dict(params=b, weight_decay=0.0)
    if lr_bias is not None:
        bias['lr'] = lr_bias
    return [dict(params=w, weight_decay=1e-2, decoupled_weight_decay=True), bias]


def rows_of(optim):
    """(lr, beta1, beta2, eps, weight_decay, decoupled) of every group of an optimiser, as param_groups has them"""
    return [(g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], bool(g.get('decoupled_weight_decay', False)))
            for g in optim.param_groups]
