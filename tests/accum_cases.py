"""Yardsticks of gradient accumulation (FusedAdam(accumulate_steps=k); tests/test_host_accum.py, tests/test_gpu_accum.py) -- not a
test module.

THE WINDOW.  k micro-batch gradients g_1 .. g_k are added into the flat gradient buffer and the k-th ``step()`` is one ordinary
Adam update on their sum times grad_scale / k.  The float64 restatement: s = sum of the g_i in double, the scale
gs_k = (float)((double)(float)grad_scale / k) -- what ``ops.accum_scale`` and the launches under lirec_set_adam_hold compute --, then
adam_cases.ref64 on (p, s, m, v) with gs_k in the place of grad_scale.

THE BOUND.  The device adds the micro-batch gradients in fp32, one after the other: fl(fl(g_1 + g_2) + g_3) ...  For k terms
that is k - 1 roundings, each at most u times the partial sum it rounds, which is at most S = sum |g_i| (to first order in u; the
exact constant is gamma_{k-1} = (k-1)u / (1 - (k-1)u), and the 16 of adam_cases.bounds is margin over far more than that
difference).  So the gradient the update sees differs from the float64 sum by at most (k - 1) u S per element, and what enters
the update, gg = g gs_k + wd p, by at most

    d = gs_k (k - 1) u S.

Pushed through the update's definition, term by term (every factor at its float64 value):

    m' = m + (1 - b1)(gg - m)                 |dm|     <= (1 - b1) d
    v' = b2 v + (1 - b2) gg^2                 |dv|     <= (1 - b2)(2 |gg| d + d^2)
    sqrt(v')                                  |dsqrt|  <= max(sqrt(v' + dv) - sqrt(v'), sqrt(v') - sqrt(max(v' - dv, 0)))
    denom = sqrt(v') / bc2 + eps              |ddenom| <= dsqrt / bc2, and denom - ddenom >= eps
    p' = p - ss m' / denom                    |dp|     <= ss (dm / low + |m'| ddenom / (denom low)),  low = max(denom - ddenom, eps)

The kernel's own roundings are what adam_cases.bounds cover, on the state and the gradient it is handed; so

    |kernel - ref64(window)| <= adam_cases.bounds(...) + (dp, dm, dv)

with G, A, V of the bounds taken at the float64 sum.  k = 1 adds nothing: the widening is zero and the bound is adam_cases'.
tests/test_host_accum.py shows the fp32 restatement -- ref32 on the sequential fp32 sum -- inside it for every case.

THE PHASE.  ``phase`` = micro-batches already in the open window; the n-th call of ``step()`` in a run with constant k finds
phase (n - 1) mod k, applies when that is k - 1, and the ``zero_grad()`` in front of it zeroes when it is 0.
"""
import numpy as np

import adam_cases as AC

U = AC.U


def accum_scale(grad_scale, k):
    """(float)((double)(float)grad_scale / k) as a Python float"""
    return float(np.float32(np.float64(np.float32(grad_scale)) / k))


def window_hyper(hyper, k):
    """the six float32 hyper-parameters with grad_scale over k"""
    h = AC.hyper32(hyper)
    return h[:5] + (accum_scale(h[5], k),)


def micro_grads(case, n, k):
    """k gradient arrays of the case's magnitude, all different (the case's own draw first)"""
    return [AC.make_state(case, n, offset=i)[1] for i in range(k)]


def sum64(grads):
    xp, f64 = AC._xp(grads[0])
    s = f64(grads[0])
    for g in grads[1:]:
        s = s + f64(g)
    return s


def sum32(grads):
    """the buffer after k accumulating backwards: sequential fp32 additions onto zeros"""
    s = np.zeros_like(np.asarray(grads[0], np.float32))
    for g in grads:
        s = (s + np.asarray(g, np.float32)).astype(np.float32)
    return s


def abs_sum64(grads):
    xp, f64 = AC._xp(grads[0])
    s = xp.abs(f64(grads[0]))
    for g in grads[1:]:
        s = s + xp.abs(f64(g))
    return s


def ref64_window(p, grads, m, v, step, hyper, k=None):
    """((p', m', v') of the float64 restatement, (bound on p', m', v')) of the window ``grads`` -- k = len(grads) micro-batch
    gradients unless given -- on the fp32 state; ``hyper``: the six hyper-parameters with the optimiser's own grad_scale"""
    k = len(grads) if k is None else k
    hk = window_hyper(hyper, k)
    lr, b1, b2, eps, wd, gsk = hk
    xp, f64 = AC._xp(p)
    s, S = sum64(grads), abs_sum64(grads)
    pn, mn, vn, G, A, V = AC.ref64(p, s, m, v, step, hk)
    bp, bm, bv = AC.bounds(p, m, G, A, V)
    d = gsk * (len(grads) - 1) * U * S
    gg = xp.abs(s * gsk + wd * f64(p))
    ss, bc2 = AC.bias_corrections(step, hk)
    dm = (1.0 - b1) * d
    dv = (1.0 - b2) * (2.0 * gg * d + d * d)
    zero = vn * 0.0
    dsqrt = xp.maximum(xp.sqrt(vn + dv) - xp.sqrt(vn), xp.sqrt(vn) - xp.sqrt(xp.maximum(vn - dv, zero)))
    denom = xp.sqrt(vn) / bc2 + eps
    dd = dsqrt / bc2
    low = xp.maximum(denom - dd, zero + eps) if eps > 0 else denom - dd
    dp = ss * (dm / low + xp.abs(mn) * dd / (denom * low))
    return (pn, mn, vn), (bp + dp, bm + dm, bv + dv)


def use_of_window_bounds(got, p, grads, m, v, step, hyper, k=None):
    """[worst |got - restatement| / bound for p', m', v']"""
    xp, f64 = AC._xp(p)
    ref, bnd = ref64_window(p, grads, m, v, step, hyper, k)
    return [float((xp.abs(f64(x) - r) / b).max()) if len(r) else 0.0 for x, r, b in zip(got, ref, bnd)]


# ---------------------------------------------------------------------------------------------------------------------------
# the phase, restated from the number of calls
# ---------------------------------------------------------------------------------------------------------------------------
def chain(ks):
    """``ks``: the value of accumulate_steps at each call of step() (it may change only where a window has just closed).  Returns
    per call (phase found, zero_grad in front zeroes?, applies?, updates applied after the call) by counting micro-batches."""
    out, in_window, updates = [], 0, 0
    for k in ks:
        phase = in_window
        in_window += 1
        applies = in_window == k
        if applies:
            in_window, updates = 0, updates + 1
        out.append((phase, phase == 0, applies, updates))
    return out


def head_chain(k, calls, phase0=0, ctr0=(0, 0, 0), every=(1, 0, 0), apply=(0, 1, 1)):
    """the window block and the counters after each of ``calls`` head launches (lirec_accum_begin) from phase ``phase0``: per call
    (zeroed?, hold flag, phase after, counters after)"""
    out, phase, ctr = [], phase0, list(ctr0)
    for _ in range(calls):
        zeroed = phase == 0
        applies = phase + 1 >= k
        ctr = [c + e + (a if applies else 0) for c, e, a in zip(ctr, every, apply)]
        phase = 0 if applies else phase + 1
        out.append((zeroed, 0 if applies else 1, phase, tuple(ctr)))
    return out
