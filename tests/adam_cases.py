"""Cases, yardsticks and bounds of the update side of the step (tests/test_gpu_optim.py, tests/test_host_optim.py) -- not a test
module.

The update (include/lirec_hip.h, "optimiser"): g' = g gs + wd p; m' = m + (1 - b1)(g' - m); v' = b2 v + (1 - b2) g'^2;
p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps).  Two restatements of it in numpy:

  ref64   the definition in float64 on the fp32 state, with the hyper-parameters as the float32 values the C ABI receives;
  ref32   the same update operation by operation in float32, in the order of the kernels' `adam1` / `adam4`
          (lirec_amd/csrc/gemm.hpp), the two bias-correction factors computed in double and cast as lirec_adam_step does.

Bounds on |kernel - ref64|, u = 2^-24, each plus one fp32 denormal:

  p   16 u (|p| + A)          A = step_size max(|m|, G) / denom     (denom: the float64 one)
  m   16 u max(|m|, G)        G = |g gs| + |wd p|
  v   16 u V                  V = b2 v + (1 - b2) G^2

The update is a dozen roundings.  G, not |g gs + wd p|: the sum may cancel, and what the roundings of its two terms leave behind
is relative to the terms.  16 is margin, not a measurement; tests/test_host_optim.py asserts that ref32 -- a correct fp32
implementation by construction -- stays under HALF of every bound for every case here, so the bounds admit such an implementation
with room and nothing much wider.
"""
import dataclasses

import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32
DENORM = 2.0 ** -149                # one fp32 denormal
K = 16.0                            # the bounds' constant

# (lr, beta1, beta2, eps, weight_decay, grad_scale)
HYPERS = [(3e-5, .9, .999, 1e-8, 1e-5, 1.0),
          (1e-3, .9, .999, 1e-8, 0.0, 0.125),
          (1e-2, 0.0, .99, 1e-3, 1e-2, 1.0),
          (3e-5, .5, .9, 1e-8, 1e-5, 1.0 / 3.0)]
STEPS = [1, 2, 3, 1000, 100000]
MAGS = [1.0, 1e-3, 1e-12, 1e3]      # the gradients' magnitude (and, after step 1, the moments')

SWEEP = 2048 * 256 * 4              # elements one sweep of adam_kernel's grid covers (the launch is capped at 2048 workgroups)
N_BIG = 2 * SWEEP + 3 * 1024 + 3    # two full sweeps, a partial third, a scalar tail of three
SIZES = [1, 3, 4, 5, 1023, N_BIG]
N_HOST = 20011                      # what the host file draws per case (odd: a scalar tail)


@dataclasses.dataclass(frozen=True)
class Case:
    hyper: int
    step: int
    mag: float

    @property
    def seed(self):
        return 1000 * self.hyper + 10 * STEPS.index(self.step) + MAGS.index(self.mag) + 12345

    @property
    def id(self):
        return 'h%d-t%d-g%g' % (self.hyper, self.step, self.mag)


def _cases():
    out = []
    for h in range(len(HYPERS)):
        for i, t in enumerate(STEPS):                         # every hyper-parameter set at every step, the magnitudes cycling
            out.append(Case(h, t, MAGS[(h + i) % len(MAGS)]))
        for j, g in enumerate(MAGS):                          # ... and at every magnitude, the steps cycling
            out.append(Case(h, STEPS[(h + 2 * j + 1) % len(STEPS)], g))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c); uniq.append(c)
    return uniq


# the cases run at N_BIG: one per hyper-parameter set, the steps and magnitudes all different
BIG_CASES = [Case(0, 3, 1.0), Case(1, 1, 1e-3), Case(2, 1000, 1e-12), Case(3, 100000, 1e3)]
CASES = _cases()
CASES += [c for c in BIG_CASES if c not in CASES]


def hyper32(h):
    """the hyper-parameters as the float32 values the ABI receives, as Python floats"""
    return tuple(float(np.float32(x)) for x in (HYPERS[h] if isinstance(h, int) else h))


def make_state(case, n, offset=0):
    """fp32 (p, g, m, v) of n elements, fixed by the case (and `offset`, for a second draw): p ~ 0.1 N(0,1), g ~ mag N(0,1); the
    moments zero at step 1, m ~ 0.3 mag N(0,1) and v ~ mag^2 U(0,1) after it.  Every 5th / 7th / 11th / 13th element of
    v / m / g / p is exactly zero (the last of each run, so that a single element is not all zeros)."""
    r = np.random.default_rng(case.seed + 7919 * offset)
    p = (0.1 * r.standard_normal(n)).astype(np.float32)
    g = (case.mag * r.standard_normal(n)).astype(np.float32)
    if case.step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (0.3 * case.mag * r.standard_normal(n)).astype(np.float32)
        v = (case.mag ** 2 * r.random(n)).astype(np.float32)
    i = np.arange(n)
    v[i % 5 == 4] = 0; m[i % 7 == 6] = 0; g[i % 11 == 10] = 0; p[i % 13 == 12] = 0
    return p, g, m, v


def bias_corrections(step, hyper):
    """(step_size, bc2_sqrt) in float64 from the float32 hyper-parameters"""
    lr, b1, b2 = hyper[0], hyper[1], hyper[2]
    return lr / (1.0 - b1 ** float(step)), float(np.sqrt(1.0 - b2 ** float(step)))


def _xp(a):
    """numpy, or torch for a tensor (the same float64 arithmetic on the device, for buffers of millions of elements)"""
    if isinstance(a, np.ndarray):
        return np, (lambda t: np.asarray(t, np.float64))
    import torch
    return torch, (lambda t: t.double())


def ref64(p, g, m, v, step, hyper):
    """(p', m', v', G, A, V) in float64.  `hyper`: six Python floats that are float32 values (hyper32).  The state: fp32 numpy
    arrays, or torch tensors (the result is then on their device)."""
    lr, b1, b2, eps, wd, gs = hyper
    assert all(float(np.float32(x)) == x for x in hyper), 'ref64 wants the float32 hyper-parameters'
    xp, f64 = _xp(p)
    p, g, m, v = (f64(a) for a in (p, g, m, v))
    step_size, bc2_sqrt = bias_corrections(step, hyper)
    gg = g * gs + wd * p
    mn = m + (1.0 - b1) * (gg - m)
    vn = b2 * v + (1.0 - b2) * gg * gg
    denom = xp.sqrt(vn) / bc2_sqrt + eps
    pn = p - step_size * mn / denom
    G = xp.abs(g * gs) + xp.abs(wd * p)
    A = step_size * xp.maximum(xp.abs(m), G) / denom
    V = b2 * v + (1.0 - b2) * G * G
    return pn, mn, vn, G, A, V


def ref32(p, g, m, v, step, hyper):
    """(p', m', v') in float32, operation by operation in the kernels' order (adam1 / adam4: no contraction)"""
    f = np.float32
    lr, b1, b2, eps, wd, gs = (f(x) for x in hyper)
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    ss, bc = bias_corrections(step, hyper)
    step_size, bc2_sqrt = f(ss), f(bc)
    one = f(1.0)
    with np.errstate(all='ignore'):
        gg = g * gs + wd * p
        mn = m + (one - b1) * (gg - m)
        vn = v * b2 + ((one - b2) * gg) * gg
        denom = np.sqrt(vn) / bc2_sqrt + eps
        pn = p - step_size * (mn / denom)
    assert pn.dtype == f and mn.dtype == f and vn.dtype == f
    return pn, mn, vn


def bounds(p, m, G, A, V):
    """(bound on p', on m', on v') against ref64, float64"""
    xp, f64 = _xp(p)
    p, m = xp.abs(f64(p)), xp.abs(f64(m))
    return K * U * (p + A) + DENORM, K * U * xp.maximum(m, G) + DENORM, K * U * V + DENORM


def use_of_bounds(got, p, g, m, v, step, hyper):
    """[worst |got - ref64| / bound for p', m', v'] of a result (three fp32 arrays) on the state it was computed from"""
    xp, f64 = _xp(p)
    pn, mn, vn, G, A, V = ref64(p, g, m, v, step, hyper)
    bp, bm, bv = bounds(p, m, G, A, V)
    return [float((xp.abs(f64(x) - r) / b).max()) if len(r) else 0.0 for x, r, b in zip(got, (pn, mn, vn), (bp, bm, bv))]


def minus_ref(lo, hi, skip):
    """[lo, hi) without the ranges of `skip`, by set difference: the maximal runs of what is left, ascending"""
    left = set(range(lo, hi))
    for a, b in skip:
        left -= set(range(a, b))
    out, run = [], None
    for x in sorted(left):
        if run is not None and x == run[1]:
            run[1] = x + 1
        else:
            run = [x, x + 1]
            out.append(run)
    return [tuple(r) for r in out]
