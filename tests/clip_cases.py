"""Yardsticks of the gradient-clipping tests (tests/test_host_clip.py, tests/test_gpu_clip.py) -- not a test module.

The clipped update is adam_cases' update with the scale gs * coef in place of gs, where coef is the fp32 clip coefficient a
device word holds (include/lirec_hip.h, lirec_set_adam_clip).  The kernels form that product ONCE, in fp32, and then multiply
every gradient by it: `ref32` restates exactly that, `ref64` is the definition in float64 with the exact product.
"""
import math

import numpy as np

import adam_cases as AC

P = 1024                                        # LIREC_CLIP_PARTIALS
COEFS = [1.0, 0.37, 1e-3]                       # (as the float32 values a device word can hold: coef32)
DROPPED_COEFS = [2.0 ** -20]                    # outside adam_cases.bounds for one case: tests/test_host_clip.py says why


def coef32(c):
    return float(np.float32(c))


def ref32(p, g, m, v, step, hyper, coef):
    """(p', m', v') in float32 as the clipped kernels compute them: the scale gs32 * coef32 rounded to fp32, then adam1 / adam4"""
    h = list(hyper)
    h[5] = float(np.float32(hyper[5]) * np.float32(coef))
    return AC.ref32(p, g, m, v, step, tuple(h))


def scaled_g(g, coef):
    """the gradients times the fp32 coefficient, in float64 (exact: 24 x 24 bits) -- with them adam_cases.ref64 / use_of_bounds
    are the clipped update's definition and bounds, scale gs * coef"""
    if isinstance(g, np.ndarray):
        return g.astype(np.float64) * coef32(coef)
    return g.double() * coef32(coef)


def use_of_bounds(got, p, g, m, v, step, hyper, coef):
    return AC.use_of_bounds(got, p, scaled_g(g, coef), m, v, step, hyper)


def norm_over(values, ranges):
    """sqrt of the exactly summed squares (math.fsum of float64 squares) of `values` over `ranges` = [(start, end), ...]"""
    return math.sqrt(sq_over(values, ranges))


def sq_over(values, ranges):
    v = np.asarray(values, np.float64)
    return math.fsum(float(x) for a, b in ranges for x in v[a:b] * v[a:b])


def coef_of(sq, grad_scale, max_norm):
    """(coef, norm) as float32 from a float64 sum of squares: lirec_clip_finalize's arithmetic in numpy float64"""
    with np.errstate(all='ignore'):
        norm = np.sqrt(np.float64(sq)) * np.float64(np.float32(grad_scale))
        x = np.float64(np.float32(max_norm)) / (norm + np.float64(1e-6))
    coef = x if x < 1.0 else (x if np.isnan(x) else np.float64(1.0))
    return np.float32(coef), np.float32(norm)
