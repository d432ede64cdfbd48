"""The yardstick of lirec_param_stats (include/lirec_hip.h, "per-range gradient, weight and update statistics") -- not a test
module.  A float64 restatement in numpy of the nine columns of a row, with the sums formed EXACTLY:

  gradient / parameter columns   the square of an fp32 value is exact in float64, and ``math.fsum`` returns the correctly rounded sum
                                 of its arguments -- the exact sum of squares, rounded once;
  update columns                 u = (m inv_bc1) / (sqrt(v) inv_sqrt_bc2 + eps) is not exact in any format; the yardstick forms it and
                                 its square in the 64-bit-significand long double (errors of 2^-64 per operation, 2^-11 of one float64
                                 rounding), splits each square into two float64 (hi + lo, exact) and takes ``math.fsum`` of those.
                                 WHICH elements are finite is decided from the float64 evaluation, the format the kernel computes in.
  maxima, counts                 plain max and counts.

The bounds (``sum_bounds``), relative to the exact sum, u = 2^-53, n the range's length:
  gradient / parameter sums      n u.  The terms are exact and >= 0, so a sum of n of them in ANY order of float64 additions carries at
                                 most n - 1 roundings per term: (1 + u)^(n-1) - 1 <= n u for every n used here.
  update sums                    (n + 16) u, the issue's figure.  What the kernel's arithmetic needs is n + 10: u_i is five roundings
                                 (the product m inv_bc1; the root; its product with inv_sqrt_bc2; the sum with eps, whose error is at most
                                 the larger of its two non-negative terms'; the quotient), its square twice that plus the square's own
                                 rounding -- 11 per term -- and n - 1 additions.  The remaining 6 u cover the second-order terms
                                 and the yardstick's own 11 x 2^-64.
Norms are taken after the square root: half the relative bound of the sum, plus one float64 rounding (``norm_bound``)."""
import math

import numpy as np

U = 2.0 ** -53
COLS = 9
GRAD, PARAM, UPDATE = 1, 2, 4
FLT_MAX = float(np.finfo(np.float32).max)
DENORMAL = float(np.float32(1e-42))
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'the yardstick needs the 64-bit-significand long double'


def update_direction(m, v, inv_bc1, inv_sqrt_bc2, eps, dtype=np.float64):
    """u elementwise in ``dtype``, every operation rounded on its own; inv_bc1 / inv_sqrt_bc2 / eps are taken as the fp32 values an
    entry carries"""
    f = [dtype(float(np.float32(x))) for x in (inv_bc1, inv_sqrt_bc2, eps)]
    with np.errstate(all='ignore'):
        return (m.astype(dtype) * f[0]) / (np.sqrt(v.astype(dtype)) * f[1] + f[2])


def _group(x64, squares_hi_lo):
    """(exact sum of squares, max |x|, non-finite count) of one group; ``squares_hi_lo``: float64 arrays whose exact sum is wanted"""
    fin = np.isfinite(x64)
    total = math.fsum(np.concatenate([s[fin] for s in squares_hi_lo]).tolist())
    return [total, float(np.abs(x64[fin]).max()) if fin.any() else 0.0, float((~fin).sum())]


def row(p, g, m, v, entry):
    """the nine columns of one entry (offset, length, flags[, inv_bc1, inv_sqrt_bc2, eps]) as float64"""
    off, n, flags = int(entry[0]), int(entry[1]), int(entry[2])
    fac = tuple(entry[3:6]) if len(entry) > 3 else (1.0, 1.0, 0.0)
    out = [0.0] * COLS
    for k, (bit, buf) in enumerate(((GRAD, g), (PARAM, p))):
        if flags & bit:
            x = buf[off:off + n].astype(np.float64)
            with np.errstate(all='ignore'):
                sq = x * x                                    # exact: 24-bit significands, exponents far inside float64's
            out[3 * k:3 * k + 3] = _group(x, [sq])
    if flags & UPDATE:
        ms, vs = m[off:off + n], v[off:off + n]
        u64 = update_direction(ms, vs, *fac)
        with np.errstate(all='ignore'):
            ul = update_direction(ms, vs, *fac, dtype=LD)
            sq = ul * ul
            hi = sq.astype(np.float64)
            lo = (sq - hi.astype(LD)).astype(np.float64)       # exact: 64 bits fit in 53 + 53
        out[6:9] = _group(u64, [hi, lo])
    return out


def reference(p, g, m, v, entries):
    return np.array([row(p, g, m, v, e) for e in entries], np.float64).reshape(len(entries), COLS)


def sum_bounds(entries):
    """[n_entries, 3]: the relative bounds of columns 0, 3 and 6"""
    return np.array([[e[1] * U, e[1] * U, (e[1] + 16) * U] for e in entries], np.float64).reshape(len(entries), 3)


def norm_bound(sum_bound):
    """a norm is the root of a sum: half the sum's relative bound (sqrt(1 + x) <= 1 + x / 2) plus the root's own rounding"""
    return 0.5 * sum_bound + U


def check(got, want, entries, what=''):
    """``got`` (float64 [n, 9], the kernel's) against ``want`` (``reference``): maxima and counts exact, sums inside ``sum_bounds``,
    groups not asked for exactly 0.  Returns the largest use of a sum's bound (1.0 = at the bound)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (len(entries), COLS), (what, got.shape, want.shape)
    bounds, worst = sum_bounds(entries), 0.0
    for r, e in enumerate(entries):
        for k, bit in enumerate((GRAD, PARAM, UPDATE)):
            s, mx, bad = got[r, 3 * k:3 * k + 3]
            if not (e[2] & bit):
                assert s == 0.0 and mx == 0.0 and bad == 0.0 and not np.signbit([s, mx, bad]).any(), (what, r, k, 'not asked for', s, mx, bad)
                continue
            ws, wm, wb = want[r, 3 * k:3 * k + 3]
            assert bad == wb, (what, r, k, 'count', bad, wb)
            assert mx == wm, (what, r, k, 'max', mx, wm)
            assert np.isfinite(s) and s >= 0.0, (what, r, k, 'sum', s)
            err = abs(s - ws)
            if ws == 0.0:
                assert s == 0.0, (what, r, k, 'sum', s)
            else:
                use = err / (bounds[r, k] * ws) if bounds[r, k] > 0 else (0.0 if err == 0.0 else np.inf)
                assert use <= 1.0, (what, r, k, 'sum', s, ws, use)
                worst = max(worst, use)
    return worst


def buffers(n, seed, dirty=True):
    """p, g, m, v: fp32 [n] with magnitudes over many binades, signs mixed, v >= 0; ``dirty``: a few -0, denormals and FLT_MAX spread
    through g and p (ordinary finite values)"""
    rng = np.random.default_rng(seed)

    def wide(scale):
        return (rng.standard_normal(n) * np.exp2(rng.integers(-20, 8, n)) * scale).astype(np.float32)
    p, g, m = wide(1.0), wide(1e-2), wide(1e-3)
    v = (wide(1e-3).astype(np.float64) ** 2).astype(np.float32)
    if dirty and n >= 8:
        at = rng.choice(n, size=min(n, 6), replace=False)
        g[at[0]], g[at[1]], g[at[2]] = -0.0, DENORMAL, FLT_MAX
        p[at[3]], p[at[4]], p[at[5]] = -0.0, -DENORMAL, -FLT_MAX
    return p, g, m, v


# the lengths, and the offsets modulo 4, every kernel test crosses
LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4097)
LONG = 200001
FACTORS = (1.0 / (1.0 - 0.9 ** 3), 1.0 / (1.0 - 0.999 ** 3) ** 0.5, 1e-8)        # an entry's inv_bc1, inv_sqrt_bc2, eps: update 3


def crossed_entries(flags=7):
    """every length at every offset modulo 4, with gaps of 0 .. 7 elements in between: 48 entries; returns (entries, extent)"""
    out, at = [], 0
    for i, n in enumerate(LENGTHS):
        for r in range(4):
            at += (r - at) % 4 + 4 * ((i + r) % 2)             # the next offset = r (mod 4); adjacent (gap 0) or a gap
            out.append((at, n, flags) + FACTORS)
            at += n
    return out, at
