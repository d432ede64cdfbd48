"""Cases and float64 references of the pooling family (tests/test_gpu_pooling.py, tests/test_host_pooling.py) -- not a test module.

The family is what sits between layer 1 and layer 2 of the context head: row compaction (lirec_compact_rows / lirec_compact_rows2),
the masked mean over a candidate's context rows, its backward (un-pooling fused with the relu / dropout derivative of layer 1), and
the older K3 pair lirec_pool_fwd / lirec_pool_bwd (masked mean -> tanh -> dropout).  Every reference here is the plain definition in
float64, written with torch on whatever device its inputs are on; tests/test_host_pooling.py pins them to torch autograd of the
un-pooled definition and to torch.nonzero.

Masks: the values come from {0, 1} (binary) or {0, 0.5, 1, 2} (weighted), so a candidate's divider -- a sum of at most 130 multiples
of 0.5, each at most 2 -- is exact in fp32 in any summation order: the divider is the same number on the device and in the reference
and does not enter an error budget.
"""
import dataclasses

import torch

U = 2.0 ** -24                      # unit roundoff of fp32
TINY = 1e-300                       # added to a derived bound so that 0 / 0 does not appear in the achieved-error log (a bound of
#                                     0 still admits no error: any fp32 difference is > 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------
# the mask generator
# ---------------------------------------------------------------------------------------------------------------------------
def patterns(n, R, clamp):
    """[(candidate, name, number of valid rows)] of the promised per-candidate patterns; candidates not listed are random.
    With n >= 8 every pattern is present (the k-valid-row ones where R allows); a smaller n keeps the first n of the list."""
    want = [('none' if clamp else 'one_mid', 0 if clamp else 1), ('one_first', 1), ('one_last', 1), ('all', R)]
    want += [('valid_%d' % k, k) for k in (8, 9, 15, 16) if k <= R]
    return [(c, name, v) for c, (name, v) in enumerate(want[:n])]


def make_mask(n, R, weighted, clamp, seed=0):
    """fp32 [n, R] on the CPU.  Without clamp no candidate is all zero (the reference itself is NaN there)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * n + R + (1000 if weighted else 0) + (500 if clamp else 0))
    vals = torch.tensor([0.5, 1.0, 2.0]) if weighted else torch.tensor([1.0])
    draw = lambda *s: vals[torch.randint(0, len(vals), s, generator=g)]
    m = draw(n, R) * (torch.rand(n, R, generator=g) < 0.6).float()
    for c, name, v in patterns(n, R, clamp):
        m[c] = 0
        if name == 'one_first':
            m[c, 0] = draw(1)
        elif name == 'one_last':
            m[c, R - 1] = draw(1)
        elif name == 'one_mid':
            m[c, R // 2] = draw(1)
        elif name != 'none':                                   # 'all' and 'valid_k': k rows scattered over the candidate
            rows = torch.randperm(R, generator=g)[:v]
            m[c, rows] = draw(v)
    if not clamp:
        for c in range(n):
            if not bool(m[c].any()):
                m[c, int(torch.randint(0, R, (1,), generator=g))] = draw(1)
    return m.float()


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------
def compact_ref(mask):
    """(rowmap [count] int32, cstart [n + 1] int32, count int, wts [count] fp32) of a mask [n, R] -- by prefix sums, not by
    torch.nonzero (tests/test_host_pooling.py compares the two)."""
    n, R = mask.shape
    flat = mask.reshape(-1)
    nz = flat != 0
    pos = torch.cumsum(nz.long(), 0) - 1                       # compact position of every valid entry
    count = int(nz.sum())
    rowmap = torch.zeros(count, dtype=torch.int32, device=mask.device)
    ids = torch.arange(n * R, device=mask.device, dtype=torch.int32)
    rowmap[pos[nz]] = ids[nz]
    per = nz.view(n, R).sum(1)
    cstart = torch.cat([torch.zeros(1, dtype=torch.long, device=mask.device), torch.cumsum(per, 0)]).int()
    wts = flat[rowmap.long()].float()
    return rowmap, cstart, count, wts


def divider(mask, clamp):
    """float64 [n]: sum of the mask row, 0 -> 1 under clamp_zero"""
    div = mask.double().sum(1)
    if clamp:
        div = torch.where(div == 0, torch.ones_like(div), div)
    return div


def masked_mean(H, mask, clamp):
    """H [n, R, W], mask [n, R] -> (Hbar [n, W], f [n], bound_unit [n, W], valid [n]) in float64:
    Hbar[c] = sum_r m[c, r] H[c, r] / div[c],  f[c] = sum_r m[c, r] / div[c];  bound_unit = sum_r |m H| / |div|, valid = the
    candidate's number of rows with a non-zero mask (both enter the device bound, see hbar_bound)."""
    m = mask.double()
    div = divider(mask, clamp)
    prod = H.double() * m.unsqueeze(2)
    Hbar = prod.sum(1) / div.unsqueeze(1)
    f = m.sum(1) / div
    return Hbar, f, prod.abs().sum(1) / div.abs().unsqueeze(1), (mask != 0).sum(1)


def hbar_bound(unit, valid):
    """|device Hbar - float64 Hbar| per element: the device forms v products m * H (exact for m in {0.5, 1, 2}, one rounding
    otherwise -- or none, contracted to an FMA), adds them left to right in fp32 (v roundings at most, each relative to a partial
    sum that is at most sum |m H| (1 + u)^v), and divides once, correctly rounded: (v + 2) u sum_r |m H| / |div| covers all of it
    to first order with one rounding to spare."""
    return (valid.double().unsqueeze(1) + 2.0) * U * unit + TINY


def unpool(dHbar, mask, clamp, scale, dec):
    """dZ1[c, r] = dHbar[c] * (m[c, r] / div[c] * scale) * dec[c, r]   (dec [n, R, W] = the relu / dropout decisions [H1 > 0])"""
    w = mask.double() / divider(mask, clamp).unsqueeze(1) * scale
    return dHbar.double().unsqueeze(1) * w.unsqueeze(2) * dec.double()


DZ1_RTOL = 4 * U                    # m / div, * scale, d * f: three roundings, one to spare
# + the RNE split into bf16 hi / lo: for a in [2^e, 2^(e+1)) |a - hi| <= 2^(e-8) (half a bf16 ulp), so half an ulp of lo = rne(a - hi)
# is at most 2^(e-17) <= 2^-17 |a|
PLANES_RTOL = 4 * U + 2.0 ** -17


def pool_fwd_ref(Z, mask, clamp, keep, p):
    """the older K3 pair (lirec_pool_fwd): Tn = tanh(masked mean), E = Tn * keep / (1 - p)"""
    P = masked_mean(Z, mask, clamp)[0]
    Tn = torch.tanh(P)
    return Tn, Tn * keep.double() / (1.0 - p)


def pool_bwd_ref(dP, mask, clamp):
    """lirec_pool_bwd: dZ[c, r] = dP[c] * m[c, r] / div[c]"""
    return dP.double().unsqueeze(1) * (mask.double() / divider(mask, clamp).unsqueeze(1)).unsqueeze(2)


def drop_scale(p):
    """the library's 1 / (1 - p): (float)(1.0 / (1.0 - (double)(float)p))"""
    if p <= 0:
        return 1.0
    pf = float(torch.tensor(p, dtype=torch.float32))
    return float(torch.tensor(1.0 / (1.0 - pf), dtype=torch.float64).float())


def pack_sign_bits(H):
    """uint8 [rows, ncb * 32] of H [rows, W]: the layout of lirec_embed_fwd_args::hbits -- per row and 256-column block 32 bytes,
    bit b of byte i = [H[row, 256 cb + 8 i + b] > 0], zero beyond column W."""
    rows, W = H.shape
    ncb = (W + 255) // 256
    bits = torch.zeros(rows, ncb * 256, dtype=torch.uint8, device=H.device)
    bits[:, :W] = (H > 0).to(torch.uint8)
    wgt = (2 ** torch.arange(8, device=H.device)).to(torch.int32)
    return (bits.view(rows, ncb * 32, 8).to(torch.int32) * wgt).sum(2).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# which kernels a pooled head takes ("Which kernel a pooled head takes")
# ---------------------------------------------------------------------------------------------------------------------------
def family(R, W):
    """'streaming' (pool_rows_kernel / unpool_rows_kernel: one wave per candidate and 256-column block) when R <= 64 and
    W % 4 == 0 (and 16-byte aligned buffers, which every torch allocation is); else 'fallback' (one workgroup per candidate:
    pool_compact_kernel / unpool_relu_compact_kernel when compact, pool_fwd_kernel's plain form / unpool_relu_kernel when dense)."""
    return 'streaming' if R <= 64 and W % 4 == 0 else 'fallback'


@dataclasses.dataclass(frozen=True)
class PoolCase:
    """one pooled head driven through embed_fwd / embed_bwd parts 3 + 5.  form: 'dense' | 'wts' (compact, 4-tuple) | 'nowts'
    (compact, 3-tuple: the kernels read mask[rowmap[j]]).  W = nseg * J; in_dim is 8 per segment."""
    form: str
    clamp: int
    weighted: bool
    n: int
    R: int
    J: int
    nseg: int
    p: float = 0.0
    hbits: bool = False

    @property
    def W(self):
        return self.nseg * self.J

    @property
    def family(self):
        return family(self.R, self.W)

    @property
    def vec(self):
        """fallback kernels: the float4 path (W % 4 == 0) or the scalar one"""
        return self.W % 4 == 0

    @property
    def id(self):
        return '%s-c%d-%s-n%d-R%d-W%d%s%s' % (self.form, self.clamp, 'wt' if self.weighted else 'bin', self.n, self.R, self.W,
                                             '-p' if self.p else '', '-hbits' if self.hbits else '')


# W: 8 = 1 x 8, 64 = 4 x 16, 260 = 4 x 65 (a partial last 256-column block), 1024 = 4 x 256 (four full blocks), 18 = 3 x 6
STREAMING = [
    PoolCase('dense', 1, False, 9, 1, 8, 1),
    PoolCase('wts', 0, True, 9, 8, 16, 4, p=0.3),
    PoolCase('nowts', 1, True, 9, 9, 65, 4),
    PoolCase('dense', 0, True, 9, 15, 65, 4, p=0.3),
    PoolCase('wts', 1, False, 10, 33, 256, 4),
    PoolCase('nowts', 0, False, 9, 63, 16, 4, p=0.3),
    PoolCase('dense', 1, True, 9, 64, 256, 4, p=0.3),
    PoolCase('wts', 1, True, 9, 64, 65, 4),
    PoolCase('nowts', 0, True, 9, 33, 8, 1),
    PoolCase('dense', 0, False, 3, 9, 16, 4),                   # n % 4 != 0: a partial last workgroup
    # the sign bits of H1 off the planes path: a partial last column block (lanes beyond W write zero nibbles), one lane pair
    PoolCase('wts', 1, True, 9, 15, 65, 4, p=0.3, hbits=True),
    PoolCase('dense', 1, False, 9, 9, 8, 1, p=0.3, hbits=True),
    # the grid-stride loop: 2048 workgroups x 4 waves = 8192 tasks per sweep; n = 300 candidates x 28 column blocks = 8400 tasks
    # (at W = 1024 a 300-candidate head has 1200 tasks and does not wrap)
    PoolCase('wts', 1, False, 300, 8, 1792, 4),
]
FALLBACK = [
    PoolCase('wts', 1, True, 9, 65, 16, 4, p=0.3),              # pool_compact_kernel / unpool_relu_compact_kernel, float4 path
    PoolCase('dense', 0, False, 9, 65, 16, 4),                  # pool_fwd_kernel (plain) / unpool_relu_kernel, float4 path
    PoolCase('nowts', 1, True, 9, 130, 6, 3),                   # ... and their scalar paths (W = 18)
    PoolCase('dense', 1, True, 9, 130, 6, 3, p=0.3),
    PoolCase('dense', 0, False, 9, 8, 6, 3),                    # R <= 64 but W % 4 != 0
    PoolCase('wts', 1, False, 9, 9, 6, 3, p=0.3),
    PoolCase('nowts', 0, True, 9, 65, 65, 4),                   # W = 260
    PoolCase('dense', 1, False, 9, 130, 65, 4),
]
POOL_CASES = STREAMING + FALLBACK

# (n, R) of the compaction tests, and what lirec_compact_rows2 runs there (lirec_compact_rows always runs the serial kernel)
COMPACT_SHAPES = [
    (1, 1, 'wave'), (3, 5, 'wave'), (9, 64, 'wave'), (301, 18, 'wave'),
    (5, 65, 'serial-lds'), (1100, 30, 'wave'), (600, 65, 'serial-global'),
]
SERIAL_LDS_BYTES = 150 * 1024


def serial_staged(n, R):
    """does compact_rows_serial_kernel stage the mask in LDS?  (the launcher's rule: n R floats + n + 1 ints within 150 KiB)"""
    return n * R * 4 + (n + 1) * 4 <= SERIAL_LDS_BYTES
