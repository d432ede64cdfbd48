"""Row compaction, the masked-mean pooling pass and the un-pooling pass at the level of an op, against the float64 references of
tests/pool_cases.py, in every form the library has: the streaming kernels (one wave per candidate and 256-column block) and the
per-candidate fallback kernels, dense / compact with ``wts`` / compact without, fp32 and bf16-plane outputs, with and without the
sign bits of H1, and the older lirec_pool_fwd / lirec_pool_bwd pair with strides.

A. Compaction alone: integer-exact ``rowmap`` / ``cstart`` / ``count``, ``wts`` bit-exact, for the three mask dtypes, on the
   wave-per-candidate kernels (R <= 64 through lirec_compact_rows2) and on both forms of the single-workgroup kernel (R > 64, and
   every call of lirec_compact_rows: mask staged in LDS while n R floats + n + 1 ints fit 150 KiB, read from global memory beyond).
   Entries of rowmap / wts at and beyond ``count`` are unspecified and not looked at.

B. Pooling and un-pooling isolated from the GEMMs.  ``embed_fwd`` runs, and the device's OWN H1 is pooled in float64: Hbar and f
   are compared with that.  ``embed_bwd`` parts 3 leaves dHbar in the workspace (include/lirec_hip.h: rows32 * nseg * J floats
   behind dZ1), parts 5 un-pools it: dZ1 is compared with the float64 un-pooling of the device's OWN dHbar under the device's own
   relu decisions [H1 > 0].  Nothing a GEMM rounds enters either comparison and no element is left out.  Bounds, with
   u = 2^-24 (derived, not measured; the mask values make every divider exact -- pool_cases.py):
     Hbar   |err| <= (v + 2) u sum_r |m H1| / |div| per element, v = the candidate's valid rows: a left-to-right fp32 sum of v
            products (contracted to FMA or not) and one correctly rounded division  (pool_cases.hbar_bound);
     f      exact;
     dZ1    relative 4 u: m / div, * scale, d * f -- three roundings and one to spare;
     rows and elements written as zeros (masked-out dense rows, relu decision 0) are bit-zero.
   Which kernels run is the dispatch rule of DESIGN.md ("Which kernel a pooled head takes"), restated as pool_cases.family: the
   profile sites ``pool_fwd`` / ``pool_bwd`` are the same for both families, so the family cannot be read off; the rule sends
   R <= 64 with W % 4 == 0 to the streaming kernels (torch allocations are 16-byte aligned) and everything else -- here R in
   {65, 130} or W = 18 -- to pool_compact_kernel / unpool_relu_compact_kernel (compact) or pool_fwd_kernel's plain form /
   unpool_relu_kernel (dense); W = 18 takes their scalar paths, W = 64 / 260 their float4 paths.  Each call is asserted to be ONE
   launch of its site.

C. The ``planes`` forms (J = 256, gemm mode 2, as tests/test_gpu_layer1_persistent.py sets them up): after the whole backward the
   workspace holds dZ1 as bf16 hi / lo planes; hi + lo must be the float64 un-pooling of the device's dHbar to 4 u + 2^-17
   relative (the RNE split: for a in [2^e, 2^(e+1)) |a - hi| <= 2^(e-8), half a bf16 ulp, so half an ulp of lo = rne(a - hi) is at
   most 2^(e-17) <= 2^-17 |a|), rows in [valid, roundup32(valid)) and
   masked-out dense rows bit-zero in both planes, and dW1 / db1 that operand times the float64 rows to grad_close's bound.  The
   sign bits equal the packed [H1 > 0] of the device's H1 in every byte of a valid row.  A pooled head with R = 65 declines the
   planes path in forward and backward together (no ``stage`` / ``embed_dW1_reduce`` site) and meets the fp32 bounds on the
   fallback kernels; with ``hbits`` both calls fail.  (Before plane_layout declined it the backward un-pooled such a head with
   the streaming kernel, which holds one row weight per lane: the 65th row of a candidate was neither computed nor zeroed and the
   divider wrapped to lane 0 -- a silently wrong dW1 / db1.)

D. lirec_pool_fwd / lirec_pool_bwd with row strides W + 4 and W + 1 and every pointer one float off 16-byte alignment (the scalar
   paths at W % 4 == 0), R = 65, a weighted mask: the fp64 reference at test_gpu_ops.test_pool_fwd_bwd's tolerances, pad columns
   untouched."""
import ctypes as C

import pytest
import torch

import pool_cases as PC
from golden_util import assert_close, grad_close
from lirec_amd import _lib, ops
from lirec_amd._lib import LirecError
from oracle import lirec_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 20261017
OUTS = [5, 3, 4, 2]                 # second-layer widths (layer 2 is not under test here)
SENTINEL = -7.25


def bits_zero(t):
    """every element is +0.0 / bf16 +0 bit for bit"""
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[t.dtype]
    return not bool(t.contiguous().view(it).any())


def prof_sites():
    torch.cuda.synchronize()
    return ops.profile_read()


# ---------------------------------------------------------------------------------------------------------------------------
# A. compaction
# ---------------------------------------------------------------------------------------------------------------------------
DTYPES = [torch.float32, torch.int64, torch.float64]


def compaction_mask(n, R, dtype, seed=0, kind='patterns'):
    if kind == 'zero':
        m = torch.zeros(n, R)
    elif kind == 'full':
        m = torch.ones(n, R)
    else:
        m = PC.make_mask(n, R, True, 1, seed)
    if dtype == torch.int64:
        return (m * 2).to(torch.int64).to(DEV)                  # {0, 1, 2, 4}
    return m.to(dtype).to(DEV)


def compact_old(mask, n, R):
    """lirec_compact_rows through the C ABI: fp32 mask, no wts, cstart of n + 1 entries, the single-workgroup kernel at any R"""
    rowmap = torch.full((n * R,), -1, dtype=torch.int32, device=DEV)
    cstart = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().lirec_compact_rows(mask.data_ptr(), n, R, rowmap.data_ptr(), cstart.data_ptr(), count.data_ptr(),
                                             ops.current_stream_handle()), 'lirec_compact_rows')
    return rowmap, cstart, count, None


def check_compaction(out, mask, n, R, tag):
    rowmap, cstart, count, wts = out
    rrm, rcs, rcount, _ = PC.compact_ref(mask)
    assert int(count.item()) == rcount, (tag, int(count.item()), rcount)
    assert cstart.numel() == n + 1 and torch.equal(cstart, rcs), tag + ': cstart'
    assert torch.equal(rowmap[:rcount], rrm), tag + ': rowmap'
    if wts is not None:
        want = mask.reshape(-1)[rrm.long()].float()
        assert torch.equal(wts[:rcount].view(torch.int32), want.view(torch.int32)), tag + ': wts'
    return rcount


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'i64', 'f64'])
@pytest.mark.parametrize('n,R,path', PC.COMPACT_SHAPES, ids=['%dx%d' % (n, R) for n, R, _ in PC.COMPACT_SHAPES])
def test_compact_rows2(n, R, path, dtype):
    """ops.compact_rows: the wave-per-candidate kernels for R <= 64, the single-workgroup kernel beyond -- staged in LDS (5 x 65)
    or reading global memory (600 x 65: 158404 bytes > 150 KiB)"""
    assert path == ('wave' if R <= 64 else ('serial-lds' if PC.serial_staged(n, R) else 'serial-global'))
    mask = compaction_mask(n, R, dtype, seed=n)
    if R == 64:
        assert bool((mask[:, 63] != 0).any())                   # (the last lane: bit 63 of the ballot)
    check_compaction(ops.compact_rows(mask, n, R), mask, n, R, 'compact_rows2 %dx%d' % (n, R))


@pytest.mark.parametrize('n,R', [(n, R) for n, R, _ in PC.COMPACT_SHAPES], ids=['%dx%d' % (n, R) for n, R, _ in PC.COMPACT_SHAPES])
def test_compact_rows_serial_kernel(n, R):
    """lirec_compact_rows: compact_rows_serial_kernel at every shape -- 1100 x 30 gives two candidates to a thread (n > 1024) with
    the mask staged in LDS (136404 bytes), 600 x 65 is not staged"""
    assert PC.serial_staged(n, R) == ((n, R) != (600, 65))
    mask = compaction_mask(n, R, torch.float32, seed=n + 1)
    check_compaction(compact_old(mask, n, R), mask, n, R, 'compact_rows %dx%d' % (n, R))


@pytest.mark.parametrize('kind', ['zero', 'full'])
@pytest.mark.parametrize('n,R', [(3, 5), (9, 64), (5, 65), (600, 65)])
def test_compact_rows_all_zero_and_all_valid(n, R, kind):
    for dtype in DTYPES:
        mask = compaction_mask(n, R, dtype, kind=kind)
        for out in (ops.compact_rows(mask, n, R),) + ((compact_old(mask, n, R),) if dtype == torch.float32 else ()):
            cnt = check_compaction(out, mask, n, R, '%s %dx%d' % (kind, n, R))
            assert cnt == (0 if kind == 'zero' else n * R)
            if kind == 'zero':
                assert not bool(out[1].any())                   # cstart all 0


@pytest.mark.parametrize('n,R', [(9, 64), (5, 65)])
def test_compact_rows_out_reuse(n, R):
    """``out=``: a sparser mask written into the buffers of a denser one"""
    dense = compaction_mask(n, R, torch.float32, kind='full')
    out = ops.compact_rows(dense, n, R)
    check_compaction(out, dense, n, R, 'dense')
    sparse = compaction_mask(n, R, torch.float32, seed=3)
    again = ops.compact_rows(sparse, n, R, out=out)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, again))
    cnt = check_compaction(again, sparse, n, R, 'sparse into dense')
    assert 0 < cnt < n * R


# ---------------------------------------------------------------------------------------------------------------------------
# B / C: one pooled head
# ---------------------------------------------------------------------------------------------------------------------------
class PooledHead:
    """buffers and arguments of one pooled head: ``form`` 'dense' | 'wts' | 'nowts' (pool_cases.PoolCase)"""

    def __init__(self, form, clamp, mask, n, R, J, dims, p, hbits=False, planes=False, seed=0):
        g = torch.Generator().manual_seed(SEED + seed)
        self.form, self.clamp, self.n, self.R, self.J, self.p = form, clamp, n, R, J, p
        ns = self.ns = len(dims)
        self.W = W = ns * J
        self.rows = rows = n * R
        self.rows32 = (rows + 31) // 32 * 32
        self.D = D = sum(dims)
        self.dims, self.offs, self.outs = dims, [sum(dims[:i]) for i in range(ns)], OUTS[:ns]
        self.Wd = sum(self.outs)
        self.segs = ops.Segments(self.offs, dims, self.outs)
        self.sel = (R, R + 1, 1)
        self.X = torch.randn(n, R + 1, D, generator=g).to(DEV)
        self.mask = mask.to(DEV)
        dev = lambda ts: [t.to(DEV) for t in ts]
        self.W1 = dev([torch.randn(J, d, generator=g) / d ** 0.5 for d in dims])
        self.b1 = dev([torch.randn(J, generator=g) * 0.1 for _ in dims])
        self.W2 = dev([torch.randn(o, J, generator=g) / J ** 0.5 for o in self.outs])
        self.b2 = dev([torch.randn(o, generator=g) * 0.1 for o in self.outs])
        self.dZ2 = torch.randn(n, self.Wd, generator=g).to(DEV)
        nan = float('nan')
        self.H1 = torch.full((rows, W), nan, device=DEV)
        self.Hbar = torch.full((n, W), nan, device=DEV)
        self.f = torch.full((n,), nan, device=DEV)
        self.Z2 = torch.full((n, self.Wd), nan, device=DEV)
        self.compact = form != 'dense'
        cmp = ops.compact_rows(self.mask, n, R) if self.compact else None
        if form == 'nowts':
            cmp = cmp[:3]
        # ('wts': the kernels must take the weights from wts -- the mask itself is withheld)
        self.pool = (None if form == 'wts' else self.mask, R, clamp, self.Hbar, self.f, cmp)
        self.hb = torch.full((max(ops.hbits_bytes(rows, W), 16),), 0xA5, dtype=torch.uint8, device=DEV) if hbits else None
        self.planes = torch.full((ops.planes_bytes(rows, D, J),), 0x3C, dtype=torch.uint8, device=DEV) if planes else None
        self.drop = ops.make_dropout(SEED, p, 1, 3)
        self.ws = torch.full((ops.workspace_bytes(rows + n, ns, J) // 4,), 3.0, device=DEV)
        self.gW1 = [torch.zeros_like(t) for t in self.W1]; self.gb1 = [torch.zeros_like(t) for t in self.b1]
        self.gW2 = [torch.zeros_like(t) for t in self.W2]; self.gb2 = [torch.zeros_like(t) for t in self.b2]
        self.rrm, _, self.cnt, _ = PC.compact_ref(self.mask)

    def fwd_args(self):
        return ops.embed_fwd_args(self.X, self.D, self.sel, self.rows, self.J, self.segs, self.W1, self.b1, self.W2, self.b2,
                                  self.H1, self.Z2.data_ptr(), self.Wd, None, 0, 0, self.drop, pool=self.pool, planes=self.planes,
                                  hbits=self.hb)

    def bwd_args(self, parts=0):
        return ops.embed_bwd_args(self.X, self.D, self.sel, self.rows, self.J, self.segs, self.W2,
                                  None if self.hb is not None else self.H1, self.dZ2.data_ptr(), self.Wd, self.gW1, self.gb1,
                                  self.gW2, self.gb2, self.ws, self.drop, pool=self.pool, planes=self.planes, hbits=self.hb,
                                  parts=parts)

    # -- what the device left -------------------------------------------------------------------------------------------
    def valid_rows(self):
        """(logical ids of the rows carrying a non-zero mask, the device rows of H1 / dZ1 / hbits that hold them)"""
        ids = self.rrm.long()
        return ids, (torch.arange(self.cnt, device=DEV) if self.compact else ids)

    def dense_H1(self):
        """float64 [rows, W]: the device's H1 at its logical rows (compact: rows never computed are 0 -- their mask is 0)"""
        ids, at = self.valid_rows()
        assert bool(torch.isfinite(self.H1[at]).all()), 'H1 not written at a valid row'
        if not self.compact:
            assert bool(torch.isfinite(self.H1).all())
            return self.H1.double()
        Hd = torch.zeros(self.rows, self.W, dtype=torch.float64, device=DEV)
        Hd[ids] = self.H1[at].double()
        return Hd

    def dHbar(self):
        o = self.rows32 * self.W
        d = self.ws[o:o + self.n * self.W].view(self.n, self.W)
        assert bool(torch.isfinite(d).all()), 'dHbar not written'
        return d

    def check_forward(self, tag):
        Hd = self.dense_H1()
        Hbar, f, unit, valid = PC.masked_mean(Hd.view(self.n, self.R, self.W), self.mask, self.clamp)
        assert bool(torch.isfinite(self.Hbar).all()) and bool(torch.isfinite(self.f).all()), tag + ': Hbar / f not written'
        assert_close(self.Hbar, Hbar, 0.0, PC.hbar_bound(unit, valid).reshape(-1), tag + ' Hbar')
        assert torch.equal(self.f.double(), f), tag + ': f is not exact'
        none = valid == 0
        if bool(none.any()):                                      # (clamp_zero: an all-masked candidate pools to exact zeros)
            assert bits_zero(self.Hbar[none]) and not bool(self.f[none].any())
        self.dec = (Hd > 0).view(self.n, self.R, self.W)
        return Hd

    def check_hbits(self, tag):
        _, at = self.valid_rows()
        ncb = (self.W + 255) // 256
        got = self.hb[:self.rows * ncb * 32].view(self.rows, ncb * 32)[at]
        want = PC.pack_sign_bits(self.H1[at])
        assert torch.equal(got, want), '%s: %d sign-bit bytes differ' % (tag, int((got != want).sum()))

    def dZ1_ref(self):
        return PC.unpool(self.dHbar(), self.mask, self.clamp, PC.drop_scale(self.p), self.dec).view(self.rows, self.W)

    def check_dZ1_fp32(self, tag):
        """the fp32 dZ1 at the start of the workspace; returns it at the valid rows (float64)"""
        ids, at = self.valid_rows()
        ref = self.dZ1_ref()
        got = self.ws[:self.rows * self.W].view(self.rows, self.W)
        assert_close(got[at], ref[ids], PC.DZ1_RTOL, PC.TINY, tag + ' dZ1')
        zero = ~self.dec.view(self.rows, self.W)[ids]
        assert bits_zero(got[at][zero]), tag + ': a dZ1 element behind a relu decision 0 is not +0'
        if not self.compact:
            masked = self.mask.reshape(-1) == 0
            assert bits_zero(got[masked]), tag + ': a masked-out dense row of dZ1 is not bit-zero'
        return got[at].double()

    def check_dZ1_planes(self, tag):
        """the bf16 hi / lo planes over the workspace; returns hi + lo at the valid rows (float64)"""
        ids, at = self.valid_rows()
        ref = self.dZ1_ref()
        pl = self.ws.view(torch.bfloat16)[:2 * self.rows32 * self.W].view(2, self.rows32, self.W)
        op = pl[0].double() + pl[1].double()
        assert_close(op[at], ref[ids], PC.PLANES_RTOL, PC.TINY, tag + ' dZ1 (hi + lo)')
        valid = self.cnt if self.compact else self.rows
        up = (valid + 31) // 32 * 32
        assert bits_zero(pl[:, valid:up]), tag + ': the rows behind the last valid one are not bit-zero'
        if not self.compact:
            masked = torch.nonzero(self.mask.reshape(-1) == 0).view(-1)
            assert bits_zero(pl[:, masked]), tag + ': a masked-out dense row is not bit-zero in both planes'
        return op[at]

    def check_dW1(self, op, tag):
        """dW1 / db1 against the given dZ1 operand (valid rows) times the float64 feature rows"""
        ids, _ = self.valid_rows()
        xr = self.X[:, 1:self.R + 1, :].reshape(self.rows, self.D).double()[ids]
        for i, (o, d) in enumerate(zip(self.offs, self.dims)):
            z = op[:, i * self.J:(i + 1) * self.J]
            grad_close(self.gW1[i], z.t() @ xr[:, o:o + d], '%s dW1[%d]' % (tag, i))
            grad_close(self.gb1[i], z.sum(0), '%s db1[%d]' % (tag, i))


@pytest.mark.parametrize('case', PC.POOL_CASES, ids=[c.id for c in PC.POOL_CASES])
def test_pool_and_unpool_against_fp64(case):
    c = case
    mask = PC.make_mask(c.n, c.R, c.weighted, c.clamp, seed=c.R)
    h = PooledHead(c.form, c.clamp, mask, c.n, c.R, c.J, [8] * c.nseg, c.p, hbits=c.hbits, seed=c.R + c.W)
    assert c.family == ('streaming' if c in PC.STREAMING else 'fallback')
    tag = c.id + ' (' + c.family + ')'
    try:
        ops.profile_enable(True)
        ops.embed_fwd(args=h.fwd_args())
        sites = prof_sites()
        assert sites['pool_fwd']['launches'] == 1 and 'stage' not in sites, sites
        h.check_forward(tag)
        if c.hbits:
            h.check_hbits(tag)
        ba = h.bwd_args(parts=3)
        ops.embed_bwd(args=ba)                                    # dHbar
        ops.profile_enable(True)
        ops.embed_bwd(args=ops.with_parts(ba, 5))                 # the un-pooling pass alone
        sites = prof_sites()
        assert set(sites) == {'pool_bwd'} and sites['pool_bwd']['launches'] == 1, sites
        h.check_dZ1_fp32(tag)
    finally:
        ops.profile_enable(False)


# ---------------------------------------------------------------------------------------------------------------------------
# C. the planes forms
# ---------------------------------------------------------------------------------------------------------------------------
def planes_mask(kind, n, R, seed):
    if kind == 'zero':
        return torch.zeros(n, R)
    if kind == 'full':
        return torch.ones(n, R)
    return PC.make_mask(n, R, kind == 'weighted', 1, seed)


def run_planes(form, R, kind, hbits, n=5, expect_planes=True):
    mask = planes_mask(kind, n, R, seed=R)
    h = PooledHead(form, 1, mask, n, R, 256, [256], 0.3, hbits=hbits, planes=True, seed=R)
    tag = 'planes %s R %d %s%s' % (form, R, kind, ' hbits' if hbits else '')
    ops.ensure_scratch(DEV)
    ops.set_gemm_mode(2)
    try:
        ops.profile_enable(True)
        ops.embed_fwd(args=h.fwd_args())
        fs = prof_sites()
        h.check_forward(tag)
        if hbits:
            h.check_hbits(tag)
        ops.profile_enable(True)
        ops.embed_bwd(args=h.bwd_args())
        bs = prof_sites()
        on = (fs.get('stage', {}).get('launches', 0) > 0, bs.get('embed_dW1_reduce', {}).get('launches', 0) > 0)
        assert on == (expect_planes, expect_planes), (tag, 'planes path taken in (forward, backward):', on, fs, bs)
        assert fs['pool_fwd']['launches'] == 1 and bs['pool_bwd']['launches'] == 1
        op = h.check_dZ1_planes(tag) if expect_planes else h.check_dZ1_fp32(tag)
        h.check_dW1(op, tag)
    finally:
        ops.profile_enable(False)
        ops.set_gemm_mode(_lib.default_gemm_mode())
    return h


@pytest.mark.parametrize('form,R,kind,hbits', [
    ('wts', 5, 'weighted', True),          # 12 valid rows or fewer: a tail of zero rows up to 32
    ('wts', 64, 'binary', False),          # 0 + 1 + 1 + 64 + 8 valid rows: not a multiple of 32
    ('nowts', 64, 'weighted', True),
    ('wts', 64, 'full', False),            # 320 valid rows: no tail
    ('wts', 5, 'zero', True),              # count == 0
    ('dense', 5, 'weighted', True),        # n R = 25: the zero tail with count == NULL, masked-out rows zeroed, dense hbits
    ('dense', 64, 'binary', False),        # n R = 320, masked-out rows only
    ('dense', 5, 'zero', False),
])
def test_planes_forms(form, R, kind, hbits):
    h = run_planes(form, R, kind, hbits)
    if kind in ('weighted', 'binary') and form != 'dense':
        assert h.cnt % 32 != 0
    if form == 'dense' and R == 5:
        assert h.rows % 32 != 0


@pytest.mark.parametrize('form', ['wts', 'dense'])
def test_planes_declined_beyond_64_context_rows(form):
    """R = 65 with ``planes``: forward and backward fall back together, and meet the fp32 bounds there"""
    h = run_planes(form, 65, 'weighted', False, expect_planes=False)
    assert h.mask[3].ne(0).sum() == 65                          # (a candidate whose 65th row is valid)


@pytest.mark.parametrize('form', ['wts', 'dense'])
def test_sign_bits_refused_beyond_64_context_rows(form):
    mask = planes_mask('weighted', 5, 65, seed=65)
    h = PooledHead(form, 1, mask, 5, 65, 256, [256], 0.3, hbits=True, planes=True, seed=65)
    h.Hbar.zero_(); h.f.zero_()
    ops.ensure_scratch(DEV)
    ops.set_gemm_mode(2)
    try:
        with pytest.raises(LirecError, match=r'\(code %d\)' % _lib.LIREC_EINVAL):
            ops.embed_fwd(args=h.fwd_args())
        with pytest.raises(LirecError, match=r'\(code %d\)' % _lib.LIREC_EINVAL):
            ops.embed_bwd(args=h.bwd_args())
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(_lib.default_gemm_mode())


# ---------------------------------------------------------------------------------------------------------------------------
# D. lirec_pool_fwd / lirec_pool_bwd with strides
# ---------------------------------------------------------------------------------------------------------------------------
def strided(rows, W, ld, fill=None, g=None):
    """a [rows, W] view with row stride ld, one float into a sentinel-filled buffer: (buffer, view)"""
    buf = torch.full((1 + rows * ld,), SENTINEL, device=DEV)
    v = buf[1:].view(rows, ld)[:, :W]
    if fill is not None:
        v.copy_(fill)
    return buf, v


def pads_untouched(buf, rows, W, ld):
    body = buf[1:].view(rows, ld)
    return float(buf[0]) == SENTINEL and bool((body[:, W:] == SENTINEL).all())


@pytest.mark.parametrize('clamp', [1, 0])
@pytest.mark.parametrize('extra', [4, 1])
def test_pool_fwd_bwd_strided(extra, clamp):
    n, R, W, p, seed = 9, 65, 48, 0.3, 5
    ld = W + extra
    g = torch.Generator().manual_seed(SEED + extra)
    mask = PC.make_mask(n, R, True, clamp, seed=extra).to(DEV)
    Z = torch.randn(n * R, W, generator=g).to(DEV)
    dP = torch.randn(n, W, generator=g).to(DEV)
    zb, zv = strided(n * R, W, ld, Z)
    tb, tv = strided(n, W, ld)
    eb, ev = strided(n, W, ld)
    pb, pv = strided(n, W, ld, dP)
    db, dv = strided(n * R, W, ld)
    ops.pool_fwd(zv, ld, mask, n, R, W, clamp, tv.data_ptr(), ld, ev.data_ptr(), ld, ops.make_dropout(seed, p, 0, 3))
    ops.pool_bwd(pv.data_ptr(), ld, mask, n, R, W, clamp, dv, ld)
    torch.cuda.synchronize()
    keep = torch.from_numpy(O.dropout_keep_mask(seed, 3, n, W, p)).to(DEV)
    Tn, E = PC.pool_fwd_ref(Z.view(n, R, W), mask, clamp, keep, p)
    assert_close(tv, Tn, 1e-5, 1e-6, 'Tn (ld W + %d)' % extra)
    assert_close(ev, E, 1e-5, 1e-6, 'E (ld W + %d)' % extra)
    assert_close(dv, PC.pool_bwd_ref(dP, mask, clamp).view(n * R, W), 1e-6, 1e-7, 'dZ (ld W + %d)' % extra)
    for buf, rows in ((tb, n), (eb, n), (db, n * R)):
        assert pads_untouched(buf, rows, W, ld)
    assert torch.equal(zv, Z) and torch.equal(pv, dP)
