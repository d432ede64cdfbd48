"""Cases, generators, float64 references and comparators of the input-gradient / piece-table family (tests/test_gpu_dx_pieces.py,
tests/test_host_dx_cases.py) -- not a test module.

The family: lirec_embed_dx (gemm_dx.hpp: dx_gemm_kernel + dx_zero_kernel), lirec_embed_dx_indexed (dxi_gemm_kernel),
lirec_embed_dw1_indexed (kernels.hpp: onehot_kernel + two weight-gradient GEMM stages) and lirec_embed_l1_indexed (table GEMMs +
gather_act_kernel).  The operand of every backward op is hand-filled (dZ1 in the head's workspace, or S), so each reference is
the plain definition in float64 of the very values the device reads; tests/test_host_dx_cases.py pins the references to torch
autograd of "expand the tables through the index into rows, Linear per segment, sum".  Everything here runs on the CPU.

Bounds (derived, not measured), u = 2^-24:
  exact core (gemm mode 0)   |err| <= (K + 4) u sum_k |a_k| |b_k| per element: every MFMA step is one fused multiply-add into an
                             fp32 accumulator, K roundings in some order, each relative to a partial sum of at most
                             sum |a| |b| (1 + u)^K; four roundings to spare (a bias, a scale, an accumulated initial value).
                             K is the full reduction length: all chunks of a piece-table problem, both stages of dW1 / db1.
  split core (gemm mode 2/3) 1e-4 |ref| + 4e-5 max |ref| of the compared block: the project's op-level bound for bf16x3
                             (test_gpu_ops.tol, test_gpu_layer1_persistent.tol).
Neighbouring segments of a head's dZ1 are scaled by 1, 10, 100, 1000 and each (head, segment) block is compared against its own
scale, so a k-tail that reads into the next segment lands far outside either bound.
"""
import dataclasses
import functools
import zlib

import torch

import pool_cases as PC
from golden_util import assert_close

U = PC.U
TINY = PC.TINY
SPLIT_RTOL, SPLIT_STOL = 1e-4, 4e-5
SEG_SCALE = (1.0, 10.0, 100.0, 1000.0)
NAN = float('nan')


def gen(name, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(name.encode()) + 7919 * salt) & 0x7fffffff)


def bound(mode, ref, absprod, K):
    """per-element bound of a block (float64 tensors), see the module docstring"""
    if mode in (0, 1):
        return (K + 4.0) * U * absprod + TINY
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    return SPLIT_RTOL * ref.abs() + SPLIT_STOL * scale + TINY


def bits_zero(t):
    """every element is +0.0 bit for bit (-0.0 and NaN fail)"""
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[t.dtype]
    return not bool(t.contiguous().view(it).any())


def close(got, ref, bnd, what):
    """finite everywhere (a NaN left from the pre-fill is an element never written), then golden_util.assert_close"""
    got = torch.as_tensor(got)
    assert bool(torch.isfinite(got).all()), '%s: %d elements not written (or not finite)' % (what, int((~torch.isfinite(got)).sum()))
    assert_close(got, ref, 0.0, bnd.reshape(-1), what)


# ---------------------------------------------------------------------------------------------------------------------------
# masks and row lists
# ---------------------------------------------------------------------------------------------------------------------------
# compact ids of the 'straddle' mask (n = 4, R = 18): four-row units whose Philox blocks (id >> 2) run 1 + 2 + 1, 1 + 1 + 1 + 1, 4,
# 1 + 3, 2 + 2, 1 + 1 + 2, 3 + 1, and a last unit of three rows, 1 + 2 (count % 4 != 0)
STRADDLE_IDS = (3, 4, 5, 9, 14, 18, 22, 26, 28, 29, 30, 31, 35, 36, 37, 38, 41, 42, 44, 45, 47, 48, 52, 53, 56, 57, 58, 60, 62, 65, 66)
STRADDLE_RUNS = {(1, 2, 1), (1, 1, 1, 1), (4,), (1, 3), (2, 2), (1, 1, 2), (3, 1), (1, 2)}


def make_mask(kind, n, R, seed=0):
    """fp32 [n, R] of {0, 1}.  'patterns': pool_cases.make_mask under clamp_zero -- a candidate with no valid row, one with only the
    first, one with only the last, one with all (n >= 4)"""
    if kind == 'zero':
        return torch.zeros(n, R)
    if kind == 'full':
        return torch.ones(n, R)
    if kind == 'patterns':
        assert n >= 4
        return PC.make_mask(n, R, False, 1, seed)
    if kind == 'straddle':
        assert n * R > max(STRADDLE_IDS)
        m = torch.zeros(n * R)
        m[list(STRADDLE_IDS)] = 1.0
        return m.view(n, R)
    dens = {'sparse': 0.3, 'dense90': 0.9}[kind]
    return (torch.rand(n, R, generator=gen(kind, 31 * n + R + seed)) < dens).float()


def philox_units(ids):
    """per four-row unit of a compact row list: the sizes of its runs of equal Philox block (id >> 2)"""
    out = []
    for i in range(0, len(ids), 4):
        blk = [int(x) >> 2 for x in ids[i:i + 4]]
        runs = []
        for j, b in enumerate(blk):
            if j and b == blk[j - 1]:
                runs[-1] += 1
            else:
                runs.append(1)
        out.append(tuple(runs))
    return out


@dataclasses.dataclass(frozen=True)
class Head:
    """one head of a call.  plain: group 1 at row 0 of every candidate; pooled: group R at rows 1 .. R.  ``mask``: None = every row
    computed (no row map), else the kind of mask the compact row list is built from.  ``segs``: ((in_off, in_dim), ...)"""
    kind: str
    J: int
    segs: tuple
    R: int = 1
    mask: str = None
    planes: bool = False
    empty: bool = False          # the indexed ops only: rows = 0

    @property
    def group(self):
        return self.R if self.kind == 'pooled' else 1

    @property
    def goff(self):
        return 1 if self.kind == 'pooled' else 0

    @property
    def nseg(self):
        return len(self.segs)


def head_rows(h, n, rp1, seed=0):
    """(mask or None, L, prow, cstart): the logical ids of the rows the head computes in dZ1 / H1 row order, their physical rows in
    the [n * rp1] block, and the compact form's candidate starts"""
    rows = n * h.group
    if h.mask is None:
        mask, cstart = None, None
        L = torch.arange(rows, dtype=torch.long)
    else:
        mask = make_mask(h.mask, n, h.R, seed)
        rm, cstart, cnt, _ = PC.compact_ref(mask)
        L = rm.long()
        assert L.numel() == cnt
    prow = (L // h.group) * rp1 + h.goff + L % h.group
    return mask, L, prow, cstart


def make_dz(rows, h, g):
    """fp32 [rows, nseg J]: segment s scaled by SEG_SCALE[s]"""
    dz = torch.randn(rows, h.nseg * h.J, generator=g)
    for s in range(h.nseg):
        dz[:, s * h.J:(s + 1) * h.J] *= SEG_SCALE[s]
    return dz


def split_planes(a):
    """fp32 -> (hi, lo) bf16: hi = rne(a), lo = rne(a - hi)"""
    hi = a.to(torch.bfloat16)
    lo = (a - hi.float()).to(torch.bfloat16)
    return hi, lo


def make_w1(h, g):
    return [torch.randn(h.J, d, generator=g) / d ** 0.5 for _, d in h.segs]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lirec_embed_dx
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class DxCase:
    name: str
    n: int
    rp1: int
    D: int
    heads: tuple

    @property
    def id(self):
        return self.name


GAPS_A = ((1, 4), (7, 132), (142, 4), (154, 8))      # gaps [0,1) [5,7) [139,142) [146,154) [162,164): widths 1 2 3 8 2
GAPS_B = ((8, 4), (17, 4), (24, 8), (34, 4))         # gaps [0,8) [12,17) [21,24) [32,34) [38,164): widths 8 5 3 2 126
GAPS_D = 164


def head_gaps(h, D):
    """[(start, width)] of the column gaps of a head inside [0, D)"""
    out, at = [], 0
    for off, dim in h.segs:
        if off > at:
            out.append((at, off - at))
        at = max(at, off + dim)
    if at < D:
        out.append((at, D - at))
    return out


DX_CASES = [
    # plain heads: rows 1 / 127 / 128 / 129 / 300, J 4 / 36 / 100 / 256, widths 4 / 132 / 256
    DxCase('plain-n1-rp1_1-J4-w4+132', 1, 1, 136, (Head('plain', 4, ((0, 4), (4, 132))),)),
    DxCase('plain-n127-J36-w132+256+4', 127, 2, 392, (Head('plain', 36, ((0, 132), (132, 256), (388, 4))),)),
    DxCase('plain-n128-J100-w256+4', 128, 3, 260, (Head('plain', 100, ((0, 256), (256, 4))),)),
    DxCase('plain-n129-J256-w4+132', 129, 2, 136, (Head('plain', 256, ((0, 4), (4, 132))),)),
    DxCase('plain-n300-rp1_1-J36-gapsA', 300, 1, GAPS_D, (Head('plain', 36, GAPS_A),)),
    # pooled heads alone (row 0 of every candidate has no owner), without a row map
    DxCase('pooled-dense-R1-n129-J100', 129, 2, 136, (Head('pooled', 100, ((0, 132), (132, 4)), R=1),)),
    DxCase('pooled-dense-R3-n43-rp1_6-J36', 43, 6, 136, (Head('pooled', 36, ((0, 4), (4, 132)), R=3),)),
    DxCase('pooled-dense-R18-n7-J4', 7, 19, 260, (Head('pooled', 4, ((0, 256), (256, 4)), R=18),)),
    # ... and compact
    DxCase('pooled-compact-R3-n9-J4-patterns', 9, 4, 136, (Head('pooled', 4, ((0, 4), (4, 132)), R=3, mask='patterns'),)),
    DxCase('pooled-compact-R18-n17-J36-patterns', 17, 19, 136, (Head('pooled', 36, ((0, 132), (132, 4)), R=18, mask='patterns'),)),
    DxCase('pooled-compact-R1-n300-J4-dense90', 300, 2, 136, (Head('pooled', 4, ((0, 4), (4, 132)), R=1, mask='dense90'),)),
    DxCase('pooled-compact-R1-n127-J100-full', 127, 3, 260, (Head('pooled', 100, ((0, 256), (256, 4)), R=1, mask='full'),)),
    DxCase('pooled-compact-R18-n8-J36-allmasked', 8, 19, 136, (Head('pooled', 36, ((0, 132), (132, 4)), R=18, mask='zero'),)),
    DxCase('pooled-compact-R18-n8-J100-full', 8, 20, 136, (Head('pooled', 100, ((0, 4), (4, 132)), R=18, mask='full'),)),
    # both heads in one call
    DxCase('both-n17-rp1_21-J36-gapsA+B-compactR18', 17, 21, GAPS_D,
           (Head('plain', 36, GAPS_A), Head('pooled', 36, GAPS_B, R=18, mask='patterns'))),
    DxCase('both-n128-J256-w256+132-denseR3', 128, 4, 388,
           (Head('plain', 256, ((0, 256), (256, 132))), Head('pooled', 256, ((0, 256), (256, 132)), R=3))),
    DxCase('both-n9-rp1_5-J4-allmasked+plain', 9, 5, 136,
           (Head('pooled', 4, ((0, 4), (4, 132)), R=3, mask='zero'), Head('plain', 4, ((0, 132), (132, 4))))),
]
# the pooled head on the bf16 hi / lo planes (gemm modes 2 and 3 only), a plain fp32 head of the same J in the same call
DX_PLANES = DxCase('planes-n5-J256-w256+256-compactR3+plain', 5, 4, 512,
                   (Head('plain', 256, ((0, 256), (256, 256)), planes=True),
                    Head('pooled', 256, ((0, 256), (256, 256)), R=3, mask='sparse', planes=True)))


@functools.lru_cache(maxsize=None)
def dx_inputs(case, operand='f32'):
    """``operand`` of the heads with ``planes``' pooled form: 'f32' (none), 'hilo' (dZ1 = hi + lo), 'hi' (dZ1 = hi, lo never read).
    Returns a dict: per head dz (what the device multiplies, fp32), hi / lo planes or None, W1, mask, L, prow, cstart; and the
    reference ``ref`` / ``absprod`` [n rp1, D] float64, ``written`` bool, ``blocks`` [(head, seg, prow, off, dim, K)]"""
    g = gen(case.name)
    n, rp1, D = case.n, case.rp1, case.D
    ref = torch.zeros(n * rp1, D, dtype=torch.float64)
    absprod = torch.zeros_like(ref)
    written = torch.zeros(n * rp1, D, dtype=torch.bool)
    heads, blocks = [], []
    for hi_, h in enumerate(case.heads):
        mask, L, prow, cstart = head_rows(h, n, rp1, seed=hi_)
        dz = make_dz(L.numel(), h, g)
        hi = lo = None
        if h.planes and h.kind == 'pooled' and operand != 'f32':
            hi, lo = split_planes(dz)
            dz = hi.float() + lo.float() if operand == 'hilo' else hi.float()
        W1 = make_w1(h, g)
        for s, (off, dim) in enumerate(h.segs):
            a = dz[:, s * h.J:(s + 1) * h.J].double()
            w = W1[s].double()
            assert not bool(written[prow, off:off + dim].any()), 'two writers'
            ref[prow, off:off + dim] = a @ w
            absprod[prow, off:off + dim] = a.abs() @ w.abs()
            written[prow, off:off + dim] = True
            blocks.append((hi_, s, prow, off, dim, h.J))
        heads.append(dict(h=h, dz=dz, hi=hi, lo=lo, W1=W1, mask=mask, L=L, prow=prow, cstart=cstart))
    return dict(case=case, heads=heads, ref=ref, absprod=absprod, written=written, blocks=blocks)


def check_dx(got, inp, mode, tag, ref=None):
    """``got``: the fp32 block after the call (pre-filled with NaN), on the CPU.  Exact zeros wherever no problem writes, each
    (head, segment) block within the core's bound of its own scale."""
    case = inp['case']
    got = got.reshape(case.n * case.rp1, case.D)
    ref = inp['ref'] if ref is None else ref
    un = got[~inp['written']]
    assert bits_zero(un), '%s: %d of %d elements no head writes are not +0' % (tag, int((un.view(torch.int32) != 0).sum()), un.numel())
    for hi_, s, prow, off, dim, K in inp['blocks']:
        if prow.numel() == 0:
            continue
        r = ref[prow, off:off + dim]
        close(got[prow, off:off + dim], r, bound(mode, r, inp['absprod'][prow, off:off + dim], K), '%s dX h%d s%d' % (tag, hi_, s))


def check_dx_bf16(got16, got32, tag):
    """the bf16 leaf: the same accumulators rounded once to nearest even"""
    assert bool(torch.isfinite(got32).all()), tag + ': the fp32 block is not finite everywhere'
    want = got32.to(torch.bfloat16)
    same = got16.contiguous().view(torch.int16) == want.contiguous().view(torch.int16)
    assert bool(same.all()), '%s: %d bf16 elements are not the fp32 result rounded to nearest even' % (tag, int((~same).sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lirec_embed_dx_indexed
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class DxiCase:
    name: str
    n_clip: int
    n_track: int
    td: int
    vd: int
    kd: int
    J: int
    rows: tuple                  # per head: its ``rows`` argument (0: the head reads no piece, its S is NaN)

    @property
    def id(self):
        return self.name


DXI_CASES = [
    DxiCase('nc1-nt127-w4+132+256-J4-1head', 1, 127, 4, 132, 256, 4, (5,)),
    DxiCase('nc127-nt128-w132+256+4-J36-2heads', 127, 128, 132, 256, 4, 36, (5, 7)),
    DxiCase('nc128-nt129-w256+4+132-J256-2heads', 128, 129, 256, 4, 132, 256, (5, 7)),
    DxiCase('nc129-nt1-w4+4+4-J36-1head', 129, 1, 4, 4, 4, 36, (5,)),
    DxiCase('nc128-nt127-w132+4+132-J36-head0_empty', 128, 127, 132, 4, 132, 36, (0, 7)),
    DxiCase('nc129-nt128-w4+132+4-J4-both_empty', 129, 128, 4, 132, 4, 4, (0, 0)),
]


@functools.lru_cache(maxsize=None)
def dxi_inputs(case):
    g = gen(case.name)
    c = case
    nc1, nt1, J = c.n_clip + 1, c.n_track + 1, c.J
    dims = (c.td, c.vd, c.kd, c.kd)
    S, W1 = [], []
    for r in c.rows:
        s = torch.randn((nc1 + nt1) * 2 * J, generator=g)           # (the trailing rows non-zero on purpose)
        S.append(s if r else torch.full_like(s, NAN))
        W1.append([torch.randn(J, d, generator=g) / d ** 0.5 for d in dims])
    return dict(case=c, S=S, W1=W1, **dxi_ref(c, S, W1))


def dxi_ref(c, S, W1, trailing_is_piece=False):
    """float64 dClip [n_clip + 1, td + vd] / dTrack [n_track + 1, kd], |A| |B| sums, K per problem.  ``trailing_is_piece``: a wrong
    reference for the host test -- the tables' zero rows computed like pieces"""
    nc1, nt1, J = c.n_clip + 1, c.n_track + 1, c.J
    dC = torch.zeros(nc1, c.td + c.vd, dtype=torch.float64)
    dT = torch.zeros(nt1, c.kd, dtype=torch.float64)
    aC, aT = torch.zeros_like(dC), torch.zeros_like(dT)
    act = 0
    for r, s, w in zip(c.rows, S, W1):
        if not r:
            continue
        act += 1
        Sc = s[:nc1 * 2 * J].view(nc1, 2 * J).double().clone()
        St = s[nc1 * 2 * J:].view(nt1, 2 * J).double().clone()
        if not trailing_is_piece:
            Sc[-1] = 0
            St[-1] = 0
        w = [x.double() for x in w]
        dC[:, :c.td] += Sc[:, :J] @ w[0]; aC[:, :c.td] += Sc[:, :J].abs() @ w[0].abs()
        dC[:, c.td:] += Sc[:, J:] @ w[1]; aC[:, c.td:] += Sc[:, J:].abs() @ w[1].abs()
        dT += St[:, :J] @ w[2] + St[:, J:] @ w[3]
        aT += St[:, :J].abs() @ w[2].abs() + St[:, J:].abs() @ w[3].abs()
    return dict(dClip=dC, dTrack=dT, aClip=aC, aTrack=aT, K_clip=act * J, K_track=2 * act * J, active=act)


def check_dxi(dClip, dTrack, inp, mode, tag, ref=None):
    c = inp['case']
    ref = inp if ref is None else ref
    assert bits_zero(dClip[c.n_clip]) and bits_zero(dTrack[c.n_track]), tag + ': a trailing zero row is not +0'
    if inp['active'] == 0:
        assert bits_zero(dClip) and bits_zero(dTrack), tag + ': no head reads a piece, yet not every element is +0'
        return
    for got, r, a, K, what in ((dClip[:c.n_clip, :c.td], ref['dClip'][:c.n_clip, :c.td], inp['aClip'][:c.n_clip, :c.td], inp['K_clip'], 'text'),
                               (dClip[:c.n_clip, c.td:], ref['dClip'][:c.n_clip, c.td:], inp['aClip'][:c.n_clip, c.td:], inp['K_clip'], 'visual'),
                               (dTrack[:c.n_track], ref['dTrack'][:c.n_track], inp['aTrack'][:c.n_track], inp['K_track'], 'track')):
        close(got, r, bound(mode, r, a, K), '%s d%s' % (tag, what))


# ---------------------------------------------------------------------------------------------------------------------------
# the index of the piece-table ops
# ---------------------------------------------------------------------------------------------------------------------------
def make_index(n, rp1, n_clip, n_track, g):
    """int32 [n, rp1, 3] in [-1, n_piece).  Track piece 0 is track-1 of EVERY row; with three or more pieces the last clip piece
    and the last track piece are named by no row; about a fifth of the clip and track-2 entries are negative."""
    def draw(np_):
        hi = np_ - 1 if np_ >= 3 else np_
        v = torch.randint(0, hi, (n, rp1), generator=g)
        return torch.where(torch.rand(n, rp1, generator=g) < 0.2, torch.full_like(v, -1), v)
    idx = torch.stack([draw(n_clip), torch.zeros(n, rp1, dtype=torch.long), draw(n_track)], 2)
    idx[0, :, 0] = -1                       # (the first candidate: the null clip piece for certain, whichever head owns the row)
    idx[0, :, 2] = -1
    return idx.to(torch.int32)


def expand_rows(idx_rows, clip, track, td):
    """float64 [rows, td + vd + 2 kd]: the tables expanded through the index rows [rows, 3] (a negative entry: zeros)"""
    def take(tab, ix):
        out = tab.double()[ix.clamp_min(0).long()]
        return out * (ix >= 0).double().unsqueeze(1)
    return torch.cat([take(clip, idx_rows[:, 0]), take(track, idx_rows[:, 1]), take(track, idx_rows[:, 2])], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. lirec_embed_dw1_indexed
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Dw1Case:
    name: str
    n: int
    rp1: int
    heads: tuple                 # Head(kind, J, (), R, mask, empty): the segments are the pieces'
    n_clip: int
    n_track: int
    td: int
    vd: int
    kd: int
    overwrite: bool

    @property
    def id(self):
        return self.name

    @property
    def J(self):
        return self.heads[0].J

    @property
    def dims(self):
        return (self.td, self.vd, self.kd, self.kd)

    @property
    def ldp(self):
        return (self.n_clip + 1 + 2 * (self.n_track + 1) + 3) // 4 * 4


ONEHOT_STRIDE_ROWS = 174763          # 2048 workgroups x 256 threads / 3 entries per row: above it onehot_kernel's loop runs again


def _ih(kind, J, R=1, mask=None, empty=False):
    return Head(kind, J, (), R=R, mask=mask, empty=empty)


DW1_CASES = [
    Dw1Case('plain-n50-J36-nc5-nt6-w4+132+4-acc', 50, 3, (_ih('plain', 36),), 5, 6, 4, 132, 4, False),
    Dw1Case('compactR3+plain-n9-J4-nc3-nt3-w132+4+132-overwrite', 9, 4, (_ih('pooled', 4, 3, 'patterns'), _ih('plain', 4)), 3, 3, 132, 4, 132, True),
    Dw1Case('compactR18-n17-J36-nc7-nt4-w4+4+132-acc', 17, 19, (_ih('pooled', 36, 18, 'patterns'),), 7, 4, 4, 4, 132, False),
    Dw1Case('plain-n175000-rp1_1-J4-nc1-nt1-w4-acc-onehot_stride', 175000, 1, (_ih('plain', 4),), 1, 1, 4, 4, 4, False),
    Dw1Case('plain+empty-n33-J256-nc130-nt2-w256+4+132-acc', 33, 2, (_ih('plain', 256), _ih('pooled', 256, 1, None, True)), 130, 2, 256, 4, 132, False),
    Dw1Case('empty+compactR3-n9-J36-nc4-nt5-w4+132+4-overwrite', 9, 4, (_ih('plain', 36, empty=True), _ih('pooled', 36, 3, 'sparse')), 4, 5, 4, 132, 4, True),
    # the all-masked batch: count = 0, S and the head's gradient are zeros (overwrite mode), the plain head beside it is not disturbed
    Dw1Case('allmaskedR3+plain-n9-J36-nc4-nt5-w4+132+4-overwrite', 9, 4, (_ih('pooled', 36, 3, 'zero'), _ih('plain', 36)), 4, 5, 4, 132, 4, True),
]


def make_tables(c, g):
    """piece tables with their trailing zero rows"""
    clip = torch.randn(c.n_clip + 1, c.td + c.vd, generator=g)
    track = torch.randn(c.n_track + 1, c.kd, generator=g)
    clip[-1] = 0
    track[-1] = 0
    return clip, track


def s_ref(dz, idx_rows, n_clip, n_track, J):
    """float64 (S, |S| sums) [(n_clip + 1) + (n_track + 1), 2J]: per piece the sum of the dZ1 rows whose index names it, the null
    piece's row last in each table"""
    nc1, nt1 = n_clip + 1, n_track + 1
    out = []
    for d in (dz.double(), dz.double().abs()):
        Sc = torch.zeros(nc1, 2 * J, dtype=torch.float64)
        St = torch.zeros(nt1, 2 * J, dtype=torch.float64)
        src = [torch.where(idx_rows[:, k] < 0, torch.full_like(idx_rows[:, k], n_clip if k == 0 else n_track), idx_rows[:, k]).long()
               for k in range(3)]
        Sc.index_add_(0, src[0], d[:, :2 * J])
        St[:, :J] = torch.zeros(nt1, J, dtype=torch.float64).index_add_(0, src[1], d[:, 2 * J:3 * J])
        St[:, J:] = torch.zeros(nt1, J, dtype=torch.float64).index_add_(0, src[2], d[:, 3 * J:])
        out.append(torch.cat([Sc, St], 0))
    return out


@functools.lru_cache(maxsize=None)
def dw1_inputs(case):
    c = case
    g = gen(c.name)
    J = c.J
    clip, track = make_tables(c, g)
    index = make_index(c.n, c.rp1, c.n_clip, c.n_track, g)
    flat = index.view(c.n * c.rp1, 3)
    heads = []
    for hi_, h in enumerate(c.heads):
        hh = dataclasses.replace(h, segs=((0, c.td), (c.td, c.vd), (c.td + c.vd, c.kd), (c.td + c.vd + c.kd, c.kd)))
        g0W = [torch.randn(J, d, generator=g) * 0.5 for d in c.dims]
        g0b = [torch.randn(J, generator=g) * 0.5 for _ in c.dims]
        if h.empty:
            heads.append(dict(h=hh, empty=True, g0W=g0W, g0b=g0b))
            continue
        mask, L, prow, cstart = head_rows(hh, c.n, c.rp1, seed=hi_)
        dz = make_dz(L.numel(), hh, g)
        ix = flat[prow]
        S, aS = s_ref(dz, ix, c.n_clip, c.n_track, J)
        X = expand_rows(ix, clip, track, c.td)
        d64 = dz.double()
        dW, aW, db, ab = [], [], [], []
        for s, (off, dim) in enumerate(hh.segs):
            z = d64[:, s * J:(s + 1) * J]
            ini_w = 0.0 if c.overwrite else g0W[s].double()
            ini_b = 0.0 if c.overwrite else g0b[s].double()
            dW.append(z.t() @ X[:, off:off + dim] + ini_w)
            aW.append(z.abs().t() @ X[:, off:off + dim].abs() + (ini_w.abs() if not c.overwrite else 0.0))
            db.append(z.sum(0) + ini_b)
            ab.append(z.abs().sum(0) + (ini_b.abs() if not c.overwrite else 0.0))
        heads.append(dict(h=hh, empty=False, dz=dz, mask=mask, L=L, prow=prow, cstart=cstart, ix=ix, S=S, aS=aS, dW=dW, aW=aW, db=db,
                          ab=ab, g0W=g0W, g0b=g0b))
    return dict(case=c, clip=clip, track=track, index=index, heads=heads)


def check_dw1(got_S, got_dW, got_db, hd, c, mode, tag):
    """one head: S (every row of both tables, the null rows included), dW1 and db1 of the four segments"""
    rows = hd['L'].numel()
    nc1, nt1, J = c.n_clip + 1, c.n_track + 1, c.J
    got_S = got_S.view(nc1 + nt1, 2 * J)
    # (S per table part against its own scale: the segments of dZ1 are scaled apart)
    for r0, r1, c0, c1, what in ((0, nc1, 0, J, 'text'), (0, nc1, J, 2 * J, 'visual'), (nc1, nc1 + nt1, 0, J, 'track-1'),
                                 (nc1, nc1 + nt1, J, 2 * J, 'track-2')):
        r = hd['S'][r0:r1, c0:c1]
        close(got_S[r0:r1, c0:c1], r, bound(mode, r, hd['aS'][r0:r1, c0:c1], rows), '%s S %s' % (tag, what))
    for s in range(4):
        K = rows + (nc1 if s < 2 else nt1)
        close(got_dW[s], hd['dW'][s], bound(mode, hd['dW'][s], hd['aW'][s], K), '%s dW1[%d]' % (tag, s))
        close(got_db[s], hd['db'][s], bound(mode, hd['db'][s], hd['ab'][s], K), '%s db1[%d]' % (tag, s))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. lirec_embed_l1_indexed
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class L1Case:
    name: str
    n: int
    rp1: int
    head: Head
    n_clip: int
    n_track: int
    td: int
    vd: int
    kd: int
    p: float
    site: int = 1

    @property
    def id(self):
        return self.name

    @property
    def dims(self):
        return (self.td, self.vd, self.kd, self.kd)


GATHER_STRIDE_ROWS = 1024            # gather_act_kernel: at most 256 row groups of 4 per sweep
L1_CASES = [
    L1Case('plain-n5-rp1_2-nc1-nt1-w4+132+4-p0', 5, 2, _ih('plain', 256), 1, 1, 4, 132, 4, 0.0),
    L1Case('plain-n1030-rp1_1-nc7-nt5-w132+4+132-p0.3-stride', 1030, 1, _ih('plain', 256), 7, 5, 132, 4, 132, 0.3, site=0),
    L1Case('compactR18-n4-straddle-nc1-nt3-w4+4+132-p0.3', 4, 19, _ih('pooled', 256, 18, 'straddle'), 1, 3, 4, 4, 132, 0.3),
    L1Case('compactR18-n4-straddle-nc3-nt1-w132+4+4-p0', 4, 19, _ih('pooled', 256, 18, 'straddle'), 3, 1, 132, 4, 4, 0.0),
    L1Case('compactR3-n9-patterns-nc5-nt4-w4+132+4-p0.3', 9, 4, _ih('pooled', 256, 3, 'patterns'), 5, 4, 4, 132, 4, 0.3),
    L1Case('compactR18-n80-dense90-nc9-nt6-w4+4+4-p0.3-stride', 80, 19, _ih('pooled', 256, 18, 'dense90'), 9, 6, 4, 4, 4, 0.3),
]


@functools.lru_cache(maxsize=None)
def l1_inputs(case):
    """tables, index, W1 / b1 and the float64 pre-activations ``pre`` [computed rows, 4J] with their |x| |w| + |b| sums"""
    c = case
    g = gen(c.name)
    J = c.head.J
    hh = dataclasses.replace(c.head, segs=((0, c.td), (c.td, c.vd), (c.td + c.vd, c.kd), (c.td + c.vd + c.kd, c.kd)))
    clip, track = make_tables(c, g)
    index = make_index(c.n, c.rp1, c.n_clip, c.n_track, g)
    mask, L, prow, cstart = head_rows(hh, c.n, c.rp1)
    W1 = make_w1(hh, g)
    b1 = [torch.randn(J, generator=g) * 0.1 for _ in c.dims]
    ix = index.view(c.n * c.rp1, 3)[prow]
    X = expand_rows(ix, clip, track, c.td)
    pre = torch.cat([X[:, o:o + d] @ w.double().t() + b.double() for (o, d), w, b in zip(hh.segs, W1, b1)], 1)
    ab = torch.cat([X[:, o:o + d].abs() @ w.double().abs().t() + b.double().abs() for (o, d), w, b in zip(hh.segs, W1, b1)], 1)
    Kcol = torch.cat([torch.full((J,), float(d), dtype=torch.float64) for d in c.dims])
    return dict(case=c, h=hh, clip=clip, track=track, index=index, mask=mask, L=L, prow=prow, cstart=cstart, W1=W1, b1=b1, ix=ix,
                pre=pre, absprod=ab, Kcol=Kcol)


def h1_ref(inp, keep_rows):
    """float64 H1 of the computed rows: ``keep_rows`` [computed rows, 4J] = the keep decisions at the rows' ORIGINAL ids"""
    sc = PC.drop_scale(inp['case'].p)
    return torch.relu(inp['pre']) * keep_rows.double() * sc


def check_h1(got, inp, keep_rows, mode, tag, relu_eps, relu_frac):
    """``got``: the device's H1 at the computed rows (CPU).  Relu decisions may differ from the float64 ones only where the
    pre-activation is within ``relu_eps`` of 0, on at most 8 + ``relu_frac`` of the elements; everything else at the bound."""
    assert bool(torch.isfinite(got).all()), tag + ': H1 not written at a computed row'
    ref = h1_ref(inp, keep_rows)
    kept = keep_rows.bool()
    diff = ((got > 0) != (ref > 0)) & kept
    if bool(diff.any()):
        worst = float(inp['pre'][diff].abs().max())
        assert worst <= relu_eps, '%s: a relu decision differs at |z| = %.3e' % (tag, worst)
        assert int(diff.sum()) <= 8 + relu_frac * diff.numel(), '%s: %d relu decisions differ' % (tag, int(diff.sum()))
    assert bits_zero(got[~kept]), tag + ': a dropped element is not +0'
    sc = PC.drop_scale(inp['case'].p)
    if mode in (0, 1):
        bnd = (inp['Kcol'].unsqueeze(0) + 4.0) * U * inp['absprod'] * sc + TINY
    else:
        bnd = SPLIT_RTOL * ref.abs() + SPLIT_STOL * float(ref.abs().max()) + TINY
    ok = ~diff
    close(got[ok], ref[ok], bnd[ok], tag + ' H1')
    return int(diff.sum())


def near_zero(inp, relu_eps):
    """how many float64 pre-activations lie within relu_eps of 0"""
    return int((inp['pre'].abs() <= relu_eps).sum())
