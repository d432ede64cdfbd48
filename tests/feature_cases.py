"""Cases and host restatements for the kernels that PRODUCE the features (tests/test_gpu_feature_path.py runs them on the device,
tests/test_host_feature_cases.py proves on the CPU that the tables hold what they claim):

  grid_pool_kernel, rows_max_kernel            raw pooling, against oracle/rawfeat_oracle.py (numpy), bit for bit
  gather_features_kernel                       fp32 / float64 tables -> fp32 / bf16 rows, against torch index_select
  to_q32b_kernel, to_q16b_kernel,              the storage writers, against the formats as gemm_bf16x3.hpp documents them
  q32b_write_rows_kernel<float|double>
  dropout_mask_kernel                          against oracle/lirec_oracle.py dropout_keep_mask

Everything here runs on the CPU; the references are computed once per process and never modified."""
import functools
import os
import warnings
from collections import defaultdict, namedtuple

import numpy as np
import torch

from lirec_amd import rawfeat as RF
from oracle import rawfeat_oracle as RO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CAP_ITEMS = 8192 * 256                 # work items of a capped grid: above it a thread takes its stride loop


def bits_equal(a, b):
    """same shape, NaN in the same places, the same BITS elsewhere (so -0.0 is not +0.0)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. grid_pool
# ---------------------------------------------------------------------------------------------------------------------------
Box = namedtuple('Box', 'frame y0 y1 x0 x1 where')
SPECIAL_C = 200                        # the channel that holds +inf, -inf and NaN
N_CLASSES = (1, 7, 8, 9, 15, 16, 127, 128, 129, 136, 255, 256, 257, 264, 513, 667)

# (h, w) per box size.  The 23 x 29 grid of the issue cannot hold 127 and 257 cells (primes above 29) nor 129 (3 x 43) as a
# rectangle: those sizes -- and 1089, a fourth level of the halving -- live on a second, 259 x 259 grid of 8 channels.
MAIN_SHAPES = {1: [(1, 1)] * 5, 7: [(1, 7), (7, 1)], 8: [(1, 8), (8, 1), (2, 4), (4, 2)], 9: [(1, 9), (9, 1), (3, 3)],
               15: [(1, 15), (15, 1), (3, 5), (5, 3)], 16: [(1, 16), (16, 1), (4, 4), (2, 8)], 128: [(8, 16), (16, 8)],
               136: [(8, 17), (17, 8)], 255: [(15, 17), (17, 15)], 256: [(16, 16)], 264: [(12, 22), (22, 12), (11, 24)],
               513: [(19, 27)], 667: [(23, 29)]}
WIDE_SHAPES = {127: [(1, 127), (127, 1)], 129: [(1, 129), (129, 1), (3, 43), (43, 3)], 257: [(1, 257), (257, 1)],
               1089: [(33, 33)]}
PLACES = ('top-left', 'top-right', 'bottom-left', 'bottom-right', 'interior')


def place_boxes(shapes, F, H, W):
    out, k = [], 0
    for n in sorted(shapes):
        for h, w in shapes[n]:
            assert h * w == n and h <= H and w <= W
            where = PLACES[k % 5]
            y0 = {'top': 0, 'bot': H - h, 'int': min(max((H - h) // 2 + 1, 0), H - h)}[where[:3]]
            x0 = 0 if where.endswith('left') else (W - w if where.endswith('right') else min((W - w) // 2 + 1, W - w))
            out.append(Box(k % F, y0, y0 + h, x0, x0 + w, where))
            k += 1
    return out


PoolGrid = namedtuple('PoolGrid', 'name grid boxes')


@functools.lru_cache(maxsize=None)
def pool_grids():
    rng = np.random.Generator(np.random.PCG64(2024))
    F, C, H, W = 3, 264, 23, 29
    g = rng.standard_normal((F, C, H, W)).astype(np.float32)
    g[2, :, 15:23, 0:8] = -np.abs(g[2, :, 15:23, 0:8]) - 0.01        # a region whose every box mean is negative in every channel
    g[0, SPECIAL_C, 2, 3] = np.inf
    g[1, SPECIAL_C, 10, 10] = -np.inf
    g[1, SPECIAL_C, 20, 25] = np.nan
    g[2, SPECIAL_C, 5, 5], g[2, SPECIAL_C, 5, 6] = np.inf, -np.inf   # both in one box: the sum is NaN
    g.setflags(write=False)
    w = rng.standard_normal((2, 8, 259, 259)).astype(np.float32)
    w.setflags(write=False)
    return (PoolGrid('main', g, tuple(place_boxes(MAIN_SHAPES, F, H, W))),
            PoolGrid('wide', w, tuple(place_boxes(WIDE_SHAPES, 2, 259, 259))))


NEG_BOX = [2, 16, 21, 1, 6]            # inside the all-negative region of frame 2


def pool_lists(pg):
    """The output lists of one grid: every box of the table alone, then (main grid) the list shapes of the kernel's element loop."""
    b = [list(x[:5]) for x in pg.boxes]
    lists = [[x] for x in b]
    names = ['%s %dx%d %s' % (pg.name, x.y1 - x.y0, x.x1 - x.x0, x.where) for x in pg.boxes]
    if pg.name != 'main':
        return lists, names
    F = pg.grid.shape[0]
    more = [('several', [b[5], b[12], b[20], b[31], b[33]]),
            ('frame -1 and >= F among valid', [[-1, 0, 3, 0, 3], b[7], [F, 0, 3, 0, 3], b[22], [F + 5, 1, 2, 1, 2]]),
            ('every element skipped', [[-1, 0, 3, 0, 3], [F, 2, 9, 2, 9]]),
            ('all-negative means + one skipped', [NEG_BOX, [2, 15, 23, 0, 8], [-1, 0, 1, 0, 1]]),
            ('all-negative means alone', [NEG_BOX, [2, 17, 18, 2, 3]]),
            ('empty box (y1 == y0) among valid', [b[6], [1, 5, 5, 3, 8], b[9]]),
            ('empty box (x1 < x0) among valid', [b[10], [0, 2, 6, 9, 4]]),
            ('before an empty list', [b[15], b[16]]),
            ('empty list', []),
            ('after an empty list', [b[17]])]
    return lists + [l for _, l in more], names + [n for n, _ in more]


@functools.lru_cache(maxsize=None)
def pool_reference(name):
    pg = {g.name: g for g in pool_grids()}[name]
    lists, names = pool_lists(pg)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                              # (np.mean of an empty crop, inf - inf)
        ref = RO.grid_pool(pg.grid, lists)
    ref.setflags(write=False)
    return lists, names, ref


def kernel_pairwise_sum(x):
    """np_pairwise_sum of kernels.hpp, restated in float32 numpy on [channels, n] (every channel sums as one device thread does):
    below 8 a plain loop; up to 128 eight accumulators over the whole groups of eight, combined as a tree, then the tail; above, two
    halves, the first rounded down to a multiple of eight."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[1]
    with np.errstate(all='ignore'):
        if n < 8:
            res = np.zeros(x.shape[0], dtype=np.float32)
            for i in range(n):
                res = res + x[:, i]
            return res
        if n <= 128:
            r = [x[:, j].copy() for j in range(8)]
            i = 8
            while i < n - n % 8:
                for j in range(8):
                    r[j] = r[j] + x[:, i + j]
                i += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            while i < n:
                res = res + x[:, i]
                i += 1
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return kernel_pairwise_sum(x[:, :n2]) + kernel_pairwise_sum(x[:, n2:])


def crop(grid, box):
    f, y0, y1, x0, x1 = box[:5]
    return grid[f][:, y0:y1, x0:x1].reshape(grid.shape[1], -1)


def kernel_box_mean(grid, box):
    x = crop(grid, box)
    with np.errstate(all='ignore'):
        return (kernel_pairwise_sum(x) / np.float32(x.shape[1])).astype(np.float32)


def recursion_levels(n):
    if n <= 128:
        return 0
    n2 = n // 2
    n2 -= n2 % 8
    return 1 + max(recursion_levels(n2), recursion_levels(n - n2))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. rows_max
# ---------------------------------------------------------------------------------------------------------------------------
ROWS_N, ROWS_LAYERS, ROWS_DIM, ROWS_LAYER = 40, 3, 264, 1


@functools.lru_cache(maxsize=None)
def rows_source():
    rng = np.random.Generator(np.random.PCG64(77))
    t = rng.standard_normal((ROWS_N, ROWS_LAYERS, ROWS_DIM)).astype(np.float32)
    v = t[:, ROWS_LAYER, :]
    v[30:35] = -np.abs(v[30:35]) - 0.01                              # all-negative rows
    v[30, 7] = v[31, 7] = -0.0                                       # -0.0 in every listed row: -0.0
    v[30, 8] = -0.0                                                  # -0.0 over negatives: -0.0
    # (no list pairs -0.0 with +0.0: IEEE leaves that maximum's sign open, and neither numpy nor fmaxf promises one)
    v[10, 100], v[11, 100], v[13, 100] = np.inf, -np.inf, -np.inf
    v[12, 260] = np.nan                                              # (in the second workgroup)
    v[14, 3], v[14, 4] = np.nan, np.inf
    t.setflags(write=False)
    return t


ROW_LISTS = [[], [0], [ROWS_N - 1], [3, 3, 3], [0, ROWS_N - 1, 17, 0], [30, 31, 32, 33, 34], [30, 31], [31, 30], [10, 11], [11, 10, 2],
             [11, 13], [12, 5], [5, 12], [10, 12, 14], [], [14], list(range(ROWS_N))]


@functools.lru_cache(maxsize=None)
def rows_reference():
    ref = RO.rows_max(rows_source()[:, ROWS_LAYER, :], ROW_LISTS)
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the fixtures the reference's own classes produced
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))


def fixture_tracks(FX):
    return [[{'frame': int(r[0]), 'x': r[1], 'y': r[2], 'w': r[3], 'h': r[4]} for r in FX['track/%d' % k]] for k in range(int(FX['n_tracks']))]


def bookkeeping(FX):
    """lirec_amd.rawfeat's host bookkeeping on a fixture's inputs (as tests/test_rawfeat.py does for the first scene)"""
    F, C, H, W = FX['grid'].shape
    time2frame = defaultdict(list)
    for frame, sec in enumerate(FX['frame2time']):
        time2frame[int(sec)].append(frame)
    sfr = float(FX['sampling_fr'])
    tnodes = [{'start': int(a), 'end': int(b)} for a, b in FX['time_nodes']]
    clip_frames = [RF.clip_frame_range(time2frame, t, F, sfr) for t in tnodes]
    clip_boxes = [[[f, 0, H, 0, W] for f in fr] for fr in clip_frames]
    tracks = fixture_tracks(FX)
    track_boxes = [RF.track_boxes(tr, tuple(FX['dims']), H, W, F, sfr) for tr in tracks]
    b = FX['token_bounds']
    ranges = [list(range(int(b[i]), int(b[i + 1]))) for i in range(len(b) - 1)]
    times = [(int(a), int(c)) for a, c in FX['dialog_times']]
    text_nodes = [{'start': int(a), 'end': int(c)} for a, c in FX['text_time_nodes']]
    tok_rows = [RF.token_rows(times, ranges, t) for t in text_nodes]
    return dict(clip_boxes=clip_boxes, track_boxes=track_boxes, tok_rows=tok_rows, time2frame=time2frame, tnodes=tnodes, tracks=tracks,
                times=times, ranges=ranges, text_nodes=text_nodes, sfr=sfr)


def raw_person_box(el, dims, H, W):
    """(ry, rx) BEFORE slicing, as visual_features.py:118-128 computes them -- what tells the host test which edge a fixture
    element stands for (a negative upper bound: the box ends left of / above the frame)"""
    sh, sw = H / dims[0], W / dims[1]
    fx, fy, fw, fh = el['x'] / 2., el['y'] / 2., el['w'] / 2., el['h'] / 2.
    pw, ph = fw / (0.65 - 0.35), fh / (0.25 - 0.10)
    px, py = fx - 0.35 * pw, fy - 0.10 * ph
    spx, spw, spy, sph = px * sw, pw * sw, py * sh, ph * sh
    return ([max(0, int(np.floor(spy))), min(int(H), int(np.ceil(spy + sph)))],
            [max(0, int(np.floor(spx))), min(int(W), int(np.ceil(spx + spw)))])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. gather_features
# ---------------------------------------------------------------------------------------------------------------------------
def f32_bits(*words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(torch.float32)


EXACT_BF16 = (0x3FC00000, 0xC0100000, 0x3A800000)                              # 1.5, -2.25, 2^-10
TIES = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x42FF8000)            # half an ulp above an even / an odd neighbour
NEAR_TIES = tuple(t + d for t in TIES[:2] for d in (-1, 1))                    # one fp32 ulp either side
ZEROS = (0x00000000, 0x80000000)
SUBNORMALS = (0x00000001, 0x007FFFFF, 0x80000001, 0x00008000, 0x00018000)      # (the last two are ties among subnormals)
BF16_SPECIALS = EXACT_BF16 + TIES + NEAR_TIES + ZEROS + SUBNORMALS + (0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000)
WRITER_SPECIALS = EXACT_BF16 + TIES + NEAR_TIES + ZEROS                        # finite, normal or zero: what the writers define
DOUBLE_ROUNDING = 1.0 + 2.0 ** -8 + 2.0 ** -30     # -> fp32 1 + 2^-8 (a tie) -> bf16 1.0; rounded to bf16 directly it is 1 + 2^-7

GatherCase = namedtuple('GatherCase', 'name rows clip_dim track_dim n_clip n_track pad_clip pad_track pad_out')
GATHER_SMALL = GatherCase('small', 37, 12, 20, 5, 7, 4, 8, 4)
GATHER_STRIDE = GatherCase('stride', 16400, 256, 128, 64, 48, 0, 0, 0)
PAD = 777.0                                        # the value of every padding column: never to be read, never to be written
SPECIAL_CLIP_ROW, SPECIAL_TRACK_ROW, DR_TRACK_ROW = 1, 3, 5


@functools.lru_cache(maxsize=None)
def gather_inputs(name, f64):
    """tables [n, dim + pad] (values in [:, :dim], PAD behind), index [rows, 3] int32"""
    c = {'small': GATHER_SMALL, 'stride': GATHER_STRIDE}[name]
    g = torch.Generator().manual_seed(31 if name == 'small' else 32)
    clip = torch.full((c.n_clip, c.clip_dim + c.pad_clip), PAD)
    track = torch.full((c.n_track, c.track_dim + c.pad_track), PAD)
    clip[:, :c.clip_dim] = torch.randn(c.n_clip, c.clip_dim, generator=g)
    track[:, :c.track_dim] = torch.randn(c.n_track, c.track_dim, generator=g)
    index = torch.stack([torch.randint(0, c.n_clip, (c.rows,), generator=g), torch.randint(0, c.n_track, (c.rows,), generator=g),
                         torch.randint(0, c.n_track, (c.rows,), generator=g)], 1).to(torch.int32)
    if name == 'small':
        sp = f32_bits(*BF16_SPECIALS)
        assert sp.numel() <= c.clip_dim + c.track_dim
        clip[SPECIAL_CLIP_ROW, :c.clip_dim] = sp[:c.clip_dim]
        track[SPECIAL_TRACK_ROW, :sp.numel() - c.clip_dim] = sp[c.clip_dim:]
        index[0] = torch.tensor([-1, SPECIAL_TRACK_ROW, 2])                      # -1 in each part alone,
        index[1] = torch.tensor([SPECIAL_CLIP_ROW, -1, SPECIAL_TRACK_ROW])
        index[2] = torch.tensor([SPECIAL_CLIP_ROW, DR_TRACK_ROW, -1])
        index[3] = torch.tensor([-1, -1, -1])                                    # in all three,
        index[4] = torch.tensor([c.n_clip - 1, c.n_track - 1, c.n_track - 1])    # the last table rows,
        index[10:26, 0] = 2                                                      # one piece used by many rows
        index[12:30, 2] = DR_TRACK_ROW
        index[c.rows - 1] = torch.tensor([c.n_clip - 1, SPECIAL_TRACK_ROW, -1])
    else:
        index[torch.rand(c.rows, 3, generator=g) < 0.1] = -1
        index[c.rows - 1] = torch.tensor([c.n_clip - 1, -1, c.n_track - 1])
    if f64:
        clip, track = clip.double(), track.double()
        if name == 'small':
            track[DR_TRACK_ROW, 0] = DOUBLE_ROUNDING
    return c, clip, track, index


def gather_reference(c, clip, track, index, out_dtype):
    """index_select on the tables, zeros where the index is negative, .float() for float64 tables, then the output type -- on
    whatever device the inputs live"""
    ix = index.long()
    parts = []
    for table, dim, col in ((clip, c.clip_dim, 0), (track, c.track_dim, 1), (track, c.track_dim, 2)):
        rows = table[:, :dim].index_select(0, ix[:, col].clamp_min(0)).float()
        parts.append(torch.where((ix[:, col] >= 0).unsqueeze(1), rows, torch.zeros_like(rows)))
    return torch.cat(parts, 1).to(out_dtype)


def raw_equal_but_nan(got, want):
    """bit identity, except that a NaN only has to be a NaN (torch writes one canonical NaN, the kernel keeps the sign bit)"""
    assert got.shape == want.shape and got.dtype == want.dtype
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        return False
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    return torch.equal(got.contiguous().view(it)[~gn], want.contiguous().view(it)[~wn])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. q32b / q16b
# ---------------------------------------------------------------------------------------------------------------------------
Q_SHAPES = ((1, 32), (31, 32), (33, 96), (37, 160), (64, 64))
Q_LD_SHAPE = (37, 160)                             # the one that also runs with ld_src = C + 4
Q_STRIDE_SHAPE = (8200, 2048)


def r32(R):
    return (R + 31) // 32 * 32


def split_hi_lo(x):
    """hi = bf16_rne(x), lo = bf16_rne(x - float(hi)), as int16 bit patterns (gemm_bf16x3.hpp: split4)"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def block_row(R, C, device='cpu'):
    """(r / 32 * (C / 32) + c / 32) * 32 + r % 32: the 32-column line of block (r / 32, c / 32) that holds element (r, c)"""
    r = torch.arange(R, device=device).view(-1, 1).expand(R, C)
    c = torch.arange(C, device=device).view(1, -1).expand(R, C)
    return (r // 32 * (C // 32) + c // 32) * 32 + r % 32, c % 32


def q32b_halfwords(R, C, device='cpu'):
    """half-word (2-byte) positions of the hi and the lo half of element (r, c): byte line * 128 + (c % 32) * 2, lo 64 bytes further"""
    line, c32 = block_row(R, C, device)
    hi = (line * 128 + c32 * 2) // 2
    return hi, hi + 32


def q16b_halfwords(R, C, device='cpu'):
    line, c32 = block_row(R, C, device)
    return (line * 64 + c32 * 2) // 2


def q32b_image(x):
    """the int16 image of lirec_to_q32b(x): R32 * C * 2 half-words, rows R .. R32 - 1 zero"""
    R, C = x.shape
    img = torch.zeros(r32(R) * C * 2, dtype=torch.int16, device=x.device)
    hi, lo = split_hi_lo(x)
    ih, il = q32b_halfwords(R, C, x.device)
    img[ih.reshape(-1)] = hi.reshape(-1)
    img[il.reshape(-1)] = lo.reshape(-1)
    return img


def q16b_image(x):
    R, C = x.shape
    img = torch.zeros(r32(R) * C, dtype=torch.int16, device=x.device)
    img[q16b_halfwords(R, C, x.device).reshape(-1)] = x.to(torch.bfloat16).view(torch.int16).reshape(-1)
    return img


def writer_values(R, C, seed):
    """normal finite fp32 with 2^-100 <= |x| <= 2^100 (so that the remainder x - hi is normal too), +-0 and the tie patterns"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, C, generator=g).clamp(-8, 8)
    x = torch.where(x.abs() < 2.0 ** -6, torch.full_like(x, 0.75), x)
    e = torch.randint(-94, 97, (R, C), generator=g)                  # |x| in [2^-6, 8] * 2^e, e in [-94, 96]
    x = torch.ldexp(x, e)
    sp = f32_bits(*WRITER_SPECIALS)
    pos = torch.randperm(R * C, generator=g)[:min(R * C, 3 * sp.numel())]
    x.view(-1)[pos] = sp.repeat(3)[:pos.numel()]
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# 6. dropout_mask
# ---------------------------------------------------------------------------------------------------------------------------
MASK_THREADS = 256 * 256
MASK_SHAPE = (1030, 67)
MASK_PS = (0.0, 0.5, 0.3)
MASK_SITES = (0, 5)
MASK_SEED = 0x1234ABCD5678EF01
CARRY_SEED = 0x00000001FFFFFFFF                    # + 1: the low word wraps and carries into the high word
