"""tests/feature_cases.py without a GPU: the tables hold every case they promise, the host restatements are what they claim to
be (the float32 restatement of the kernel's summation order IS np.mean; the q32b / q16b maps are bijections; the split loses at
most 2^-16 of a value), the numpy oracle is inside its derived float64 bound, and the second reference-made fixture agrees with
the oracle and with lirec_amd.rawfeat's bookkeeping."""
import numpy as np
import pytest
import torch

import feature_cases as FC
from lirec_amd import rawfeat as RF
from oracle import rawfeat_oracle as RO
from test_rawfeat import same


# ---------------------------------------------------------------------------------------------------------------------------
# raw pooling
# ---------------------------------------------------------------------------------------------------------------------------
def test_box_table_holds_every_size_class_shape_and_place():
    sizes, places, kinds = set(), set(), set()
    for pg in FC.pool_grids():
        F, C, H, W = pg.grid.shape
        for b in pg.boxes:
            h, w = b.y1 - b.y0, b.x1 - b.x0
            assert 0 <= b.frame < F and 0 <= b.y0 < b.y1 <= H and 0 <= b.x0 < b.x1 <= W, b
            sizes.add(h * w)
            kinds.add('1 x n' if h == 1 else ('n x 1' if w == 1 else 'rectangle'))
            if pg.name == 'main':
                at = (b.y0 == 0, b.y1 == H, b.x0 == 0, b.x1 == W)
                places.add({(True, False, True, False): 'top-left', (True, False, False, True): 'top-right',
                            (False, True, True, False): 'bottom-left', (False, True, False, True): 'bottom-right',
                            (False, False, False, False): 'interior'}.get(at, 'other'))
                assert w < W or h * w == H * W or h * w > (H - 1) * W, b       # narrower than the grid wherever the size allows
    assert sizes >= set(FC.N_CLASSES)
    assert kinds == {'1 x n', 'n x 1', 'rectangle'}
    assert places >= set(FC.PLACES)
    main = FC.pool_grids()[0]
    assert main.grid.shape == (3, 264, 23, 29) and main.grid.shape[1] > 256          # a second, partly filled workgroup in x
    # the paths of np_pairwise_sum: the plain loop, eight accumulators without / with a tail, 1 .. 3 levels of halving
    assert {n for n in sizes if n < 8} and {n for n in sizes if 8 <= n <= 128 and n % 8 == 0} and {n for n in sizes if 8 < n <= 128 and n % 8}
    assert {FC.recursion_levels(n) for n in sizes} >= {0, 1, 2, 3}
    assert FC.recursion_levels(136) == 1 and FC.recursion_levels(257) == 2 and FC.recursion_levels(513) == 3
    assert (136 // 2 - 136 // 2 % 8, 257 // 2 - 257 // 2 % 8, 513 // 2 - 513 // 2 % 8) == (64, 128, 256)


def test_output_lists_hold_every_list_shape():
    lists, names, ref = FC.pool_reference('main')
    F = FC.pool_grids()[0].grid.shape[0]
    by = dict(zip(names, range(len(names))))
    assert len(by) == len(names) == len(lists) == ref.shape[0]
    assert any(len(l) == 1 for l in lists) and len(lists[by['several']]) >= 3
    mixed = lists[by['frame -1 and >= F among valid']]
    assert {-1, F} <= {b[0] for b in mixed} and any(0 <= b[0] < F for b in mixed) and any(b[0] > F for b in mixed)
    skipped = by['every element skipped']
    assert all(not 0 <= b[0] < F for b in lists[skipped]) and ref[skipped].tobytes() == bytes(4 * ref.shape[1])     # zeros, not NaN
    neg = by['all-negative means + one skipped']
    assert ref[neg].tobytes() == bytes(4 * ref.shape[1])                                                           # the maximum is +0
    assert (ref[by['all-negative means alone']] < 0).all()
    for k in ('empty box (y1 == y0) among valid', 'empty box (x1 < x0) among valid'):
        assert np.isnan(ref[by[k]]).all() and any(b[2] <= b[1] or b[4] <= b[3] for b in lists[by[k]])
    e = by['empty list']
    assert lists[e] == [] and lists[e - 1] and lists[e + 1] and not ref[e].any() and ref[e - 1].any() and ref[e + 1].any()


def test_special_channel_is_the_only_one_with_non_finite_means():
    pg = FC.pool_grids()[0]
    lists, names, ref = FC.pool_reference('main')
    assert np.isfinite(np.delete(pg.grid, FC.SPECIAL_C, axis=1)).all()
    empty = np.array(['empty box' in n for n in names])
    others = np.delete(ref[~empty], FC.SPECIAL_C, axis=1)
    assert np.isfinite(others).all()
    col = ref[~empty][:, FC.SPECIAL_C]
    assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any() and np.isfinite(col).any()


@pytest.mark.parametrize('name', ['main', 'wide'])
def test_kernel_summation_order_is_np_mean_and_the_oracle_meets_its_float64_bound(name):
    """For every box of the table: (a) the float32 restatement of np_pairwise_sum / n equals np.mean's bits; (b) the oracle's mean
    lies within n * 2^-24 * mean|x| of the float64 mean -- (n - 1) u sum|x| for a recursive sum in any order plus one rounding of the
    quotient, u = 2^-24, divided by n."""
    pg = {g.name: g for g in FC.pool_grids()}[name]
    finite = np.ones(pg.grid.shape[1], dtype=bool)
    if name == 'main':
        finite[FC.SPECIAL_C] = False
    for b in pg.boxes:
        x = FC.crop(pg.grid, b)
        n = x.shape[1]
        with np.errstate(all='ignore'):
            want = np.mean(pg.grid[b.frame][:, b.y0:b.y1, b.x0:b.x1].reshape(1, pg.grid.shape[1], -1), axis=2)[0]
        assert want.dtype == np.float32
        assert FC.bits_equal(FC.kernel_box_mean(pg.grid, b), want), (b, n)
        x64 = x[finite].astype(np.float64)
        err = np.abs(want[finite].astype(np.float64) - x64.mean(axis=1))
        bound = n * 2.0 ** -24 * np.abs(x64).mean(axis=1)
        assert (err <= bound).all(), (b, float((err / bound).max()))
    lists, names, ref = FC.pool_reference(name)
    for o, b in enumerate(pg.boxes):                                   # the oracle's output row of a one-box list IS that mean
        assert FC.bits_equal(ref[o], FC.kernel_box_mean(pg.grid, b)), names[o]


def test_restated_summation_differs_from_a_plain_loop():
    """the comparison above can fail: a left-to-right float32 sum is NOT np.mean at these sizes"""
    pg = FC.pool_grids()[0]
    b = [x for x in pg.boxes if (x.y1 - x.y0) * (x.x1 - x.x0) == 513][0]
    x = np.delete(FC.crop(pg.grid, b), FC.SPECIAL_C, axis=0)
    plain = np.zeros(x.shape[0], dtype=np.float32)
    for i in range(x.shape[1]):
        plain = plain + x[:, i]
    assert not np.array_equal(plain / np.float32(513), FC.kernel_pairwise_sum(x) / np.float32(513))


def test_rows_max_lists_hold_every_row_kind():
    src = FC.rows_source()[:, FC.ROWS_LAYER, :]
    ref = FC.rows_reference()
    L = FC.ROW_LISTS
    assert not src.flags['C_CONTIGUOUS'] and src.shape == (40, 264)
    assert [] in L and [0] in L and [FC.ROWS_N - 1] in L and any(len(set(l)) < len(l) for l in L)
    assert L.index([]) < len(L) - 1 and L[L.index([]) + 1]
    neg = L.index([30, 31, 32, 33, 34])
    assert (ref[neg] <= 0).all() and (ref[neg] < 0).sum() >= 260
    z = L.index([30, 31])
    assert ref[z].view(np.uint32)[7] == 0x80000000 and ref[z].view(np.uint32)[8] == 0x80000000
    assert ref[L.index([10, 11]), 100] == np.inf and ref[L.index([11, 13]), 100] == -np.inf
    for l in (i for i, x in enumerate(L) if 12 in x):
        assert np.isnan(ref[l, 260]) and np.isfinite(np.delete(ref[l], [260, 3, 4, 100])).all()
    assert np.isnan(ref[L.index([14]), 3]) and ref[L.index([14]), 4] == np.inf
    for i, l in enumerate(L):
        if not l:
            assert ref[i].tobytes() == bytes(4 * FC.ROWS_DIM)
    for a, b in ((L.index([30, 31]), L.index([31, 30])), (L.index([12, 5]), L.index([5, 12]))):
        assert FC.bits_equal(ref[a], ref[b])                         # (no case depends on the order of the rows)


# ---------------------------------------------------------------------------------------------------------------------------
# the second fixture
# ---------------------------------------------------------------------------------------------------------------------------
def test_edges_fixture_matches_oracle_and_bookkeeping():
    FX = FC.fixture('rawfeat_edges')
    bk = FC.bookkeeping(FX)
    assert same(RO.grid_pool(FX['grid'], bk['clip_boxes']), FX['clip_visual'])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert same(RO.grid_pool(FX['grid'], bk['track_boxes']), FX['track'])
    assert same(RO.rows_max(FX['tokens'][:, -2, :], bk['tok_rows']), FX['clip_text'])


def test_edges_fixture_holds_the_edges():
    FX = FC.fixture('rawfeat_edges')
    F, C, H, W = FX['grid'].shape
    assert (F, C, H, W) == (4, 16, 13, 15)
    bk = FC.bookkeeping(FX)
    kinds = set()
    for tr, boxes in zip(bk['tracks'], bk['track_boxes']):
        for el, (f, y0, y1, x0, x1) in zip(tr, boxes):
            ry, rx = FC.raw_person_box(el, tuple(FX['dims']), H, W)
            assert 0 <= y0 and y1 <= H and 0 <= x0 and x1 <= W                   # what the device is handed lies inside the grid
            if f == -1:
                kinds.add('skipped')
                assert int(el['frame'] * bk['sfr']) == F
                continue
            # the cells the reference's slice selects
            cells = np.arange(H * W).reshape(H, W)[ry[0]:ry[1], rx[0]:rx[1]]
            mine = np.arange(H * W).reshape(H, W)[y0:max(y0, y1), x0:max(x0, x1)]
            assert np.array_equal(cells.reshape(-1), mine.reshape(-1)), (el, ry, rx)
            if rx[1] < 0:
                kinds.add('left of the frame' if cells.size else 'left of the frame, empty')
            if ry[1] < 0:
                kinds.add('above the frame')
            if rx[1] >= 0 and ry[1] >= 0:
                el_x, el_y = el['x'], el['y']
                kinds.add('whole grid' if cells.size == H * W else ('one cell' if cells.size == 1 else None))
                kinds.add('left border' if el_x < 0 and rx == [0, rx[1]] and 0 < rx[1] < W else None)
                kinds.add('top border' if el_y < 0 and 0 < ry[1] < H else None)
                kinds.add('right border' if rx[1] == W and 0 < rx[0] and cells.size != H * W else None)
                kinds.add('bottom border' if ry[1] == H and 0 < ry[0] and cells.size != H * W else None)
    assert kinds >= {'skipped', 'left of the frame', 'left of the frame, empty', 'above the frame', 'whole grid', 'one cell', 'left border',
                     'top border', 'right border', 'bottom border'}
    # an off-frame box pools cells and gives a FINITE mean (numpy counts the negative bound from the far end); NaN only when empty
    assert np.isfinite(FX['track'][:3]).all() and np.isnan(FX['track']).any(axis=1).sum() == 1
    assert not FX['track'][-1].any()                                             # nothing but a skipped element
    # clips
    t2f = bk['time2frame']
    ends = [int(b) for _, b in FX['time_nodes']]
    frames = [[b[0] for b in l] for l in bk['clip_boxes']]
    assert any(e not in t2f for e in ends)                                       # the end - 1 rule
    assert any(int(t2f[e if e in t2f else e - 1][-1] * bk['sfr']) >= F for e in ends) and all(max(f) < F for f in frames)
    assert any(int(a) == int(b) for a, b in FX['time_nodes']) and all(frames)
    # text: each clause of Time.includes alone, and a clip without dialog
    seen = set()
    for t in bk['text_nodes']:
        s, e = t['start'], t['end']
        hit = [(ts <= s <= te, ts <= e <= te, s <= ts and e >= te) for ts, te in bk['times']]
        seen |= {h for h in hit if sum(h) == 1}
        if not any(any(h) for h in hit):
            seen.add('none')
    assert seen >= {(True, False, False), (False, True, False), (False, False, True), 'none'}
    assert any(len(r) == 0 for r in bk['tok_rows']) and (FX['clip_text'][[len(r) == 0 for r in bk['tok_rows']]] == 0).all()


def test_first_fixture_boxes_are_unchanged_by_the_slice_rule():
    """no box of the first scene has a negative bound: what track_boxes returns for it is (ry, rx) itself, clamped to the grid as the
    slice clamps it"""
    FX = FC.fixture('rawfeat')
    F, C, H, W = FX['grid'].shape
    bk = FC.bookkeeping(FX)
    for tr, boxes in zip(bk['tracks'], bk['track_boxes']):
        for el, (f, y0, y1, x0, x1) in zip(tr, boxes):
            ry, rx = FC.raw_person_box(el, tuple(FX['dims']), H, W)
            assert ry[1] >= 0 and rx[1] >= 0
            assert [y0, y1, x0, x1] == [min(ry[0], H), ry[1], min(rx[0], W), rx[1]]


# ---------------------------------------------------------------------------------------------------------------------------
# gather_features
# ---------------------------------------------------------------------------------------------------------------------------
def test_planted_values_are_what_they_claim():
    bits = lambda t: [int(v) & 0xFFFFFFFF for v in t.view(torch.int32)]
    for w in FC.TIES + FC.SUBNORMALS[3:]:
        assert w & 0xFFFF == 0x8000                                              # a tie: exactly half a bf16 ulp
    even, odd = FC.TIES[0], FC.TIES[1]
    assert (even >> 16) & 1 == 0 and (odd >> 16) & 1 == 1
    rnd = lambda *w: [int(v) & 0xFFFF for v in FC.f32_bits(*w).to(torch.bfloat16).view(torch.int16)]
    assert rnd(even, odd) == [even >> 16, (odd >> 16) + 1]                       # to the even neighbour: down, up
    assert rnd(*FC.NEAR_TIES) == [even >> 16, (even >> 16) + 1, odd >> 16, (odd >> 16) + 1]
    assert {w & 0xFFFF for w in FC.NEAR_TIES} == {0x7FFF, 0x8001}
    assert all(w & 0xFFFF == 0 for w in FC.EXACT_BF16)
    for w in FC.SUBNORMALS:
        assert (w >> 23) & 0xFF == 0 and w & 0x7FFFFF
    assert rnd(0x7F7FFFFF, 0xFF7FFFFF) == [0x7F80, 0xFF80]                       # the largest finite fp32 rounds to inf
    sp = FC.f32_bits(*FC.BF16_SPECIALS)
    assert bits(sp) == list(FC.BF16_SPECIALS) and torch.isnan(sp).sum() == 1 and torch.isinf(sp).sum() == 2
    d = torch.tensor([FC.DOUBLE_ROUNDING], dtype=torch.float64)
    assert float(d[0]) != 1.0 + 2.0 ** -8 and bits(d.float()) == [even]
    assert rnd(*bits(d.float())) == [0x3F80]
    direct = 1.0 + 2.0 ** -7                                                     # the nearest bf16 of the float64 value itself
    assert abs(FC.DOUBLE_ROUNDING - direct) < abs(FC.DOUBLE_ROUNDING - 1.0)


@pytest.mark.parametrize('f64', [False, True])
def test_gather_small_case_holds_its_index_patterns(f64):
    c, clip, track, index = FC.gather_inputs('small', f64)
    assert (c.rows, c.clip_dim, c.track_dim, c.n_clip, c.n_track) == (37, 12, 20, 5, 7)
    assert clip.shape == (5, 16) and track.shape == (7, 28) and (clip[:, 12:] == FC.PAD).all() and (track[:, 20:] == FC.PAD).all()
    neg = (index < 0)
    pats = {tuple(r.tolist()) for r in neg}
    assert pats >= {(True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, False, False)}
    assert (index[:, 0] == c.n_clip - 1).any() and (index[:, 1] == c.n_track - 1).any() and (index[:, 2] == c.n_track - 1).any()
    assert int((index[:, 0] == 2).sum()) >= 16
    assert int(index.min()) == -1 and int(index[:, 0].max()) < c.n_clip and int(index[:, 1:].max()) < c.n_track
    for dt in (torch.float32, torch.bfloat16):
        ref = FC.gather_reference(c, clip, track, index, dt)
        assert ref.shape == (37, 52) and ref.dtype == dt and not (ref.float() == FC.PAD).any()
        # every planted value reaches the output: through part 0 and through parts 1 and 2
        if dt == torch.float32:
            have = lambda t: {int(v) & 0xFFFFFFFF for v in t.contiguous().view(torch.int32).reshape(-1)}
            assert have(ref[:, :12]) >= set(FC.BF16_SPECIALS[:12])
            assert have(ref[:, 12:32]) >= set(FC.BF16_SPECIALS[12:]) and have(ref[:, 32:]) >= set(FC.BF16_SPECIALS[12:])
        assert torch.isnan(ref[:, 12:32]).any() and torch.isnan(ref[:, 32:]).any()
        assert not ref[3].any()
    if f64:
        got = FC.gather_reference(c, clip, track, index, torch.bfloat16)
        rows = (index[:, 1] == FC.DR_TRACK_ROW).nonzero().view(-1)
        assert rows.numel() and all(int(got[r, 12].view(torch.int16)) == 0x3F80 for r in rows)
        assert int(track[FC.DR_TRACK_ROW, :1].to(torch.bfloat16).view(torch.int16)) in (0x3F80, 0x3F81)


def test_grid_stride_shapes_exceed_the_cap():
    c = FC.GATHER_STRIDE
    D = c.clip_dim + 2 * c.track_dim
    assert c.rows * D // 4 == 2099200 > FC.CAP_ITEMS and (c.rows - 1) * D // 4 < FC.CAP_ITEMS + 8192
    R, C = FC.Q_STRIDE_SHAPE
    assert FC.r32(R) * C // 8 == 2105344 > FC.CAP_ITEMS and R % 32 != 0
    rows, cols = FC.MASK_SHAPE
    assert rows * cols == 69010 > FC.MASK_THREADS and rows % 4 != 0
    assert (FC.CARRY_SEED + 1) >> 32 == (FC.CARRY_SEED >> 32) + 1 and (FC.CARRY_SEED + 1) & 0xFFFFFFFF == 0


# ---------------------------------------------------------------------------------------------------------------------------
# q32b / q16b
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,C', FC.Q_SHAPES + ((72, 2048),))
def test_layout_maps_are_bijections(R, C):
    R32 = FC.r32(R)
    hi, lo = FC.q32b_halfwords(R32, C)
    assert torch.equal(lo, hi + 32)                                              # 64 bytes further
    both = torch.cat([hi.reshape(-1), lo.reshape(-1)])
    assert torch.equal(both.sort().values, torch.arange(R32 * C * 2))
    # per plane: the hi halves fill the first 64 bytes of every 128-byte line, in (block, row, column) order
    assert torch.equal((hi // 64 * 32 + hi % 64).reshape(-1).sort().values, torch.arange(R32 * C)) and int((hi % 64).max()) == 31
    q = FC.q16b_halfwords(R32, C)
    assert torch.equal(q.reshape(-1).sort().values, torch.arange(R32 * C))
    # the documented byte offsets, element by element
    for r, c in ((0, 0), (R32 - 1, C - 1), (R32 // 2, C // 2 + 1), (31, 31)):
        line = (r // 32 * (C // 32) + c // 32) * 32 + r % 32
        assert int(hi[r, c]) * 2 == line * 128 + (c % 32) * 2 and int(lo[r, c]) * 2 == line * 128 + (c % 32) * 2 + 64
        assert int(q[r, c]) * 2 == line * 64 + (c % 32) * 2


@pytest.mark.parametrize('R,C', FC.Q_SHAPES)
def test_split_restatement_and_images(R, C):
    x = FC.writer_values(R, C, seed=R * 1000 + C)
    nz = x[x != 0]
    assert torch.isfinite(x).all() and float(nz.abs().min()) >= 2.0 ** -100 and float(x.abs().max()) <= 2.0 ** 100
    if R * C >= 64:
        have = {int(v) & 0xFFFFFFFF for v in x.view(torch.int32).reshape(-1)}
        assert have >= set(FC.WRITER_SPECIALS)
    hi, lo = FC.split_hi_lo(x)
    h, l = hi.view(torch.bfloat16).double(), lo.view(torch.bfloat16).double()
    # two bf16 roundings, unit roundoff 2^-8 each: |x - hi| <= 2^-8 |x|, |(x - hi) - lo| <= 2^-8 |x - hi|
    assert bool(((x.double() - (h + l)).abs() <= 2.0 ** -16 * x.double().abs()).all())
    rem = x - h.float()
    assert bool((rem.double() == x.double() - h).all())                          # the remainder is exact in fp32
    assert bool(((rem == 0) | (rem.abs() >= 2.0 ** -126)).all())                 # and never subnormal
    img = FC.q32b_image(x)
    assert img.numel() * 2 == FC.r32(R) * C * 4
    ih, il = FC.q32b_halfwords(R, C)
    back = img[ih].view(torch.bfloat16).float() + img[il].view(torch.bfloat16).float()
    assert bool(((back.double() - x.double()).abs() <= 2.0 ** -16 * x.double().abs()).all())
    pad = torch.ones(img.numel(), dtype=torch.bool)
    pad[ih.reshape(-1)] = False
    pad[il.reshape(-1)] = False
    assert int(pad.sum()) == (FC.r32(R) - R) * C * 2 and not img[pad].any()
    img16 = FC.q16b_image(x)
    assert img16.numel() * 2 == FC.r32(R) * C * 2 and torch.equal(img16[FC.q16b_halfwords(R, C)], hi)


def test_images_reject_a_wrong_rounding():
    """the planted ties tell round-to-nearest-even from truncation and from round-half-up"""
    R, C = FC.Q_LD_SHAPE
    x = FC.writer_values(R, C, seed=R * 1000 + C)
    hi, _ = FC.split_hi_lo(x)
    u = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    as16 = lambda t: ((t & 0xFFFF) - ((t & 0x8000) << 1)).to(torch.int16)
    trunc, half_up = as16(u >> 16), as16((u + 0x8000) >> 16)
    assert not torch.equal(trunc, hi) and not torch.equal(half_up, hi)
    even = (u == FC.TIES[0])
    assert bool(even.any()) and torch.equal(trunc[even], hi[even]) and not torch.equal(half_up[even], hi[even])
    assert torch.equal(as16((u + 0x7FFF + ((u >> 16) & 1)) >> 16), hi)           # the bit formula of kernels.hpp: bf16_rne


def test_dropout_oracle_at_the_mask_shape():
    from oracle.lirec_oracle import dropout_keep_mask
    rows, cols = FC.MASK_SHAPE
    m0 = dropout_keep_mask(FC.MASK_SEED, 0, rows, cols, 0.0)
    assert m0.shape == (rows, cols) and m0.all()
    m5 = dropout_keep_mask(FC.MASK_SEED, 0, rows, cols, 0.5)
    assert abs(m5.mean() - 0.5) < 0.01 and not np.array_equal(m5, dropout_keep_mask(FC.MASK_SEED, 5, rows, cols, 0.5))
    a, b = dropout_keep_mask(FC.CARRY_SEED, 0, rows, cols, 0.5), dropout_keep_mask(FC.CARRY_SEED + 1, 0, rows, cols, 0.5)
    wrong = dropout_keep_mask(FC.CARRY_SEED & 0xFFFFFFFF00000000, 0, rows, cols, 0.5)       # the low word wrapped, no carry
    assert not np.array_equal(a, b) and not np.array_equal(b, wrong)
