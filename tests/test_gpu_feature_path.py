"""The kernels that PRODUCE the features, on the device, at their edges (cases and host restatements: tests/feature_cases.py, proved on
the CPU by tests/test_host_feature_cases.py):

  grid_pool_kernel, rows_max_kernel          == oracle/rawfeat_oracle.py (np.mean / np.max), bit for bit
  gather_features_kernel<f64, bf16>          == index_select + .float() + .to(bfloat16), bit for bit (a NaN only has to be a NaN)
  to_q32b / to_q16b / q32b_write_rows        == the layouts and the hi / lo split as gemm_bf16x3.hpp documents them, byte for byte
  dropout_mask_kernel                        == oracle/lirec_oracle.py dropout_keep_mask

No tolerance anywhere.  The three grid-stride cases move 35 - 135 MB each (the smallest shapes over the 8192-workgroup cap); they
take well under a second apiece on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_cases as FC
from lirec_amd import _lib, ops
from lirec_amd import rawfeat as RF
from lirec_amd._lib import lib
from test_rawfeat import same

pytestmark = pytest.mark.gpu
SENT = -12345.0


def stream():
    return ops.current_stream_handle()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. grid_pool
# ---------------------------------------------------------------------------------------------------------------------------
def pool_direct(grid, lists, pad):
    """lirec_grid_pool into a sentinel-filled [n_out, C + pad] buffer"""
    F, Cc, H, W = grid.shape
    boxes, est = RF._segments(lists, 5, grid.device)
    out = torch.full((max(len(lists), 1), Cc + pad), SENT, dtype=torch.float32, device=grid.device)
    code = lib().lirec_grid_pool(grid.data_ptr(), F, Cc, H, W, boxes.data_ptr() if boxes.numel() else est.data_ptr(), est.data_ptr(),
                                 len(lists), out.data_ptr(), Cc + pad, stream())
    return code, out


def first_difference(got, ref, names):
    for o in range(ref.shape[0]):
        if not FC.bits_equal(got[o], ref[o]):
            bad = [c for c in range(ref.shape[1]) if not FC.bits_equal(got[o, c:c + 1], ref[o, c:c + 1])]
            return '%s: %d channels differ, first %d: device %r numpy %r' % (names[o], len(bad), bad[0], got[o, bad[0]], ref[o, bad[0]])
    return None


@pytest.mark.parametrize('name', ['main', 'wide'])
def test_grid_pool_is_np_mean_then_np_max_bit_for_bit(name):
    pg = {g.name: g for g in FC.pool_grids()}[name]
    lists, names, ref = FC.pool_reference(name)
    grid = torch.from_numpy(pg.grid.copy()).cuda()
    got = RF.grid_pool(grid, lists).cpu().numpy()
    assert got.shape == ref.shape
    assert first_difference(got, ref, names) is None
    if name == 'main':
        # NaN reaches the special channel's outputs and the rows of an empty crop, nothing else
        empty = np.array(['empty box' in n for n in names])
        assert not np.isnan(np.delete(got[~empty], FC.SPECIAL_C, axis=1)).any() and np.isnan(got[~empty][:, FC.SPECIAL_C]).any()
        assert np.isnan(got[empty]).all()


def test_grid_pool_leading_dimension_and_no_output():
    pg = FC.pool_grids()[0]
    lists, names, ref = FC.pool_reference('main')
    grid = torch.from_numpy(pg.grid.copy()).cuda()
    Cc = grid.shape[1]
    code, out = pool_direct(grid, lists, 8)
    assert code == 0
    out = out.cpu().numpy()
    assert first_difference(out[:, :Cc], ref, names) is None
    assert (out[:, Cc:] == SENT).all()                                            # the padding columns stay untouched
    code, out = pool_direct(grid, [], 8)                                          # n_out = 0: OK, nothing written
    assert code == 0 and bool((out == SENT).all())
    assert RF.grid_pool(grid, []).shape == (0, Cc)
    assert lib().lirec_grid_pool(grid.data_ptr(), 3, Cc, 23, 29, out.data_ptr(), out.data_ptr(), 1, out.data_ptr(), Cc - 1,
                                 stream()) == _lib.LIREC_EINVAL                   # ld_out < C


# ---------------------------------------------------------------------------------------------------------------------------
# 2. rows_max
# ---------------------------------------------------------------------------------------------------------------------------
def test_rows_max_is_np_max_bit_for_bit_on_a_strided_view():
    src = torch.from_numpy(FC.rows_source().copy()).cuda()
    view = src[:, FC.ROWS_LAYER, :]
    assert view.stride(0) == FC.ROWS_LAYERS * FC.ROWS_DIM and not view.is_contiguous()
    ref = FC.rows_reference()
    names = [str(l) for l in FC.ROW_LISTS]
    got = RF.rows_max(view, FC.ROW_LISTS).cpu().numpy()
    assert first_difference(got, ref, names) is None
    # ld_out = dim + 8 over a sentinel
    idx, est = RF._segments([[[r] for r in l] for l in FC.ROW_LISTS], 1, src.device)
    out = torch.full((len(FC.ROW_LISTS), FC.ROWS_DIM + 8), SENT, dtype=torch.float32, device=src.device)
    assert lib().lirec_rows_max(view.data_ptr(), view.stride(0), idx.data_ptr(), est.data_ptr(), len(FC.ROW_LISTS), FC.ROWS_DIM,
                                out.data_ptr(), FC.ROWS_DIM + 8, stream()) == 0
    out = out.cpu().numpy()
    assert first_difference(out[:, :FC.ROWS_DIM], ref, names) is None and (out[:, FC.ROWS_DIM:] == SENT).all()
    assert RF.rows_max(view, []).shape == (0, FC.ROWS_DIM)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the second fixture of the reference's own classes
# ---------------------------------------------------------------------------------------------------------------------------
def test_edges_fixture_device_pooling_is_bit_identical(tmp_path):
    FX = FC.fixture('rawfeat_edges')
    bk = FC.bookkeeping(FX)
    p = str(tmp_path / 'grid.npy')
    np.save(p, FX['grid'])
    grid = RF.load_npy(p, 'cuda')
    assert same(RF.grid_pool(grid, bk['clip_boxes']).cpu().numpy(), FX['clip_visual'])
    got = RF.grid_pool(grid, bk['track_boxes']).cpu().numpy()
    for k in range(got.shape[0]):
        assert same(got[k], FX['track'][k]), ('track %d' % k, bk['track_boxes'][k], got[k, :4], FX['track'][k, :4])
    assert same(RF.clip_visual_features(grid, bk['time2frame'], bk['tnodes'], bk['sfr']).cpu().numpy(), FX['clip_visual'])
    assert same(RF.track_features(grid, bk['tracks'], tuple(FX['dims']), bk['sfr']).cpu().numpy(), FX['track'])
    tokens = torch.from_numpy(FX['tokens']).cuda()
    assert same(RF.clip_text_features(tokens, bk['times'], bk['ranges'], bk['text_nodes']).cpu().numpy(), FX['clip_text'])
    assert RF.grid_pool(grid, [[]]).abs().sum().item() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. gather_features
# ---------------------------------------------------------------------------------------------------------------------------
def gather_direct(c, clip, track, index, bf16, rows=None, clip_dim=None, ld_out=None, out_offset=0):
    D = c.clip_dim + 2 * c.track_dim
    dt = torch.bfloat16 if bf16 else torch.float32
    out = torch.full((c.rows, D + c.pad_out), FC.PAD, dtype=dt, device=clip.device)
    fn = lib().lirec_gather_features_bf16 if bf16 else lib().lirec_gather_features
    code = fn(clip.data_ptr(), clip.shape[1], track.data_ptr(), track.shape[1], int(clip.dtype == torch.float64), index.data_ptr(),
              c.rows if rows is None else rows, c.clip_dim if clip_dim is None else clip_dim, c.track_dim, out.data_ptr() + out_offset,
              D + c.pad_out if ld_out is None else ld_out, stream())
    return code, out


@pytest.mark.parametrize('bf16', [False, True], ids=['f32out', 'bf16out'])
@pytest.mark.parametrize('f64', [False, True], ids=['f32tab', 'f64tab'])
def test_gather_features_small_case_with_leading_dimensions(f64, bf16):
    c, clip, track, index = FC.gather_inputs('small', f64)
    D = c.clip_dim + 2 * c.track_dim
    want = FC.gather_reference(c, clip, track, index, torch.bfloat16 if bf16 else torch.float32)
    code, out = gather_direct(c, clip.cuda(), track.cuda(), index.cuda(), bf16)
    assert code == 0
    out = out.cpu()
    assert FC.raw_equal_but_nan(out[:, :D].contiguous(), want)
    assert bool((out[:, D:] == torch.tensor(FC.PAD).to(out.dtype)).all())         # the sentinel columns
    if c.pad_out == 4 and not f64:                                                # the wrapper (ld == dim) on the same values
        got = ops.gather_features(clip[:, :c.clip_dim].cuda(), track[:, :c.track_dim].cuda(), index.cuda(),
                                  torch.bfloat16 if bf16 else torch.float32).cpu()
        assert FC.raw_equal_but_nan(got, want)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32out', 'bf16out'])
def test_gather_features_grid_stride_loop(bf16):
    """rows * D / 4 = 2,099,200 work items for 8192 * 256 threads: the last 2,048 are taken in a second trip (34 MB of output)"""
    c, clip, track, index = FC.gather_inputs('stride', False)
    clip, track, index = clip.cuda(), track.cuda(), index.cuda()
    want = FC.gather_reference(c, clip, track, index, torch.bfloat16 if bf16 else torch.float32)      # (torch, on the device)
    code, out = gather_direct(c, clip, track, index, bf16)
    assert code == 0
    it = torch.int16 if bf16 else torch.int32
    assert torch.equal(out.view(it), want.view(it))
    assert bool((out[-1, :c.clip_dim] == clip[c.n_clip - 1].to(out.dtype)).all()) and not bool(out[-1, c.clip_dim:c.clip_dim + c.track_dim].any())


def test_gather_features_entry_checks():
    c, clip, track, index = FC.gather_inputs('small', False)
    clip, track, index = clip.cuda(), track.cuda(), index.cuda()
    D = c.clip_dim + 2 * c.track_dim
    for bf16 in (False, True):
        assert gather_direct(c, clip, track, index, bf16, clip_dim=6)[0] == _lib.LIREC_EINVAL
        assert gather_direct(c, clip, track, index, bf16, ld_out=D - 4)[0] == _lib.LIREC_EINVAL
        assert gather_direct(c, clip, track, index, bf16, rows=c.rows - 1, out_offset=4)[0] == _lib.LIREC_EINVAL     # misaligned output
        code, out = gather_direct(c, clip, track, index, bf16, rows=0)
        assert code == 0 and bool((out.float() == float(torch.tensor(FC.PAD).to(out.dtype))).all())                 # nothing written


# ---------------------------------------------------------------------------------------------------------------------------
# 5. q32b / q16b
# ---------------------------------------------------------------------------------------------------------------------------
FILL = 0xA5
SLACK = 512


def filled(nbytes, device='cuda'):
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=device)


@pytest.mark.parametrize('R,C_', FC.Q_SHAPES)
def test_q32b_and_q16b_layout_and_split_against_the_host_restatement(R, C_):
    """q32b: element (r, c) has its hi half bf16_rne(x) at byte ((r / 32 * (C / 32) + c / 32) * 32 + r % 32) * 128 + (c % 32) * 2 and
    its lo half bf16_rne(x - float(hi)) 64 bytes further; q16b: its one half bf16_rne(x) at ((...) * 32 + r % 32) * 64 + (c % 32) * 2;
    rows R .. R32 - 1 are zero bytes; nothing past R32 * C * 4 (* 2) bytes is written."""
    x = FC.writer_values(R, C_, seed=R * 1000 + C_)
    R32 = FC.r32(R)
    n32, n16 = int(lib().lirec_q32b_bytes(R, C_)), int(lib().lirec_q16b_bytes(R, C_))
    assert n32 == R32 * C_ * 4 and n16 == R32 * C_ * 2
    want32, want16 = FC.q32b_image(x), FC.q16b_image(x)
    srcs = [(x.cuda(), C_, 'wrapper')]
    if (R, C_) == FC.Q_LD_SHAPE:
        wide = torch.full((R, C_ + 4), FC.PAD)
        wide[:, :C_] = x
        srcs.append((wide.cuda(), C_ + 4, 'ld_src = C + 4'))
    for src, ld, how in srcs:
        d32, d16 = filled(n32 + SLACK), filled(n16 + SLACK)
        if how == 'wrapper':
            q = ops.to_q32b(src, out=d32)
            assert q.planes == 2 and q.x_q32 == 1 and q.data is d32
            q = ops.to_q16b(src, out=d16)
            assert q.planes == 1 and q.x_q32 == 2 and not q.k64
        else:
            assert lib().lirec_to_q32b(src.data_ptr(), ld, R, C_, d32.data_ptr(), stream()) == 0
            assert lib().lirec_to_q16b(src.data_ptr(), ld, R, C_, d16.data_ptr(), stream()) == 0
        d32, d16 = d32.cpu(), d16.cpu()
        assert torch.equal(d32[:n32].view(torch.int16), want32), how
        assert torch.equal(d16[:n16].view(torch.int16), want16), how
        assert bool((d32[n32:] == FILL).all()) and bool((d16[n16:] == FILL).all()), how


def test_q32b_and_q16b_grid_stride_loop():
    """R32 * C / 8 = 2,105,344 work items for 8192 * 256 threads (67 MB in, 67 + 34 MB out); the restatement runs on the device"""
    R, C_ = FC.Q_STRIDE_SHAPE
    g = torch.Generator(device='cuda').manual_seed(9)
    x = torch.randn(R, C_, device='cuda', generator=g).clamp(-8, 8)
    x = torch.where(x.abs() < 2.0 ** -6, torch.full_like(x, -0.75), x)
    x = torch.ldexp(x, torch.randint(-94, 97, (R, 1), device='cuda', generator=g))
    sp = FC.f32_bits(*FC.WRITER_SPECIALS).cuda()
    x.view(-1)[-sp.numel():] = sp                                                 # (the last row: taken in the second trip)
    x.view(-1)[:sp.numel()] = sp
    n32, n16 = int(lib().lirec_q32b_bytes(R, C_)), int(lib().lirec_q16b_bytes(R, C_))
    assert n32 == FC.r32(R) * C_ * 4 and n16 == FC.r32(R) * C_ * 2
    d32, d16 = filled(n32 + SLACK), filled(n16 + SLACK)
    ops.to_q32b(x, out=d32)
    ops.to_q16b(x, out=d16)
    assert torch.equal(d32[:n32].view(torch.int16), FC.q32b_image(x))
    assert torch.equal(d16[:n16].view(torch.int16), FC.q16b_image(x))
    assert bool((d32[n32:] == FILL).all()) and bool((d16[n16:] == FILL).all())


@pytest.mark.parametrize('f64', [False, True], ids=['f32', 'f64'])
def test_q32b_write_rows_writes_its_rows_and_nothing_else(f64):
    C_, dst_rows = 96, 64
    n = dst_rows * C_ * 4
    ih, il = FC.q32b_halfwords(dst_rows, C_)
    for row0, rows, pad in ((29, 7, 4), (0, dst_rows, 0), (63, 1, 0)):            # across a block boundary; everything; the last row
        x = FC.writer_values(rows, C_, seed=500 + row0)
        src = torch.full((rows, C_ + pad), FC.PAD, dtype=torch.float64 if f64 else torch.float32)
        src[:, :C_] = x.double() if f64 else x
        if f64:
            src[0, 0] = FC.DOUBLE_ROUNDING
        hi, lo = FC.split_hi_lo(src[:, :C_].float())                              # a float64 value goes through fp32 first
        want = filled(n + SLACK, 'cpu').view(torch.int16).clone()
        want[ih[row0:row0 + rows].reshape(-1)] = hi.reshape(-1)
        want[il[row0:row0 + rows].reshape(-1)] = lo.reshape(-1)
        dst = filled(n + SLACK)
        sd = src.cuda()
        if pad:
            assert lib().lirec_q32b_write_rows(sd.data_ptr(), int(f64), C_ + pad, rows, C_, dst.data_ptr(), row0, dst_rows, stream()) == 0
        else:
            ops.q32b_write_rows(sd, dst, row0, dst_rows)
        assert torch.equal(dst.cpu().view(torch.int16), want), (row0, rows)
        if f64:
            assert int(want[ih[row0, 0]]) == 0x3F80 and int(want[il[row0, 0]]) == 0x3B80      # 1 + 2^-8 -> hi 1.0, lo 2^-8
        if rows == dst_rows and not f64:
            assert torch.equal(want[:n // 2], FC.q32b_image(x))                   # what to_q32b writes for the same values
    dst = filled(n)
    assert lib().lirec_q32b_write_rows(dst.data_ptr(), 0, C_, 2, C_, dst.data_ptr(), 63, dst_rows, stream()) == _lib.LIREC_EINVAL


# ---------------------------------------------------------------------------------------------------------------------------
# 6. dropout_mask
# ---------------------------------------------------------------------------------------------------------------------------
def oracle_mask(seed, site, p):
    from oracle.lirec_oracle import dropout_keep_mask
    return torch.from_numpy(dropout_keep_mask(seed, site, FC.MASK_SHAPE[0], FC.MASK_SHAPE[1], p).astype(np.uint8))


def test_dropout_mask_stride_loop_against_the_oracle():
    rows, cols = FC.MASK_SHAPE
    assert rows * cols > FC.MASK_THREADS
    for p in FC.MASK_PS:
        for site in FC.MASK_SITES:
            got = ops.dropout_mask(rows, cols, FC.MASK_SEED, p, site, 'cuda').cpu()
            assert torch.equal(got, oracle_mask(FC.MASK_SEED, site, p)), (p, site)
            if p == 0:
                assert bool((got == 1).all())


def test_dropout_mask_device_seed_offset_carries_into_the_high_word():
    rows, cols = FC.MASK_SHAPE

    def mask(seed, offset):
        t = None if offset is None else torch.tensor([offset], dtype=torch.int64, device='cuda')
        d = ops.make_dropout(seed, 0.5, seed_dev=t)
        keep = torch.full((rows, cols), 7, dtype=torch.uint8, device='cuda')
        assert lib().lirec_dropout_mask(keep.data_ptr(), rows, cols, C.byref(d), 3, stream()) == 0
        return keep.cpu()
    assert torch.equal(mask(FC.CARRY_SEED, 1), oracle_mask(FC.CARRY_SEED + 1, 3, 0.5))
    assert torch.equal(mask(FC.CARRY_SEED, 0), mask(FC.CARRY_SEED, None))
    assert torch.equal(mask(FC.CARRY_SEED, None), oracle_mask(FC.CARRY_SEED, 3, 0.5))
