"""The input-feature gradient and the piece-table kernels at the level of an op, against the float64 references of
tests/dx_cases.py: lirec_embed_dx (dx_gemm_kernel + dx_zero_kernel), lirec_embed_dx_indexed (dxi_gemm_kernel),
lirec_embed_dw1_indexed (onehot_kernel + its two weight-gradient GEMM stages) and lirec_embed_l1_indexed (gather_act_kernel).

The operand is hand-filled: dZ1 goes into the head's workspace (fp32 rows, or bf16 hi / lo planes for the pooled head of the
planes case), S into its buffer, and the reference multiplies the very same values in float64 -- no relu decision and no rounding
of an earlier kernel enters a comparison.  Every buffer is sized by the library's own size functions; every output is pre-filled
with NaN (an element never written stays NaN and fails; rows of dZ1 / S the call must not read are NaN as well).  Every case runs
on the exact core (gemm mode 0) and on the split core (mode 2); the bounds are dx_cases.bound's.

What a wrong kernel would do to these comparisons is rehearsed without a GPU in tests/test_host_dx_cases.py (a dropped k-tile, a
column offset off by one, an omitted gap, the trailing S row taken for a piece, the compact row number as the dropout counter)."""
import pytest
import torch

import dx_cases as DC
from lirec_amd import _lib, ops
from test_gpu_layer1_persistent import RELU_EPS, RELU_FRAC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 20261019
MODES = [0, 2]
MODE_IDS = ['f32mfma', 'bf16x3']


class gemm_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        ops.ensure_scratch(DEV)
        ops.set_gemm_mode(self.mode)

    def __exit__(self, *exc):
        ops.set_gemm_mode(_lib.default_gemm_mode())


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, DC.NAN, dtype=dtype, device=DEV)


def dummy_x(dtype=torch.float32):
    return torch.zeros(64, dtype=dtype, device=DEV)             # (none of the ops under test reads the feature rows)


def head_pool(h, hd, n):
    """(sel, pool tuple or None, device row lists) of a head; the compact form's lists come from ops.compact_rows and are checked
    against the reference's"""
    sel = (h.group, None, h.goff)
    if h.kind == 'plain':
        return sel, None, None
    Hbar, f = nans(1), nans(1)                                  # (never read by these ops)
    if h.mask is None:
        return sel, (torch.ones(n, h.R, device=DEV), h.R, 1, Hbar, f, None), None
    mask = hd['mask'].to(DEV)
    cmp = ops.compact_rows(mask, n, h.R)
    cnt = hd['L'].numel()
    assert int(cmp[2].item()) == cnt and torch.equal(cmp[0][:cnt].cpu().long(), hd['L']) and torch.equal(cmp[1].cpu(), hd['cstart'])
    return sel, (None, h.R, 1, Hbar, f, cmp), cmp


def workspace(h, n):
    rows = n * h.group
    return nans(ops.workspace_bytes(rows + (n if h.kind == 'pooled' else 0), h.nseg, h.J) // 4)


def bwd_args(h, hd, n, rp1, D, ws, gW=(), gb=(), rows=None, planes=None, X=None):
    sel, pool, _ = head_pool(h, hd, n) if rows != 0 else ((h.group, None, h.goff), None, None)
    segs = ops.Segments([o for o, _ in h.segs], [d for _, d in h.segs], [1] * h.nseg)
    a = ops.embed_bwd_args(dummy_x() if X is None else X, D, (sel[0], rp1, sel[2]), n * h.group if rows is None else rows, h.J, segs, [],
                           None, None, 0, list(gW), list(gb), [], [], ws, ops.make_dropout(SEED, 0.0), pool=pool, planes=planes)
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lirec_embed_dx
# ---------------------------------------------------------------------------------------------------------------------------
def run_dx(case, mode, operand='f32'):
    inp = DC.dx_inputs(case, operand)
    n, rp1, D = case.n, case.rp1, case.D
    tag = '%s mode %d' % (case.name, mode)
    with gemm_mode(mode):
        args, W1s, keepalive = [], [], []
        X = dummy_x(torch.bfloat16 if mode == 3 else torch.float32)
        for hd in inp['heads']:
            h = hd['h']
            ws = workspace(h, n)
            cnt, ldh = hd['L'].numel(), h.nseg * h.J
            rows32 = (n * h.group + 31) // 32 * 32
            planes = None
            if hd['hi'] is not None:
                # bf16 planes over the workspace: hi [rows32][ldh] at the start, lo behind it; NaN at and beyond row `cnt`
                pl = ws.view(torch.bfloat16)
                pl[:cnt * ldh] = hd['hi'].reshape(-1).to(DEV)
                if operand == 'hilo':
                    pl[rows32 * ldh:rows32 * ldh + cnt * ldh] = hd['lo'].reshape(-1).to(DEV)
            else:
                ws[:cnt * ldh] = hd['dz'].reshape(-1).to(DEV)
            if h.planes:
                planes = torch.full((ops.planes_bytes(n * h.group, sum(d for _, d in h.segs), h.J, False, mode == 3),), 0x3C,
                                    dtype=torch.uint8, device=DEV)
                assert planes.data_ptr() % 256 == 0
            args.append(bwd_args(h, hd, n, rp1, D, ws, planes=planes, X=X))
            W1s.append([w.to(DEV) for w in hd['W1']])
            keepalive.append((ws, planes))
        dX = nans(n, rp1, D)
        ops.embed_dx(args, W1s, dX)
        dX16 = nans(n, rp1, D, dtype=torch.bfloat16)
        ops.embed_dx(args, W1s, dX16)
        torch.cuda.synchronize()
        for hd, (ws, _) in zip(inp['heads'], keepalive):
            if hd['hi'] is not None:                            # the reference operand is what the workspace holds
                cnt, ldh = hd['L'].numel(), hd['h'].nseg * hd['h'].J
                got = ws.view(torch.bfloat16)[:cnt * ldh].cpu().view(cnt, ldh).float()
                if operand == 'hilo':
                    r32 = (n * hd['h'].group + 31) // 32 * 32
                    got = got + ws.view(torch.bfloat16)[r32 * ldh:r32 * ldh + cnt * ldh].cpu().view(cnt, ldh).float()
                assert torch.equal(got, hd['dz'])
    got32, got16 = dX.cpu(), dX16.cpu()
    DC.check_dx(got32, inp, mode, tag)
    DC.check_dx_bf16(got16, got32, tag + ' bf16 leaf')
    assert DC.bits_zero(got16.reshape(n * rp1, D)[~inp['written']]), tag + ': bf16 leaf, an element no head writes is not +0'


@pytest.mark.parametrize('mode', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('case', DC.DX_CASES, ids=[c.id for c in DC.DX_CASES])
def test_embed_dx_against_fp64(case, mode):
    run_dx(case, mode)


@pytest.mark.parametrize('mode,operand', [(2, 'hilo'), (3, 'hi')], ids=['bf16x3-hi+lo', 'onepass-hi'])
def test_embed_dx_plane_operands(mode, operand):
    """the pooled head's dZ1 as bf16 planes laid over its workspace (hi + lo in mode 2; hi alone in mode 3, the lo plane left NaN),
    the plain head of the same call fp32.  Were the plane layout not taken the kernel would read the planes as fp32 rows."""
    run_dx(DC.DX_PLANES, mode, operand)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lirec_embed_dx_indexed
# ---------------------------------------------------------------------------------------------------------------------------
def piece_head(J, dims):
    offs = [sum(dims[:i]) for i in range(4)]
    return DC.Head('plain', J, tuple(zip(offs, dims)))


@pytest.mark.parametrize('mode', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('case', DC.DXI_CASES, ids=[c.id for c in DC.DXI_CASES])
def test_embed_dx_indexed_against_fp64(case, mode):
    c = case
    inp = DC.dxi_inputs(c)
    dims = (c.td, c.vd, c.kd, c.kd)
    h = piece_head(c.J, dims)
    with gemm_mode(mode):
        clip, track = nans(c.n_clip + 1, c.td + c.vd), nans(c.n_track + 1, c.kd)      # (the tables themselves are not read)
        index = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
        pc = ops.make_pieces(clip, track, index, c.td, c.vd)
        ws = nans(4)
        args = [bwd_args(h, None, 0, 1, sum(dims), ws, rows=r) for r in c.rows]
        S = [s.to(DEV) for s in inp['S']]
        W1 = [[w.to(DEV) for w in ws_] for ws_ in inp['W1']]
        dClip, dTrack = nans(*clip.shape), nans(*track.shape)
        ops.embed_dx_indexed(args, S, W1, pc, dClip, dTrack)
        torch.cuda.synchronize()
    DC.check_dxi(dClip.cpu(), dTrack.cpu(), inp, mode, '%s mode %d' % (c.name, mode))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. lirec_embed_dw1_indexed
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('case', DC.DW1_CASES, ids=[c.id for c in DC.DW1_CASES])
def test_embed_dw1_indexed_against_fp64(case, mode):
    c = case
    inp = DC.dw1_inputs(c)
    J, nc1, nt1 = c.J, c.n_clip + 1, c.n_track + 1
    tag = '%s mode %d' % (c.name, mode)
    with gemm_mode(mode):
        try:
            ops.set_grad_overwrite(c.overwrite)
            clip, track, index = inp['clip'].to(DEV), inp['track'].to(DEV), inp['index'].to(DEV)
            pc = ops.make_pieces(clip, track, index, c.td, c.vd)
            args, Ps, Ss, grads = [], [], [], []
            for hd in inp['heads']:
                h = hd['h']
                if c.overwrite:
                    gW, gb = [nans(*w.shape) for w in hd['g0W']], [nans(*b.shape) for b in hd['g0b']]
                else:
                    gW, gb = [w.to(DEV) for w in hd['g0W']], [b.to(DEV) for b in hd['g0b']]
                if hd['empty']:
                    ws, rows = nans(4), 0
                    Ps.append(nans(4))
                    args.append(bwd_args(h, None, 0, c.rp1, sum(c.dims), ws, gW, gb, rows=0))
                else:
                    ws, rows = workspace(h, c.n), c.n * h.group
                    cnt = hd['L'].numel()
                    ws[:cnt * 4 * J] = hd['dz'].reshape(-1).to(DEV)
                    Ps.append(nans(rows * c.ldp))
                    args.append(bwd_args(h, hd, c.n, c.rp1, sum(c.dims), ws, gW, gb))
                Ss.append(nans((nc1 + nt1) * 2 * J))
                grads.append((gW, gb, ws))
            ops.embed_dw1_indexed(args, pc, Ps, Ss)
            torch.cuda.synchronize()
        finally:
            ops.set_grad_overwrite(False)
    for i, (hd, (gW, gb, _), S) in enumerate(zip(inp['heads'], grads, Ss)):
        if hd['empty']:
            # a head without rows: S not written, its gradients untouched (bit for bit the initial values, or the NaN pre-fill)
            assert bool(torch.isnan(S).all()), tag + ': S of the empty head written'
            for g, g0 in zip(gW + gb, hd['g0W'] + hd['g0b']):
                assert bool(torch.isnan(g).all()) if c.overwrite else torch.equal(g.cpu(), g0), tag + ': gradient of the empty head touched'
            continue
        DC.check_dw1(S.cpu(), [g.cpu() for g in gW], [g.cpu() for g in gb], hd, c, mode, '%s h%d' % (tag, i))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. lirec_embed_l1_indexed
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('case', DC.L1_CASES, ids=[c.id for c in DC.L1_CASES])
def test_embed_l1_indexed_against_fp64(case, mode):
    c = case
    inp = DC.l1_inputs(c)
    h = inp['h']
    J, rows, cnt = h.J, c.n * h.group, inp['L'].numel()
    tag = '%s mode %d' % (c.name, mode)
    with gemm_mode(mode):
        clip, track, index = inp['clip'].to(DEV), inp['track'].to(DEV), inp['index'].to(DEV)
        pc = ops.make_pieces(clip, track, index, c.td, c.vd)
        sel, pool, _ = head_pool(h, inp, c.n)
        segs = ops.Segments([o for o, _ in h.segs], [d for _, d in h.segs], [1] * 4)
        W1, b1 = [w.to(DEV) for w in inp['W1']], [b.to(DEV) for b in inp['b1']]
        H1 = nans(rows, 4 * J)
        a = ops.embed_fwd_args(dummy_x(), sum(c.dims), (sel[0], c.rp1, sel[2]), rows, J, segs, W1, b1, [], [], H1, None, 0, None, 0, 0,
                               ops.make_dropout(SEED, c.p, c.site, c.site + 2), pool=pool)
        zclip, ztrk = nans(c.n_clip + 1, 2 * J), nans(c.n_track + 1, 2 * J)
        ops.embed_l1_indexed([a], pc, [zclip], [ztrk])
        keep = ops.dropout_mask(rows, 4 * J, SEED, c.p, c.site, DEV) if c.p > 0 else torch.ones(rows, 4 * J, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
    got = H1.cpu()
    assert bool(torch.isnan(got[cnt:]).all()), tag + ': H1 written beyond the row count'
    assert cnt > 0
    flips = DC.check_h1(got[:cnt], inp, keep.cpu()[inp['L']], mode, tag, RELU_EPS, RELU_FRAC)
    print('%s: %d relu decisions differ from the float64 ones' % (tag, flips))
