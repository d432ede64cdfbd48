"""The gradient of de-duplicated piece tables (lirec_embed_dx_indexed) without a GPU: the ABI of the new call, its argument checks
(LIREC_EINVAL before any device call), and the yardstick the GPU tests use -- on the CPU oracle, the block gradient scattered
onto the tables by the index is the tables' own autograd gradient through the gather."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from golden_util import grad_close
from lirec_amd import _lib
from lirec_amd import features as F
from oracle import lirec_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 18


def test_abi_of_the_new_call():
    L = _lib.lib()
    assert L.lirec_abi_sizeof(9) == C.sizeof(_lib.EmbedDxIndexedArgs)
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    hdr = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    assert re.search(r'\blirec_embed_dx_indexed\s*\(', hdr)
    assert 'lirec_embed_dx_indexed' in _lib.EXPORTS and hasattr(L, 'lirec_embed_dx_indexed')


def _valid_args():
    """A well-formed argument set over fake (aligned, never dereferenced) device addresses: each case below breaks ONE thing of it,
    so that the call must return before it reaches the device."""
    td, vd, kd, J = 768, 2048, 2048, 512
    pc = _lib.Pieces(0x10000, td + vd, 40, 0x20000, kd, 70, 0x30000, td, vd, kd)
    heads = []
    for h in range(2):
        b = _lib.EmbedBwdArgs()
        b.nseg, b.J, b.rows = 4, J, 64 * (1 if h == 0 else R)
        for i, (off, dim) in enumerate(((0, td), (td, vd), (td + vd, kd), (td + vd + kd, kd))):
            b.in_off[i], b.in_dim[i], b.out_dim[i] = off, dim, J if i < 2 else J // 2
        heads.append(b)
    a = _lib.EmbedDxIndexedArgs()
    a.nh = 2
    for h in range(2):
        a.heads[h] = C.pointer(heads[h])
        a.S[h] = 0x100000 * (h + 1)
        for i in range(4):
            a.W1[h][i] = 0x1000000 + 0x100000 * (4 * h + i)
    a.pieces = C.pointer(pc)
    a.dClip, a.ld_clip = 0x4000000, td + vd
    a.dTrack, a.ld_track = 0x5000000, kd
    a._keep = (pc, heads)
    return a, pc, heads


def _break(what):
    a, pc, heads = _valid_args()
    if what == 'nh0':
        a.nh = 0
    elif what == 'nh3':
        a.nh = 3
    elif what == 'pieces':
        a.pieces = C.POINTER(_lib.Pieces)()
    elif what == 'head':
        a.heads[1] = C.POINTER(_lib.EmbedBwdArgs)()
    elif what == 'S':
        a.S[1] = None
    elif what == 'S_misaligned':
        a.S[0] = 0x100004
    elif what == 'W1':
        a.W1[0][2] = None
    elif what == 'W1_misaligned':
        a.W1[1][3] += 8
    elif what == 'dClip':
        a.dClip = None
    elif what == 'dTrack_misaligned':
        a.dTrack += 4
    elif what == 'ld_clip_short':
        a.ld_clip = pc.text_dim + pc.visual_dim - 4
    elif what == 'ld_track_odd':
        a.ld_track = pc.track_dim + 2
    elif what == 'nseg':
        heads[0].nseg = 3
    elif what == 'J_odd':
        heads[0].J = heads[1].J = 510
    elif what == 'J_differs':
        heads[1].J = 256
    elif what == 'in_dim':
        heads[1].in_dim[1] = pc.visual_dim - 4
    elif what == 'dims_odd':
        pc.text_dim = heads[0].in_dim[0] = heads[1].in_dim[0] = 766
        a.ld_clip = 766 + pc.visual_dim + 2
    elif what == 'no_pieces_rows':
        pc.n_track = 0
    return a


CASES = ('nh0', 'nh3', 'pieces', 'head', 'S', 'S_misaligned', 'W1', 'W1_misaligned', 'dClip', 'dTrack_misaligned', 'ld_clip_short',
         'ld_track_odd', 'nseg', 'J_odd', 'J_differs', 'in_dim', 'dims_odd', 'no_pieces_rows')


@pytest.mark.parametrize('what', CASES)
def test_argument_checks_return_einval_without_a_device(what):
    L = _lib.lib()
    a = _break(what)
    assert L.lirec_embed_dx_indexed(C.byref(a), None) == _lib.LIREC_EINVAL
    assert L.lirec_embed_dx_indexed(None, None) == _lib.LIREC_EINVAL


def table_gather(clip, track, idx):
    """Differentiable statement of features.gather_reference: the (..., cd + 2 td) block from the tables and the index, the
    constant 0 where an index is negative (the tables' trailing zero row is never read)."""
    def take(tab, i):
        i = torch.as_tensor(i).long()
        return torch.where((i >= 0).unsqueeze(-1), tab[i.clamp(min=0)], tab.new_zeros(()))
    return torch.cat([take(clip, idx[..., 0]), take(track, idx[..., 1]), take(track, idx[..., 2])], -1)


def scatter_block_grad(g, idx, clip_shape, track_shape):
    """d loss / d tables from d loss / d block: the block gradient summed onto the rows the index names (float64, negative
    indices dropped)."""
    cd, td = clip_shape[1], track_shape[1]
    g = torch.as_tensor(g).detach().cpu().double().reshape(-1, cd + 2 * td)
    idx = torch.as_tensor(idx).cpu().long().reshape(-1, 3)
    dc = torch.zeros(clip_shape, dtype=torch.float64)
    dt = torch.zeros(track_shape, dtype=torch.float64)
    m = idx[:, 0] >= 0
    dc.index_add_(0, idx[m, 0], g[m, :cd])
    for part in (1, 2):
        m = idx[:, part] >= 0
        dt.index_add_(0, idx[m, part], g[m, cd + (part - 1) * td:cd + part * td])
    return dc, dt


def small_world_batch(n=6):
    world = F.synthetic_world(3, n_scenes=4, per_scene=3)
    class_of = {nm: k for k, nm in enumerate(world.inter_names)}
    samples = [F.assemble_sample(world, i, R, len(world.inter_names), class_of) for i in range(n)]
    return world, F.collate(world, samples)


def test_gather_reference_statement():
    _, batch = small_world_batch()
    blk = table_gather(batch['clip_table'].double(), batch['track_table'].double(), batch['feature_index'])
    assert torch.equal(blk, F.gather_reference(batch))


def test_scattered_block_grad_is_the_oracle_table_grad():
    """The yardstick of tests/test_gpu_pieces_input_grad.py: on the oracle alone, scatter-adding the block gradient by the index
    gives what autograd gives through the gather."""
    world, batch = small_world_batch()
    C_, NR = len(world.inter_names), len(world.rel_names)
    cfg = O.OracleCfg()
    P = O.fill_params(O.param_shapes(cfg, C_, NR), 7)
    hb = {k: v for k, v in batch.items() if k not in F.PIECE_KEYS}
    res = {}
    for how in ('block', 'tables'):
        ct = batch['clip_table'].double().requires_grad_(how == 'tables')
        tt = batch['track_table'].double().requires_grad_(how == 'tables')
        blk = table_gather(ct, tt, batch['feature_index'])
        if how == 'block':
            blk = blk.detach().requires_grad_(True)
        ob = dict(hb, features=blk)
        oo = O.model_forward({k: v.clone().requires_grad_(True) for k, v in P.items()}, cfg, dict(ob), O.PhiloxDropout(5, cfg.dropout))
        O.loss_forward(cfg, oo, ob, NR).sum().backward()
        res[how] = scatter_block_grad(blk.grad, batch['feature_index'], ct.shape, tt.shape) if how == 'block' else (ct.grad, tt.grad)
    for a, b, what in zip(res['tables'], res['block'], ('clip', 'track')):
        assert a.abs().sum() > 0
        grad_close(a, b, 'oracle table grad vs scattered block grad: ' + what)
        assert torch.equal(a[-1], torch.zeros_like(a[-1]))          # the trailing zero row
