"""Gradients of de-duplicated piece tables (lirec_embed_dx_indexed): a ``feature_pieces`` batch whose ``clip`` / ``track`` tables
require grad gets ``clip.grad`` / ``track.grad`` = d loss / d table, autograd through the reference's gather
(features.gather_reference) -- against the CPU oracle, against the block path's ``features.grad`` scattered onto the tables, with
exact zeros where the reference's block holds constants or masked rows, and the rest of the step bit-identical to a run whose
tables do not require grad."""
import numpy as np
import pytest
import torch

from golden_util import grad_close
from lirec_amd import _lib, config, ops
from lirec_amd import features as F
from lirec_amd._lib import LirecError
from lirec_amd.config import opt
from oracle import lirec_oracle as O
from test_gpu_bench_shape import DeviceReluDecisions, device_relu_decisions
from test_host_pieces_input_grad import R, scatter_block_grad, small_world_batch, table_gather

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 2], ids=['f32mfma', 'bf16x3'])
def gemm_mode(request):
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(_lib.default_gemm_mode())


def make_model(world, compact=True, planes=None, params=None, train=True):
    from lirec_amd import model as M
    config.recipe('int_rel_ch', rels_n_clips=R, dropout_seed=5)
    opt.device = 'cuda'
    opt.compact_ctx_rows = compact
    if planes is not None:
        opt.layer1_planes = planes
    torch.manual_seed(0)
    model, loss, optim = M.create_model(len(world.inter_names), n_rels=len(world.rel_names))
    if params is not None:
        model.load_state_dict(params, strict=True)
    model.train() if train else model.eval()
    return model, loss, optim


def pieces_step(model, loss, b, clip=None, track=None):
    """forward + loss + backward on an indexed batch; ``clip`` / ``track``: tables to put in (e.g. ones that require grad)"""
    pcs = dict(b['feature_pieces'])
    if clip is not None:
        pcs['clip'] = clip
    if track is not None:
        pcs['track'] = track
    b = dict(b, feature_pieces=pcs)
    out = model(b)
    lv = loss(out, b)
    lv.backward()
    torch.cuda.synchronize()
    return out, lv


def leaves(b, dtype=torch.float32):
    pcs = b['feature_pieces']
    return (pcs['clip'].detach().clone().to(dtype).requires_grad_(True), pcs['track'].detach().clone().to(dtype).requires_grad_(True))


def oracle_table_grad(world, batch, P, seed, relu, drop=True):
    NR = len(world.rel_names)
    cfg = O.OracleCfg()
    ct = batch['clip_table'].double().requires_grad_(True)
    tt = batch['track_table'].double().requires_grad_(True)
    hb = {k: v for k, v in batch.items() if k not in F.PIECE_KEYS}
    hb['features'] = table_gather(ct, tt, batch['feature_index'])
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    oo = O.model_forward(Pg, cfg, dict(hb), O.PhiloxDropout(seed, cfg.dropout) if drop else O.no_dropout, relu)
    O.loss_forward(cfg, oo, hb, NR).sum().backward()
    return ct.grad, tt.grad


@pytest.mark.parametrize('compact', [True, False])
def test_table_grad_matches_the_oracle(gemm_mode, compact):
    world, batch = small_world_batch(6)
    cfg = O.OracleCfg()
    P = O.fill_params(O.param_shapes(cfg, len(world.inter_names), len(world.rel_names)), 7)
    model, loss, _ = make_model(world, compact, params=P)
    model.debug_keep_state = True
    b = F.indexed_batch(batch, 'cuda')
    clip, track = leaves(b)
    pieces_step(model, loss, b, clip, track)
    assert clip.grad is not None and track.grad is not None
    assert clip.grad.dtype == torch.float32 and clip.grad.is_cuda and clip.grad.shape == clip.shape
    relu = DeviceReluDecisions(device_relu_decisions(model, int(model.last_dropout_seed), cfg.dropout))
    model.last_state = None
    oc, ot = oracle_table_grad(world, batch, P, int(model.last_dropout_seed), relu)
    grad_close(clip.grad, oc, 'dClip vs oracle')
    grad_close(track.grad, ot, 'dTrack vs oracle')


def block_vs_tables(batch, world, compact=True):
    """(table grads from the block path's features.grad scattered by the index, table grads of the pieces path); layer-1 planes
    off on both sides: the two forwards are bit-identical and take the same relu decisions"""
    res = []
    for mode in ('block', 'pieces'):
        model, loss, _ = make_model(world, compact, planes=False)
        if mode == 'block':
            b = F.gather_features(batch, 'cuda')
            f = b['features'].requires_grad_(True)
            loss(model(b), b).backward()
            torch.cuda.synchronize()
            res.append(scatter_block_grad(f.grad, batch['feature_index'], batch['clip_table'].shape, batch['track_table'].shape))
        else:
            b = F.indexed_batch(batch, 'cuda')
            clip, track = leaves(b)
            pieces_step(model, loss, b, clip, track)
            res.append((clip.grad, track.grad))
        del model, loss
    return res


@pytest.mark.parametrize('compact', [True, False])
def test_table_grad_matches_the_block_path(compact):
    world, batch = small_world_batch(8)
    (bc, bt), (pc, pt) = block_vs_tables(batch, world, compact)
    grad_close(pc, bc, 'dClip vs scattered block dX')
    grad_close(pt, bt, 'dTrack vs scattered block dX')


def test_exact_zeros():
    """the tables' zero rows, a piece that only masked context rows name, and a piece no row names: exactly 0"""
    world, batch = small_world_batch(8)
    ct, idx = batch['clip_table'], batch['feature_index'].clone()
    nc = ct.shape[0] - 1
    m = batch['rels_mask'] == 0                               # (B, T, R): masked context rows
    assert m.any()
    where = m.nonzero()[:3]
    for b_, t_, r_ in where.tolist():
        idx[b_, t_, r_ + 1, 0] = nc                           # -> the planted piece nc (masked uses only)
    g = torch.Generator().manual_seed(3)
    planted = torch.rand((2, ct.shape[1]), generator=g) + 0.5  # nc: masked uses only; nc + 1: no use at all
    batch = dict(batch, clip_table=torch.cat([ct[:-1], planted, ct[-1:]]), feature_index=idx)
    for compact in (True, False):
        model, loss, _ = make_model(world, compact)
        b = F.indexed_batch(batch, 'cuda')
        clip, track = leaves(b)
        pieces_step(model, loss, b, clip, track)
        gc, gt = clip.grad.cpu(), track.grad.cpu()
        for rows, what in ((gc[-1], 'clip zero row'), (gt[-1], 'track zero row'), (gc[nc], 'masked-only piece'),
                           (gc[nc + 1], 'unused piece')):
            assert torch.equal(rows, torch.zeros_like(rows)), (what, compact)
        assert gc[:nc].abs().sum(-1).max() > 0 and gt[:-1].abs().sum(-1).max() > 0


def test_step_bit_identical_to_the_no_grad_tables():
    """logits, loss and every parameter gradient: tables that require grad (defaults: routed to the once-per-piece path) against
    tables that do not, with opt.pieces_q32b = False; and the no-grad tables under the defaults still take the q32b path"""
    world, batch = small_world_batch(8)
    res = []
    for how in ('plain', 'grad', 'plain_default'):
        model, loss, optim = make_model(world)
        assert opt.pieces_q32b and opt.layer1_planes
        if how == 'plain':
            opt.pieces_q32b = False
        optim.zero_grad()
        b = F.indexed_batch(batch, 'cuda')
        out, lv = pieces_step(model, loss, b, *(leaves(b) if how == 'grad' else ()))
        res.append((out['inters'].detach().clone(), out['rels'].detach().clone(), lv.detach().clone(),
                    {k: p.grad.detach().clone() for k, p in model.named_parameters()}, model.last_layer1_planes))
    (a, g, d) = res
    for x, y in zip(a[:3], g[:3]):
        assert torch.equal(x, y)
    for k in a[3]:
        assert torch.equal(a[3][k], g[3][k]), k
    assert not a[4] and not g[4]                # (no layer-1 planes: the once-per-piece path)
    assert d[4]                                 # (the q32b operand rows staged from the tables, as before)


def test_autograd_composition():
    world, batch = small_world_batch(6)
    cfg = O.OracleCfg()
    P = O.fill_params(O.param_shapes(cfg, len(world.inter_names), len(world.rel_names)), 7)
    NR = len(world.rel_names)
    # an adapter on the raw clip pieces (then the zero row): its weights get the oracle's gradient
    cd = batch['clip_table'].shape[1]
    torch.manual_seed(0)
    W0 = (torch.randn(cd, cd) / cd ** 0.5).float()
    b0 = (torch.randn(cd) * 0.01).float()
    model, loss, _ = make_model(world, params=P)
    model.debug_keep_state = True
    ad = torch.nn.Linear(cd, cd).cuda()
    with torch.no_grad():
        ad.weight.copy_(W0); ad.bias.copy_(b0)
    b = F.indexed_batch(batch, 'cuda')
    raw = b['feature_pieces']['clip'][:-1]
    clip = torch.cat([ad(raw), raw.new_zeros((1, cd))])
    pieces_step(model, loss, b, clip)
    relu = DeviceReluDecisions(device_relu_decisions(model, int(model.last_dropout_seed), cfg.dropout))
    model.last_state = None
    Wo, bo = W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    ct = batch['clip_table'].float()
    oc = torch.cat([ct[:-1] @ Wo.t() + bo, ct.new_zeros((1, cd))])
    hb = {k: v for k, v in batch.items() if k not in F.PIECE_KEYS}
    hb['features'] = table_gather(oc, batch['track_table'].float(), batch['feature_index'])
    oo = O.model_forward({k: v.clone().requires_grad_(True) for k, v in P.items()}, cfg, dict(hb),
                         O.PhiloxDropout(int(model.last_dropout_seed), cfg.dropout), relu)
    O.loss_forward(cfg, oo, hb, NR).sum().backward()
    grad_close(ad.weight.grad, Wo.grad, 'adapter weight grad')
    grad_close(ad.bias.grad, bo.grad, 'adapter bias grad')

    # leaves of other dtypes: gradients of their own dtype (float64 from the same fp32 values: the same numbers)
    model, loss, _ = make_model(world, params=P)
    b = F.indexed_batch(batch, 'cuda')
    c32, t32 = leaves(b)
    pieces_step(model, loss, b, c32, t32)
    model, loss, _ = make_model(world, params=P)
    c64, t64 = leaves(b, torch.float64)
    pieces_step(model, loss, b, c64, t64)
    assert c64.grad.dtype == torch.float64 and t64.grad.dtype == torch.float64
    assert torch.equal(c64.grad, c32.grad.double()) and torch.equal(t64.grad, t32.grad.double())
    model, loss, _ = make_model(world, params=P)
    c16, t16 = leaves(b, torch.bfloat16)
    pieces_step(model, loss, b, c16, t16)
    assert c16.grad.dtype == torch.bfloat16 and t16.grad.dtype == torch.bfloat16 and c16.grad.shape == c16.shape
    assert c16.grad.float().abs().sum() > 0 and torch.isfinite(c16.grad.float()).all()

    # a host table through indexed_batch: its gradient on the CPU
    model, loss, _ = make_model(world, params=P)
    hbatch = dict(batch, clip_table=batch['clip_table'].clone().requires_grad_(True))
    b = F.indexed_batch(hbatch, 'cuda')
    assert b['feature_pieces']['clip'].requires_grad
    out = model(b)
    loss(out, b).backward()
    torch.cuda.synchronize()
    g = hbatch['clip_table'].grad
    assert g is not None and g.device.type == 'cpu' and g.dtype == torch.float32
    assert torch.equal(g, c32.grad.cpu())

    # two backward passes accumulate (eval mode: the same computation twice)
    model, loss, _ = make_model(world, params=P, train=False)
    b = F.indexed_batch(batch, 'cuda')
    clip, track = leaves(b)
    pieces_step(model, loss, b, clip, track)
    g1 = clip.grad.clone(), track.grad.clone()
    pieces_step(model, loss, b, clip, track)
    assert torch.equal(clip.grad, 2 * g1[0]) and torch.equal(track.grad, 2 * g1[1])


def test_eval_saliency_matches_the_oracle():
    """model.eval() (p = 0) under enable_grad: saliency over the pieces"""
    world, batch = small_world_batch(6)
    cfg = O.OracleCfg()
    P = O.fill_params(O.param_shapes(cfg, len(world.inter_names), len(world.rel_names)), 7)
    model, loss, _ = make_model(world, params=P, train=False)
    model.debug_keep_state = True
    b = F.indexed_batch(batch, 'cuda')
    clip, track = leaves(b)
    with torch.enable_grad():
        pieces_step(model, loss, b, clip, track)
    relu = DeviceReluDecisions(device_relu_decisions(model, 0, 0.0))
    model.last_state = None
    oc, ot = oracle_table_grad(world, batch, P, 0, relu, drop=False)
    grad_close(clip.grad, oc, 'eval dClip')
    grad_close(track.grad, ot, 'eval dTrack')


def test_recorded_step_refuses_tables_that_require_grad():
    from lirec_amd.graph import RecordedTrainStep
    world, batch = small_world_batch(8)
    model, loss, optim = make_model(world)
    b = F.indexed_batch(batch, 'cuda')
    b['feature_pieces'] = dict(b['feature_pieces'], clip=b['feature_pieces']['clip'].requires_grad_(True))
    with pytest.raises(LirecError):
        RecordedTrainStep(model, loss, optim, b)


def test_bench_world_table_grad_matches_the_block_path():
    """64 shuffled clips of bench.py's pieces world (T = 20, R = 18), GEMM mode 2: against the block path's dX scattered"""
    wd = F.synthetic_world(4321, n_scenes=256, per_scene=8, n_rel_names=15, n_inter_names=101)
    ds = F.PiecesDataset(wd, R, 101, pin_memory=False)
    pick = torch.randperm(len(ds), generator=torch.Generator().manual_seed(7))[:64].tolist()
    batch = ds.collate_fn([ds[i] for i in pick])
    assert batch['feature_index'].shape[1] == 20
    ops.set_gemm_mode(2)
    try:
        (bc, bt), (pc, pt) = block_vs_tables(batch, wd)
    finally:
        ops.set_gemm_mode(_lib.default_gemm_mode())
    grad_close(pc, bc, 'bench world dClip vs scattered block dX')
    grad_close(pt, bt, 'bench world dTrack vs scattered block dX')
    assert torch.equal(pc[-1].cpu(), torch.zeros_like(pc[-1].cpu())) and torch.equal(pt[-1].cpu(), torch.zeros_like(pt[-1].cpu()))
