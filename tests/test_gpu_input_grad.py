"""Input-feature gradients (lirec_embed_dx): ``batch['features'].requires_grad_(True)`` -> ``features.grad`` = d loss / d features,
as the reference's plain-PyTorch module gives it through autograd (its ``.float()`` / ``.cuda()`` are differentiable).

Compared with the reference's own gradients (tests/golden/input_grad/cells.npz, tools/make_golden_input_grad.py) and with the CPU
oracle's autograd dX at the gradient tolerance of golden_util.grad_close; exact zeros where the reference multiplies by 0; and
the rest of the step bit-identical to a run whose features do not require grad.
"""
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, Cell, grad_close
from lirec_amd import _lib, config, ops
from lirec_amd._lib import LirecError
from lirec_amd.config import opt
from oracle import lirec_oracle as O
from test_gpu_bench_shape import N_CLASSES, N_RELS, PARAM_SEED, SEED, DeviceReluDecisions, device_relu_decisions, host_batch
from test_gpu_parity import setup_cell

pytestmark = pytest.mark.gpu

CELLS = ('modalties_m', 'modalties_t', 'int_rels_train', 'int_rels_nogate', 'int_ch_train', 'int_rel_ch_train',
         'int_rel_ch_cat_train', 'full_int_rel_ch')
REF = dict(np.load(os.path.join(GOLDEN, 'input_grad', 'cells.npz')))


@pytest.fixture(params=[0, 2], ids=['f32mfma', 'bf16x3'])
def gemm_mode(request):
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(_lib.default_gemm_mode())


def hip_input_grad(cell, batch=None, mode_eval=None):
    model, loss, _ = setup_cell(cell)
    if mode_eval:
        model.eval()
    batch = cell.batch() if batch is None else batch
    f = batch['features'].requires_grad_(True)
    out = model(batch)
    lv = loss(out, batch)
    lv.sum().backward()
    torch.cuda.synchronize()
    return f, model, lv


def oracle_input_grad(cell, drop=None):
    P = {k: v.clone().requires_grad_(True) for k, v in cell.params().items()}
    ob = cell.batch()
    f = ob['features'].requires_grad_(True)
    oo = O.model_forward(P, cell.ocfg, ob, cell.dropout() if drop is None else drop)
    ol = O.loss_forward(cell.ocfg, oo, ob, cell.n_rels, sampler=cell.sampler(), use_ce=cell.use_ce)
    ol.sum().backward()
    return f.grad.detach().clone()


@pytest.mark.parametrize('name', CELLS)
def test_input_grad_matches_reference_and_oracle(name, gemm_mode):
    cell = Cell(name)
    f, _, _ = hip_input_grad(cell)
    assert f.grad is not None, 'features.grad is None'
    assert f.grad.dtype == torch.float64 and f.grad.device.type == 'cpu' and f.grad.shape == f.shape
    og = oracle_input_grad(cell)
    grad_close(f.grad, og, 'dX vs oracle')
    if name + '/norm' in REF:
        n = float(REF[name + '/norm'])
        assert abs(og.double().norm().item() - n) <= 1e-4 * n, 'oracle dX norm vs reference'
        assert abs(f.grad.double().norm().item() - n) <= 2e-4 * n
        head = torch.from_numpy(REF[name + '/head']).double()
        grad_close(f.grad.reshape(-1, f.shape[-1])[:4], head, 'dX head vs reference')
    else:
        grad_close(f.grad, torch.from_numpy(REF[name]), 'dX vs reference')


def test_exact_zeros_unused_segments_and_masked_rows():
    # modality 't': only the text columns reach the model (mlp/model.py:54-92)
    cell = Cell('modalties_t')
    f, _, _ = hip_input_grad(cell)
    td = cell.cfg['text_dim']
    assert torch.equal(f.grad[..., td:], torch.zeros_like(f.grad[..., td:]))
    assert torch.equal(f.grad[:, 1:], torch.zeros_like(f.grad[:, 1:]))            # rows the Modalities head does not read
    assert f.grad[:, 0, :td].abs().sum() > 0
    # masked context rows: exactly 0 (the reference multiplies them by the mask), with and without compaction
    cell = Cell('int_rel_ch_train')
    for compact in (True, False):
        model, loss, _ = setup_cell(cell)
        opt.compact_ctx_rows = compact
        batch = cell.batch()
        f = batch['features'].requires_grad_(True)
        m = batch['rels_mask'].clone()
        lv = loss(model(batch), batch)
        lv.sum().backward()
        g = f.grad.reshape(-1, f.shape[-2], f.shape[-1])
        masked = (m.reshape(-1, m.shape[-1]) == 0)
        assert masked.any()
        assert torch.equal(g[:, 1:][masked], torch.zeros_like(g[:, 1:][masked])), compact
        assert g[:, 1:][~masked].abs().sum(-1).min() > 0
        # padded candidate pairs (no track: their logits are masked to -inf by the loss): the reference's gradient is 0 there too
        og = oracle_input_grad(cell).reshape(g.shape)
        zero_rows = (og == 0).all(-1)
        assert torch.equal(g[zero_rows], torch.zeros_like(g[zero_rows]))


def test_step_unchanged_by_requires_grad():
    """logits, loss and every parameter gradient bit-identical with and without requires_grad on the features"""
    cell = Cell('int_rel_ch_train')
    res = []
    for rg in (False, True):
        model, loss, _ = setup_cell(cell)
        batch = cell.batch()
        if rg:
            batch['features'].requires_grad_(True)
        out = model(batch)
        logits = out['inters'].detach().clone(), out['rels'].detach().clone()
        lv = loss(out, batch)
        lv.sum().backward()
        res.append((logits, lv.detach().cpu(), model.flat_grads().detach().cpu().clone()))
    assert torch.equal(res[0][0][0], res[1][0][0]) and torch.equal(res[0][0][1], res[1][0][1])
    assert torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])


def test_leaf_dtypes_autograd_grad_and_accumulation():
    cell = Cell('int_rel_ch_train')
    f64, _, _ = hip_input_grad(cell)
    # a resident fp32 leaf: the same numbers as the loader's float64 leaf, in fp32 on the device
    b = cell.batch()
    b['features'] = b['features'].float().cuda()
    f32, _, _ = hip_input_grad(cell, batch=b)
    assert f32.grad.dtype == torch.float32 and f32.grad.is_cuda
    assert torch.equal(f64.grad, f32.grad.cpu().double())
    # bf16 leaf: bf16 gradient
    b = cell.batch()
    b['features'] = b['features'].to(torch.bfloat16).cuda()
    fb, _, _ = hip_input_grad(cell, batch=b)
    assert fb.grad.dtype == torch.bfloat16 and fb.grad.shape == fb.shape and fb.grad.float().abs().sum() > 0
    # torch.autograd.grad
    model, loss, _ = setup_cell(cell)
    b = cell.batch()
    f = b['features'].requires_grad_(True)
    (g,) = torch.autograd.grad(loss(model(b), b).sum(), f)
    assert torch.equal(g, f64.grad)
    # two backward passes accumulate (eval mode: the two passes are the same computation, so the sum is exactly twice one pass)
    model, loss, _ = setup_cell(cell)
    model.eval()
    b = cell.batch()
    f = b['features'].requires_grad_(True)
    loss(model(dict(b)), b).sum().backward()
    g1 = f.grad.clone()
    loss(model(dict(b)), b).sum().backward()
    assert torch.equal(f.grad, 2 * g1)


def test_eval_saliency_matches_oracle():
    """model.eval() (p = 0) under enable_grad: saliency on a trained model"""
    cell = Cell('int_rel_ch_train')
    with torch.enable_grad():
        f, _, _ = hip_input_grad(cell, mode_eval=True)
    grad_close(f.grad, oracle_input_grad(cell, drop=O.no_dropout), 'eval dX')


def test_adapter_in_front_gets_the_oracle_gradient():
    cell = Cell('int_rel_ch_train')
    D = cell.ocfg.mlp_dim
    torch.manual_seed(0)
    lin = torch.nn.Linear(D, D).double()
    W0, b0 = lin.weight.detach().clone(), lin.bias.detach().clone()
    # device: adapter on the GPU in fp32
    model, loss, _ = setup_cell(cell)
    ad = torch.nn.Linear(D, D).cuda()
    with torch.no_grad():
        ad.weight.copy_(W0.float()); ad.bias.copy_(b0.float())
    b = cell.batch()
    b['features'] = ad(b['features'].float().cuda())
    loss(model(b), b).sum().backward()
    # oracle: the same graph on the CPU
    P = {k: v.clone().requires_grad_(True) for k, v in cell.params().items()}
    ob = cell.batch()
    Wo, bo = W0.float().requires_grad_(True), b0.float().requires_grad_(True)
    ob['features'] = ob['features'].float() @ Wo.t() + bo
    oo = O.model_forward(P, cell.ocfg, ob, cell.dropout())
    O.loss_forward(cell.ocfg, oo, ob, cell.n_rels, sampler=cell.sampler()).sum().backward()
    grad_close(ad.weight.grad, Wo.grad, 'adapter weight grad')
    grad_close(ad.bias.grad, bo.grad, 'adapter bias grad')


def test_single_pass_mode_and_recorded_step_refuses():
    """GEMM mode 3 on a bf16 leaf (the context head's dZ1 then exists as its bf16 hi plane only) against the oracle on the same bf16
    inputs, rounded weights and device relu decisions.  dX sits at the END of the single-pass backward chain, behind the hidden-layer
    gradients that tests/test_gpu_onepass.py holds to 1e-2 of their scale: measured 1.46e-2 of dX's scale on this cell, so the bar
    here is 2e-2 (mode 3 is outside the 1e-4 parity contract by design)."""
    cell = Cell('full_int_rel_ch')
    b = cell.batch()
    b['features'] = b['features'].to(torch.bfloat16).cuda()
    from test_gpu_onepass import RELU_TOL, ROUNDED
    ops.set_gemm_mode(3)
    try:
        model, loss, _ = setup_cell(cell)
        model.debug_keep_state = True
        f = b['features'].requires_grad_(True)
        loss(model(b), b).sum().backward()
        torch.cuda.synchronize()
        # (the oracle takes the device's relu decisions: with operands rounded to bf16 a few pre-activations near 0 fall on the
        #  other side, each shifting the upstream gradients by a rank-one term -- tests/test_gpu_bench_shape.py)
        relu = DeviceReluDecisions(device_relu_decisions(model, int(cell.fx['dropout_seed']), cell.cfg['dropout']), **RELU_TOL)
        model.last_state = None
    finally:
        ops.set_gemm_mode(_lib.default_gemm_mode())
    assert f.grad.dtype == torch.bfloat16
    P = {k: v.clone().requires_grad_(True) for k, v in cell.params().items()}
    # (the single pass rounds the first-layer and gate weights to bf16 inside its GEMMs: so does the oracle, straight-through, as
    #  tests/test_gpu_onepass.py)
    Pu = {k: (v + (v.detach().to(torch.bfloat16).to(v.dtype) - v.detach()) if k in ROUNDED else v) for k, v in P.items()}
    ob = cell.batch()
    fo = ob['features'].to(torch.bfloat16).float().requires_grad_(True)
    ob['features'] = fo
    oo = O.model_forward(Pu, cell.ocfg, ob, cell.dropout(), relu)
    O.loss_forward(cell.ocfg, oo, ob, cell.n_rels, sampler=cell.sampler()).sum().backward()
    og = fo.grad
    err = (f.grad.float().cpu() - og).abs().max().item() / og.abs().max().item()
    assert err <= 2e-2, err
    from lirec_amd.graph import RecordedTrainStep
    config.recipe('int_rel_ch', rels_n_clips=3)
    opt.device = 'cuda'
    from lirec_amd import model as M
    from lirec_amd.data import synthetic_batch, to_device_batch
    model, loss, optim = M.create_model(N_CLASSES, n_rels=N_RELS)
    model.train()
    b = to_device_batch(synthetic_batch(SEED, 'int_rel_ch', 4, T=4, R=3), 'cuda')
    b['features'].requires_grad_(True)
    with pytest.raises(LirecError):
        RecordedTrainStep(model, loss, optim, b)


@pytest.mark.parametrize('fill,compact', [('survey', True), ('survey', False), ('dense', True)])
def test_bench_shape_input_grad(fill, compact):
    """B=64, T=16, R=18, int_rel_ch, train mode with dropout: dX against the oracle's autograd dX (device relu decisions)"""
    from lirec_amd import model as M
    from lirec_amd.data import to_device_batch
    B, T, R = 64, 16, 18
    cfg = O.OracleCfg()
    hb = host_batch(B, T, R, fill)
    config.recipe('int_rel_ch', dropout_seed=SEED, rels_n_clips=R)
    opt.device = 'cuda'
    opt.compact_ctx_rows = compact
    model, loss, _ = M.create_model(N_CLASSES, n_rels=N_RELS)
    model.load_state_dict(O.fill_params(O.param_shapes(cfg, N_CLASSES, N_RELS), PARAM_SEED), strict=True)
    model.train()
    model.debug_keep_state = True
    batch = to_device_batch(hb, 'cuda')
    f = batch['features'].requires_grad_(True)
    lv = loss(model(dict(batch)), batch)
    lv.sum().backward()
    torch.cuda.synchronize()
    g = f.grad.detach().cpu()
    relu = DeviceReluDecisions(device_relu_decisions(model, SEED, cfg.dropout))
    model.last_state = None
    del model, loss, batch, f
    torch.cuda.empty_cache()
    P = O.fill_params(O.param_shapes(cfg, N_CLASSES, N_RELS), PARAM_SEED)
    fo = hb['features'].float().requires_grad_(True)
    ob = dict(hb, features=fo)
    oo = O.model_forward(P, cfg, ob, O.PhiloxDropout(SEED, cfg.dropout), relu)
    O.loss_forward(cfg, oo, ob, N_RELS).sum().backward()
    grad_close(g, fo.grad, 'bench-shape dX')
    m = hb['rels_mask'].reshape(B * T, R) == 0
    gz = g.reshape(B * T, R + 1, -1)[:, 1:][m]
    assert torch.equal(gz, torch.zeros_like(gz))
