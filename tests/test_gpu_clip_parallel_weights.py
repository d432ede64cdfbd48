"""Clip weights under data parallelism: two ranks on one GPU (gloo, as tests/test_gpu_parallel.py), each with half of a batch
whose weight sums differ between the halves.  With ``clip_weight_norm='sum'`` the loss kernels divide by the all-reduced GLOBAL
weight sums over world (``DataParallel(model, optimizer, loss=loss)``), so the averaged gradient is the single process's on the
whole batch -- for MultiTaskMaxMargin (whose relationship mean runs over the labelled clips' weights) and for
MarginTrackRelsLoss (a plain weighted mean: the divisors are needed although the local batches are even)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)
KINDS = {'mtmm': 'int_rels', 'mtr': 'int_rel_ch'}
STEP_TIMEOUT = 240                 # seconds a rank's result, and then its exit, are waited for


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make(form):
    from lirec_amd import config
    from lirec_amd.config import opt
    config.recipe(KINDS[form], joint_dim=16, rels_n_clips=3, dropout=0.0, dropout_seed=77, clip_weight_norm='sum', **DIMS)
    opt.device = 'cuda'
    torch.manual_seed(11)
    from lirec_amd import model as M
    model, loss, optim = M.create_model(11, n_rels=5)
    optim.param_groups[0]['lr'] = 1e-3
    model.train()
    return model, loss, optim


def _weights():
    """rank 0's clips weigh 0.85 together, rank 1's 32.5 (one of them 0)"""
    return torch.tensor([0.25, 0.5, 0.05, 0.05, 4.0, 0.0, 20.0, 8.5], dtype=torch.float64)


def _batch(form, lo, hi, weighted=True):
    from lirec_amd.data import synthetic_batch, to_device_batch
    kw = dict(T=6) if form == 'mtr' else {}
    b = synthetic_batch(23, KINDS[form], 8, R=3, n_classes=11, n_rels=5, **DIMS, **kw)
    if form == 'mtmm':                               # labelled clips unequally spread, as tests/test_gpu_parallel.py
        r = b['rels_label'].clone()
        r[:4], r[4:] = torch.tensor([0, 1, 2, 3]), torch.tensor([5, 4, 5, 2])
        b['rels_label'] = r
    if weighted:
        b['clip_weight'] = _weights()
    b = {k: (v[lo:hi].clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    return to_device_batch(b, 'cuda')


def _steps(model, loss, optim, batch, n=2):
    grads = None
    for i in range(n):
        optim.zero_grad()
        lv = loss(model(dict(batch)), batch)
        lv.backward()
        if model.grad_sync is not None:
            model.grad_sync.wait()
        if i == 0:
            grads, first = model.flat_grads(attach=False).detach().clone() * optim.grad_scale, lv.detach().sum()
        optim.step()
    torch.cuda.synchronize()
    return grads.cpu(), model.flat_params().detach().cpu().clone(), float(first)


def _worker(rank, world, port, form, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from lirec_amd.parallel import DataParallel
        per = 8 // world
        model, loss, optim = _make(form)
        DataParallel(model, optim, loss=loss, sharded=False)
        g, p, l = _steps(model, loss, optim, _batch(form, rank * per, (rank + 1) * per))
        q.put((rank, g.numpy(), p.numpy(), l))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('form', ['mtmm', 'mtr'])
def test_weighted_mean_two_ranks_equal_single_process(form):
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')                     # fresh processes
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, form, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=STEP_TIMEOUT) for _ in range(world)], key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    model, loss, optim = _make(form)
    g_ref, p_ref, l_ref = _steps(model, loss, optim, _batch(form, 0, 8))
    # for scale: each rank dividing by its own weight sums, averaged -- what the loss computes without the global divisors -- and
    # the unweighted step
    naive = []
    for r in range(world):
        m_, l_, o_ = _make(form)
        naive.append(_steps(m_, l_, o_, _batch(form, 4 * r, 4 * r + 4), 1)[0])
    scale = float(g_ref.abs().max())
    assert float((sum(naive) / world - g_ref).abs().max()) > 1e-2 * scale, 'the case was meant to separate the two forms'
    m_, l_, o_ = _make(form)
    assert float((_steps(m_, l_, o_, _batch(form, 0, 8, weighted=False), 1)[0] - g_ref).abs().max()) > 1e-2 * scale
    for rank, g, p, l in res:
        g, p = torch.from_numpy(g), torch.from_numpy(p)
        tol = 1e-6 + 1e-4 * g_ref.abs() + 6e-5 * scale
        assert ((g - g_ref).abs() <= tol).all(), ('averaged gradients differ', rank, float((g - g_ref).abs().max()), scale)
        assert float((p - p_ref).abs().max()) <= 2e-4, ('parameters differ', rank, float((p - p_ref).abs().max()))
    # the ranks' losses average to the global loss (local numerators over the global denominators)
    assert abs(sum(r[3] for r in res) / world - l_ref) <= 1e-5 + 1e-4 * abs(l_ref)
    assert (res[0][2] == res[1][2]).all(), 'ranks diverged'
    from lirec_amd import config
    config.reset()
