"""Gradient clipping under data parallelism: two ranks (both on cuda:0, gloo, as in tests/test_gpu_parallel.py) each run three
clipped steps on half of a batch, with the sharded update and without.  Every rank gets the coefficient of the AVERAGED global
gradient: the ranks' parameters stay bit-identical, ``grad_norm`` is the same on both and is the single process's on the whole
batch; a RecordedTrainStep with clipping under world > 1 refuses to be built.

``max_grad_norm`` is half of the first step's global norm (GradSync.global_sq_norm after an explicit wait(), the same double on
every rank), so the first step clips; steps 2 and 3 go through step()'s own wait for the reductions.

Measured on an MI355X (two ranks on one GPU, gloo): grad_norm 7.5620 / 7.4387 / 7.3734 and clip_coef 0.5000 / 0.5083 / 0.5128 over
the three steps, the same float32 on both ranks, sharded or not, AND in the single process (relative difference 0 in all three
steps); first-step averaged gradient against the single process's: 4.2e-8 of its largest element; parameters after three steps
within 3.0e-8 of the single process's.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
STEPS = 3
DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)


# (the small model, batch and port helper of tests/test_gpu_parallel.py, copied)
def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make(seed=11, dropout=0.0):
    from lirec_amd import config
    from lirec_amd.config import opt
    config.recipe('int_rel_ch', joint_dim=16, rels_n_clips=3, dropout=dropout, dropout_seed=77, **DIMS)
    opt.device = 'cuda'
    torch.manual_seed(seed)
    from lirec_amd import model as M
    model, loss, optim = M.create_model(11, n_rels=5)
    optim.param_groups[0]['lr'] = 1e-3
    model.train()
    return model, loss, optim


def _batch(lo, hi):
    from lirec_amd.data import synthetic_batch, to_device_batch
    b = synthetic_batch(21, 'int_rel_ch', 8, T=6, R=3, n_classes=11, n_rels=5, **DIMS)
    b = {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in b.items()}
    return to_device_batch(b, 'cuda')


def _clipped_steps(model, loss, optim, batch, bound=None):
    """(max_grad_norm used, [grad_norm], [clip_coef], parameters, first step's averaged gradient)"""
    norms, coefs, g1 = [], [], None
    for i in range(STEPS):
        optim.zero_grad()
        lv = loss(model(dict(batch)), batch)
        lv.backward()
        if i == 0:
            sync = model.grad_sync
            if sync is not None:
                sync.wait()
                sq = float(sync.global_sq_norm(optim.grad_scale))
            else:
                sq = float((model.flat_grads(attach=False).double() ** 2).sum())
            g1 = (model.flat_grads(attach=False).detach().clone() * optim.grad_scale).cpu().numpy()
            optim.max_grad_norm = bound if bound is not None else 0.5 * sq ** 0.5
        optim.step()
        torch.cuda.synchronize()
        norms.append(float(optim.grad_norm)); coefs.append(float(optim.clip_coef))
    return float(optim.max_grad_norm), norms, coefs, model.flat_params().detach().cpu().numpy().copy(), g1


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from lirec_amd._lib import LirecError
        from lirec_amd.graph import RecordedTrainStep
        from lirec_amd.parallel import DataParallel
        per = 8 // world
        out = []
        for sharded in (True, False):
            model, loss, optim = _make(seed=11 + 5 * rank)
            DataParallel(model, optim, sharded=sharded)
            batch = _batch(rank * per, (rank + 1) * per)
            res = _clipped_steps(model, loss, optim, batch)
            refused = False
            try:
                RecordedTrainStep(model, loss, optim, batch, warmup=0)
            except LirecError as e:
                refused = 'clipping' in str(e)
            out.append(res + (refused,))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_clip_like_a_single_process():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for k, sharded in enumerate((True, False)):
        (b0, n0, c0, p0, g0, r0), (b1, n1, c1, p1, g1, r1) = res[0][1][k], res[1][1][k]
        assert r0 and r1, 'a RecordedTrainStep with clipping under world > 1 was built'
        assert b0 == b1 and n0 == n1 and c0 == c1, ('the ranks saw different norms', sharded, (b0, n0, c0), (b1, n1, c1))
        assert (p0 == p1).all(), ('ranks diverged', sharded, int((p0 != p1).sum()))
        assert c0[0] < 1.0, c0
        model, loss, optim = _make(seed=11)
        _, n_ref, c_ref, p_ref, g_ref = _clipped_steps(model, loss, optim, _batch(0, 8), bound=b0)
        rel = [abs(a - b) / b for a, b in zip(n0, n_ref)]
        gdiff = float(np.abs(g0 - g_ref).max()) / float(np.abs(g_ref).max())
        print('CLIP-FIGURE parallel sharded=%s max_grad_norm=%.6g norms=%s single=%s rel=%s coefs=%s single=%s '
              'first-step gradient difference (max abs / max abs)=%.3g parameters max abs diff=%.3g'
              % (sharded, b0, n0, n_ref, ['%.3g' % r for r in rel], c0, c_ref, gdiff, float(np.abs(p0 - p_ref).max())))
        assert max(rel) <= 1e-6, (sharded, rel)
        assert float(np.abs(p0 - p_ref).max()) <= 2e-4, ('parameters differ from the single process', sharded)
