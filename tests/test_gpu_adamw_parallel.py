"""Decoupled weight decay under data parallelism: two ranks (both on cuda:0, gloo, the pattern of
tests/test_gpu_groups_parallel.py) each run three steps on half of a batch with the SHARDED update and the two groups of
tests/adamw_cases.py -- the weights decoupled at 1e-2, the biases at 0: a rank's slice of a bucket is intersected with the grouped
ranges, and the first bucket is updated on the collectives' early stream from that stream's own table, flag included.  The ranks
stay bit-identical; against one process on the whole batch: the margin that file uses (parameters within 2e-4).  Two GPU
processes, every wait under its own time limit."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import adamw_cases as WC
import group_cases as GC
import test_gpu_groups_parallel as TGP

pytestmark = pytest.mark.gpu


def _make(seed=11, decoupled=True):
    from lirec_amd import config
    from lirec_amd.config import opt
    from lirec_amd.optim import FusedAdam
    config.recipe('int_rel_ch', joint_dim=GC.JOINT, rels_n_clips=GC.R, dropout=0.0, dropout_seed=77, **GC.DIMS)
    opt.device = 'cuda'
    torch.manual_seed(seed)
    from lirec_amd import model as M
    model, loss, _ = M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)
    groups = WC.two_groups(model)
    groups[0]['decoupled_weight_decay'] = decoupled
    optim = FusedAdam(model, lr=WC.LR, param_groups=groups)
    model.train()
    return model, loss, optim


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from lirec_amd.parallel import DataParallel
        per = 8 // world
        model, loss, optim = _make(seed=11 + 5 * rank)
        DataParallel(model, optim, sharded=True)
        q.put((rank, TGP._steps(model, loss, optim, TGP._batch(rank * per, (rank + 1) * per))))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_decoupled_decay_and_the_sharded_update():
    world, port = 2, TGP._free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    (p0, m0, v0, roles0), (p1, m1, v1, roles1) = res[0][1], res[1][1]
    for a, b, what in ((p0, p1, 'parameters'), (m0, m1, 'exp_avg'), (v0, v1, 'exp_avg_sq')):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ('ranks diverged', what, int((a != b).sum()))
    assert roles0 == roles1 == ['early', 'main'], (roles0, roles1)
    p_ref = TGP._steps(*_make(seed=11), TGP._batch(0, 8))[0]
    p_coupled = TGP._steps(*_make(seed=11, decoupled=False), TGP._batch(0, 8))[0]
    diff, other = float(np.abs(p0 - p_ref).max()), float(np.abs(p0 - p_coupled).max())
    print('ADAMW-FIGURE parallel issuing streams=%s parameters max abs diff to the single process=%.3g (the same groups coupled: %.3g)'
          % (roles0, diff, other))
    assert diff <= 2e-4, 'parameters differ from the single process'
    # the flag reached the sharded update: coupled, the decay of 1e-2 goes through Adam's normaliser and the weights end elsewhere
    assert other > 10 * diff
