"""Skipping non-finite steps under data parallelism: two ranks (both on cuda:0, gloo, as in tests/test_gpu_clip_parallel.py) each
run three guarded steps on half of a batch, with the sharded update and without.  During step 2 one feature element of RANK 0's
half is NaN: only rank 0's local gradient is non-finite, the reduced one is everywhere -- under the sharded update in every
rank's slices of it, whose squares the one all-reduced double adds up.  Both ranks skip (the same flag and count with no further
collective), their parameters stay bit-identical, and they are the single process's that runs the whole batch with the same
element poisoned and skips the same step, within that file's tolerance (2e-4).  A RecordedTrainStep with the guard under
world > 1 refuses to be built.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_gpu_clip_parallel as CP

pytestmark = pytest.mark.gpu
STEPS = 3


def _spot(batch):
    """a feature element of a candidate of clip 0 that is part of the clip"""
    t = int(torch.nonzero(batch['mem_mask'][0].reshape(-1) == 1)[0])
    f = batch['features']
    return f.reshape(f.shape[0], -1, f.shape[-2], f.shape[-1])[0, t, 0, 40:41]


def _guarded_steps(model, loss, optim, batch, poison):
    """([found_nonfinite], [skipped_steps], [parameters after each step])"""
    optim.skip_nonfinite = True
    spot = _spot(batch) if poison else None
    keep = spot.clone() if poison else None
    found, skipped, params = [], [], []
    for i in range(STEPS):
        if poison:
            spot.fill_(float('nan')) if i == 1 else spot.copy_(keep)
        optim.zero_grad()
        lv = loss(model(dict(batch)), batch)
        lv.backward()
        optim.step()
        torch.cuda.synchronize()
        found.append(float(optim.found_nonfinite)); skipped.append(int(optim.skipped_steps))
        params.append(model.flat_params().detach().cpu().numpy().copy())
    return found, skipped, params


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
            model, loss, optim = CP._make(seed=11 + 5 * rank)
            DataParallel(model, optim, sharded=sharded)
            batch = CP._batch(rank * per, (rank + 1) * per)
            res = _guarded_steps(model, loss, optim, batch, poison=rank == 0)
            refused = False
            try:
                RecordedTrainStep(model, loss, optim, batch, warmup=0)
            except LirecError as e:
                refused = 'skip_nonfinite' in str(e)
            out.append(res + (refused,))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_skip_like_a_single_process():
    world, port = 2, CP._free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    model, loss, optim = CP._make(seed=11)
    f_ref, s_ref, p_ref = _guarded_steps(model, loss, optim, CP._batch(0, 8), poison=True)
    assert f_ref == [0.0, 1.0, 0.0] and s_ref == [0, 1, 1]
    assert (p_ref[0] == p_ref[1]).all() and not (p_ref[1] == p_ref[2]).all()
    for k, sharded in enumerate((True, False)):
        (f0, s0, p0, r0), (f1, s1, p1, r1) = res[0][1][k], res[1][1][k]
        assert r0 and r1, 'a RecordedTrainStep with the guard under world > 1 was built'
        assert f0 == f1 == [0.0, 1.0, 0.0] and s0 == s1 == [0, 1, 1], (sharded, f0, f1, s0, s1)
        for i in range(STEPS):
            assert (p0[i] == p1[i]).all(), ('ranks diverged', sharded, i + 1, int((p0[i] != p1[i]).sum()))
        assert (p0[0] == p0[1]).all(), 'the skipped step changed parameters'
        diff = float(np.abs(p0[2] - p_ref[2]).max())
        print('GUARD-FIGURE parallel sharded=%s found=%s skipped=%s parameters max abs diff to the single process=%.3g' % (sharded, f0, s0, diff))
        assert np.isfinite(p0[2]).all() and diff <= 2e-4, ('parameters differ from the single process', sharded, diff)
