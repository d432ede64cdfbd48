"""The weight average under the sharded data-parallel update: two ranks (both on cuda:0, gloo, as in tests/test_gpu_parallel.py)
each run three steps on half of a batch with FusedAdam(ema_decay=0.9) -- plain, and guarded + clipped (the route that lands every
reduction first, ``_step_parallel_clipped``).  A rank lerps its own slices only; after ``consolidate_state()`` each rank's shadow

  * is, bit for bit, the chain of CPU lerps over that rank's own parameter snapshots (the parameters are whole on every rank
    after each step's gather), and the same bits on both ranks;
  * equals the single process's shadow on the whole batch within 2e-4, the tolerance this directory holds the two-rank PARAMETERS
    to against the single process (tests/test_gpu_parallel.py; the averaged gradient is summed in another order): a shadow is a
    convex combination of parameter snapshots, each within that tolerance, so it is within it too.

Before the gather the shadow outside a rank's slices is stale (it still holds the start values there) and ``ema_state_dict()`` warns.
"""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_gpu_clip_parallel as CP

pytestmark = pytest.mark.gpu
STEPS = 3
DECAY = 0.9
VARIANTS = ['plain', 'guarded_clipped']


def _steps(model, loss, optim, batch, variant, consolidate):
    """(shadow at the start, [parameters after each step], shadow at the end, shadow before consolidate_state(), warned?)"""
    optim.ema_decay = DECAY
    if variant == 'guarded_clipped':
        optim.skip_nonfinite = True
        optim.max_grad_norm = 1.0
    params, start = [], None
    for i in range(STEPS):
        optim.zero_grad()
        lv = loss(model(dict(batch)), batch)
        lv.backward()
        if start is None:
            optim._ensure_state()
            torch.cuda.synchronize()
            start = optim.ema.cpu()
        optim.step()
        torch.cuda.synchronize()
        params.append(model.flat_params().detach().cpu())
    raw = optim.ema.cpu()
    warned = False
    if consolidate:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            optim.ema_state_dict()
            warned = any('stale' in str(w.message) for w in seen)
        optim.consolidate_state()
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            optim.ema_state_dict()
            warned = warned and not any('stale' in str(w.message) for w in seen)
    return start, params, optim.ema.cpu(), raw, warned, optim.ema_updates()


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from lirec_amd.parallel import DataParallel
        per = 8 // world
        out = []
        for variant in VARIANTS:
            model, loss, optim = CP._make(seed=11 + 5 * rank)
            DataParallel(model, optim, sharded=True)
            batch = CP._batch(rank * per, (rank + 1) * per)
            res = _steps(model, loss, optim, batch, variant, consolidate=True)
            mine = [model.grad_sync.my_slice(lo, hi) for lo, hi in model.grad_sync.ranges]
            out.append(tuple(x.numpy() if torch.is_tensor(x) else ([p.numpy() for p in x] if isinstance(x, list) else x) for x in res) + (mine,))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_keep_the_single_process_average():
    from lirec_amd import ops
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
    w = ops.ema_weight(DECAY)
    for k, variant in enumerate(VARIANTS):
        model, loss, optim = CP._make(seed=11)
        _, _, e_ref, _, _, n_ref = _steps(model, loss, optim, CP._batch(0, 8), variant, consolidate=False)
        assert n_ref == STEPS
        shadows = []
        for rank in range(world):
            start, params, shadow, raw, warned, updates, mine = res[rank][1][k]
            assert warned, 'ema_state_dict() did not warn about a stale shadow before consolidate_state() (or still did after)'
            assert updates == STEPS
            chain = torch.from_numpy(start)
            for p in params:
                chain = torch.lerp(chain, torch.from_numpy(p), w)
            got = torch.from_numpy(shadow)
            diff = int((got.view(torch.int32) != chain.view(torch.int32)).sum())
            assert diff == 0, (variant, rank, 'shadow elements off the lerp chain of the rank\'s parameters', diff)
            # before the gather: current on the rank's own slices, the start values everywhere else
            own = torch.zeros(got.numel(), dtype=torch.bool)
            for a, b in mine:
                own[a:b] = True
            rawt = torch.from_numpy(raw)
            assert torch.equal(rawt[own].view(torch.int32), chain[own].view(torch.int32))
            assert torch.equal(rawt[~own].view(torch.int32), torch.from_numpy(start)[~own].view(torch.int32))
            assert bool(own.any()) and bool((~own).any())
            shadows.append(got)
            d = float((got - e_ref).abs().max())
            print('EMA-FIGURE parallel variant=%s rank=%d shadow max abs diff to the single process=%.3g' % (variant, rank, d))
            assert np.isfinite(shadow).all() and d <= 2e-4, (variant, rank, d)
        assert torch.equal(shadows[0].view(torch.int32), shadows[1].view(torch.int32)), (variant, 'the ranks\' shadows differ')
        assert not torch.equal(shadows[0], torch.from_numpy(res[0][1][k][0])), 'the shadow never moved'
