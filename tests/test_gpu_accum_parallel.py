"""Gradient accumulation under data parallelism: two ranks (both on cuda:0, gloo, launched as tests/test_gpu_clip_parallel.py
launches its ranks) take two windows of k = 2 and one more hold step, each on its half of every global micro-batch, with the
sharded update and without, and once with max_grad_norm set.  The collectives a step issues are counted by a wrapper around the
model's GradSync (bucket reductions as they are launched, parameter all-gathers): none on a hold step -- the backward's buckets
stay local, nothing is gathered --, on an apply step what a step of the same optimiser without accumulation issues.  The ranks
stay bit-identical to each other after every micro-step, a hold step changes no parameter bit, and the parameters are the single
process's that steps on the whole micro-batches with the same k, within that file's tolerance (2e-4).  A RecordedTrainStep with
accumulation under world > 1 refuses to be built.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_gpu_clip_parallel as CP

pytestmark = pytest.mark.gpu
K, MICRO = 2, 5
BOUND = 1.0                                  # (max_grad_norm of the clipped run: the averaged gradient's norm is several times that)


class _CountingSync:
    """Stands in for the model's GradSync: everything goes to the real one; bucket reductions are counted where they are
    launched, parameter all-gathers where they are asked for"""

    def __init__(self, real):
        self.__dict__['real'] = real
        self.__dict__['count'] = 0

    def __getattr__(self, name):
        return getattr(self.real, name)

    def __setattr__(self, name, value):          # (FusedAdam sets `hold` on whatever the model's grad_sync is)
        setattr(self.real, name, value)

    def bucket_ready(self, stage, also=None):
        before = len(self.real.pending)
        self.real.bucket_ready(stage, also=also)
        self.__dict__['count'] += len(self.real.pending) - before

    def wait_each(self):
        if self.real.world > 1:
            for s in self.real.stages:
                self.bucket_ready(s)
        return self.real.wait_each()

    def wait(self):
        if self.real.world > 1:
            for s in self.real.stages:
                self.bucket_ready(s)
        return self.real.wait()

    def gather_params(self, lo, hi):
        if self.real.sharded:
            self.__dict__['count'] += 1
        return self.real.gather_params(lo, hi)

    def take(self):
        n, self.__dict__['count'] = self.count, 0
        return n


def _batch(j, lo, hi):
    from lirec_amd.data import synthetic_batch, to_device_batch
    b = synthetic_batch(21 + j, 'int_rel_ch', 8, T=6, R=3, n_classes=11, n_rels=5, **CP.DIMS)
    b = {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in b.items()}
    return to_device_batch(b, 'cuda')


def _steps(model, loss, optim, lo, hi, k, clip, counting=None):
    """MICRO micro-steps with accumulate_steps = k: ([collectives per step], [parameters after each step], [grad_norm at applies])"""
    optim.accumulate_steps = k
    optim.max_grad_norm = clip
    counts, params, norms = [], [], []
    for j in range(MICRO):
        applies = (j + 1) % k == 0
        optim.zero_grad()
        lv = loss(model(dict(_batch(j, lo, hi))), _batch(j, lo, hi))
        lv.backward()
        optim.step()
        torch.cuda.synchronize()
        if counting is not None:
            counts.append(counting.take())
        params.append(model.flat_params().detach().cpu().numpy().copy())
        if clip and applies:
            norms.append(float(optim.grad_norm))
    return counts, params, norms


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
        for sharded, clip in ((True, None), (False, None), (True, BOUND)):
            # what a step without accumulation issues
            model, loss, optim = CP._make(seed=11 + 5 * rank)
            DataParallel(model, optim, sharded=sharded)
            model.grad_sync = counting = _CountingSync(model.grad_sync)
            usual, _, _ = _steps(model, loss, optim, rank * per, (rank + 1) * per, 1, clip, counting)
            # ... and with it
            model, loss, optim = CP._make(seed=11 + 5 * rank)
            DataParallel(model, optim, sharded=sharded)
            model.grad_sync = counting = _CountingSync(model.grad_sync)
            counts, params, norms = _steps(model, loss, optim, rank * per, (rank + 1) * per, K, clip, counting)
            refused = False
            model.grad_sync = counting.real
            try:
                RecordedTrainStep(model, loss, optim, _batch(0, rank * per, (rank + 1) * per), warmup=0)
            except LirecError as e:
                refused = 'accumulation' in str(e)
            out.append((usual, counts, params, norms, refused, optim._step, optim.accum_phase))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_accumulate_like_a_single_process():
    world, port = 2, CP._free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    stuck = [p for p in procs if p.is_alive()]
    for p in stuck:                              # (no rank is left behind with the GPU open)
        p.terminate()
        p.join(timeout=10)
    assert not stuck and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    for i, (sharded, clip) in enumerate(((True, None), (False, None), (True, BOUND))):
        model, loss, optim = CP._make(seed=11)
        _, p_ref, n_ref = _steps(model, loss, optim, 0, 8, K, clip)
        (u0, c0, p0, n0, r0, s0, ph0), (u1, c1, p1, n1, r1, s1, ph1) = res[0][1][i], res[1][1][i]
        assert r0 and r1, 'a RecordedTrainStep with accumulation under world > 1 was built'
        assert (s0, ph0) == (s1, ph1) == (MICRO // K, MICRO % K)
        usual = u0[0]
        assert usual > 0 and u0 == u1 == [usual] * MICRO, (sharded, clip, u0, u1)
        assert c0 == c1 == [usual if (j + 1) % K == 0 else 0 for j in range(MICRO)], (sharded, clip, c0, c1, usual)
        for j in range(MICRO):
            assert (p0[j] == p1[j]).all(), ('ranks diverged', sharded, clip, j + 1, int((p0[j] != p1[j]).sum()))
            if (j + 1) % K:
                before = p0[j - 1] if j else None
                assert before is None or (p0[j] == before).all(), ('a hold step changed parameters', j + 1)
        assert not (p0[1] == p0[0]).all() and not (p0[3] == p0[2]).all()
        diff = float(np.abs(p0[-1] - p_ref[-1]).max())
        print('ACCUM-FIGURE parallel sharded=%s clip=%s collectives per step=%s (without accumulation %d) norms=%s single=%s '
              'parameters max abs diff to the single process=%.3g' % (sharded, clip, c0, usual, n0, n_ref, diff))
        assert np.isfinite(p0[-1]).all() and diff <= 2e-4, ('parameters differ from the single process', sharded, clip, diff)
        if clip:
            assert n0 == n1 and len(n0) == MICRO // K and all(n > clip for n in n0), (n0, n1)
            for a, b in zip(n0, n_ref):
                assert abs(a - b) <= 1e-6 * abs(b), ('the ranks\' norm is not the single process\'s', n0, n_ref)      # (that file's criterion)
