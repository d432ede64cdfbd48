"""Parameter groups under data parallelism: two ranks (both on cuda:0, gloo, as in tests/test_gpu_parallel.py) each run three
steps on half of a batch with the SHARDED update and the three groups of tests/group_cases.py: a rank's slice of a bucket is
intersected with the grouped ranges, and the first bucket is updated on the collectives' early stream from that stream's own
hyper-parameter table.  The ranks stay bit-identical; against one process on the whole batch: the comparison and the tolerance
tests/test_gpu_clip_parallel.py uses for the same pair of runs (parameters within 2e-4).  Under opt.strict the groups' membership
is part of the hash the ranks compare: a rank with other groups is told.  Two GPU processes."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import group_cases as GC

pytestmark = pytest.mark.gpu
STEPS = 3


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make(seed=11):
    from lirec_amd import config
    from lirec_amd.config import opt
    from lirec_amd.optim import FusedAdam
    config.recipe('int_rel_ch', joint_dim=GC.JOINT, rels_n_clips=GC.R, dropout=0.0, dropout_seed=77, **GC.DIMS)
    opt.device = 'cuda'
    torch.manual_seed(seed)
    from lirec_amd import model as M
    model, loss, _ = M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)
    groups = GC.three_groups(model)
    optim = FusedAdam(model, lr=1e-3, weight_decay=1e-5, param_groups=groups)
    model.train()
    return model, loss, optim


def _batch(lo, hi):
    from lirec_amd.data import synthetic_batch, to_device_batch
    b = synthetic_batch(21, 'int_rel_ch', 8, T=GC.T, R=GC.R, n_classes=GC.N_CLASSES, n_rels=GC.N_RELS, **GC.DIMS)
    b = {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in b.items()}
    return to_device_batch(b, 'cuda')


def _steps(model, loss, optim, batch):
    roles = set()
    for i in range(STEPS):
        optim.zero_grad()
        lv = loss(model(dict(batch)), batch)
        lv.backward()
        optim.step()
        torch.cuda.synchronize()
        roles |= {r for r, t in optim._tables.items() if t[1] is not None}
    if getattr(model, 'grad_sync', None) is not None:
        optim.consolidate_state()
    torch.cuda.synchronize()
    f = lambda t: t.detach().cpu().numpy().copy()
    return f(model.flat_params()), f(optim._m), f(optim._v), sorted(roles)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from lirec_amd.parallel import DataParallel
        per = 8 // world
        model, loss, optim = _make(seed=11 + 5 * rank)
        DataParallel(model, optim, sharded=True)
        # the check opt.strict makes in step(): the same membership on every rank passes, one that differs on one rank is refused on all
        flags, mem = optim._flags(), optim.group_membership()
        model.grad_sync.check_frozen_set(flags, mem)
        told = []
        try:
            model.grad_sync._frozen_checked = None
            model.grad_sync.check_frozen_set(flags, mem)          # (the same membership passes)
            told.append(False)
        except RuntimeError:
            told.append(True)
        model.grad_sync._frozen_checked = None          # (checked once per set: make both ranks check again)
        try:
            model.grad_sync.check_frozen_set(flags, mem[:-1] + ((mem[-1] + rank) % 3,))
            told.append(False)
        except RuntimeError as e:
            told.append('parameter groups' in str(e))
        res = _steps(model, loss, optim, _batch(rank * per, (rank + 1) * per))
        q.put((rank, res, told))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_three_groups_and_the_sharded_update():
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
    (p0, m0, v0, roles0), (p1, m1, v1, roles1) = res[0][1], res[1][1]
    for a, b, what in ((p0, p1, 'parameters'), (m0, m1, 'exp_avg'), (v0, v1, 'exp_avg_sq')):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ('ranks diverged', what, int((a != b).sum()))
    # the first bucket was updated on the collectives' early stream from that stream's own table; no side-stream table under
    # data parallelism (nothing is updated there)
    assert roles0 == roles1 == ['early', 'main'], (roles0, roles1)
    assert res[0][2] == [False, True] and res[1][2] == [False, True], (res[0][2], res[1][2])
    model, loss, optim = _make(seed=11)
    p_ref, m_ref, v_ref, _ = _steps(model, loss, optim, _batch(0, 8))
    one = _make(seed=11)
    one_group = type(optim)(one[0], lr=1e-3, weight_decay=1e-5)
    p_one = _steps(one[0], one[1], one_group, _batch(0, 8))[0]
    diff = float(np.abs(p0 - p_ref).max())
    print('GROUP-FIGURE parallel issuing streams=%s parameters max abs diff to the single process=%.3g (one group instead: %.3g)'
          % (roles0, diff, float(np.abs(p0 - p_one).max())))
    assert diff <= 2e-4, 'parameters differ from the single process'
    # the groups reached the sharded update: the embeddings' weights (lr 1e-5) moved a hundredth of what one group at 1e-3 moves them
    assert float(np.abs(p0 - p_one).max()) > 10 * diff
