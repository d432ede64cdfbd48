"""Input-feature gradients under data parallelism: two ranks (both on cuda:0, gloo -- as tests/test_gpu_parallel.py) each run the
real kernels on half of a batch whose features require grad.

Nothing reduces dX: each rank's ``features.grad`` is the gradient of ITS loss with respect to ITS rows.  That loss is the rank's
numerators over (the global batch's denominators / world) -- the form whose parameter gradients AVERAGE to the global batch's:

  * MarginTrackRelsLoss (recipe int_rel_ch): a plain mean over the rank's B / world clips;
  * MultiTaskMaxMargin (recipe int_rels) attached to the DataParallel (``loss=loss``): the interaction term over clips / world, the
    relationship term over the all-reduced count of labelled clips / world (model.py ``_DPMeans``, parallel.py
    ``global_divisors``) -- here with the labelled clips spread unequally over the ranks (4 and 1).

Either way rank r's dX = c x (the single process's dX of the whole batch, on r's rows) with c = world -- C_FACTOR below, one entry
per loss.  Held with the tolerance tests/test_gpu_input_grad.py holds dX to its reference with (golden_util.grad_close, defaults).
Dropout is off: a row's Philox mask is keyed by its index in the LOCAL batch, so with dropout on the two runs are different draws.
And, as test_gpu_input_grad.py::test_step_unchanged_by_requires_grad for one process: the averaged parameter gradients and the
step are bit for bit the same with and without ``requires_grad`` on the features, on both ranks.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from golden_util import grad_close
from test_gpu_parallel import _batch, _free_port, _make, _rels_batch, _rels_make

pytestmark = pytest.mark.gpu

WORLD, CLIPS = 2, 8
# d (rank's loss) / d (its rows) = C_FACTOR x d (global loss) / d (those rows)
C_FACTOR = {'MarginTrackRelsLoss': lambda world: world, 'MultiTaskMaxMargin': lambda world: world}


def _setup(name):
    if name == 'MarginTrackRelsLoss':
        return _make(seed=11, dropout=0.0), _batch
    return _rels_make(False, seed=11, dropout=0.0), (lambda lo, hi: _rels_batch(lo, hi, False))


def _one_step(name, lo, hi, requires_grad, parallel):
    """a fresh model, one step on clips [lo, hi): (dX or None, averaged flat gradients, parameters after the step)"""
    (model, loss, optim), batch_of = _setup(name)
    assert type(loss).__name__ == name
    if parallel:
        from lirec_amd.parallel import DataParallel
        DataParallel(model, optim, loss=loss)
    batch = batch_of(lo, hi)
    f = batch['features']
    if requires_grad:
        f.requires_grad_(True)
    optim.zero_grad()
    lv = loss(model(dict(batch)), batch)
    lv.sum().backward()
    if model.grad_sync is not None:
        model.grad_sync.wait()
    g = (model.flat_grads(attach=False).detach().clone() * optim.grad_scale).cpu()
    dx = f.grad.detach().cpu().clone() if requires_grad else None
    assert requires_grad or f.grad is None
    optim.step()
    torch.cuda.synchronize()
    return dx, g, model.flat_params().detach().cpu().clone()


def _worker(rank, world, port, name, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        per = CLIPS // world
        _, g0, p0 = _one_step(name, rank * per, (rank + 1) * per, False, True)
        dx, g1, p1 = _one_step(name, rank * per, (rank + 1) * per, True, True)
        q.put((rank, dx.numpy(), bool(torch.equal(g0, g1)), bool(torch.equal(p0, p1)), g1.numpy()))
    except BaseException as e:                     # the assertion text travels back to the test
        import traceback
        q.put((rank, 'FAILED: %s\n%s' % (e, traceback.format_exc())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('name', sorted(C_FACTOR))
def test_two_rank_input_grad_is_c_times_the_single_process_gradient_on_the_ranks_rows(name):
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, name, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(WORLD)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in res:
        assert len(r) == 5, r[1]
    dx_ref, g_ref, _ = _one_step(name, 0, CLIPS, True, False)
    assert float(dx_ref.abs().max()) > 0
    c, per = C_FACTOR[name](WORLD), CLIPS // WORLD
    for rank, dx, same_grads, same_params, g in res:
        dx = torch.from_numpy(dx)
        want = c * dx_ref[rank * per:(rank + 1) * per]
        assert dx.shape == want.shape and float(want.abs().max()) > 0
        grad_close(dx, want, '%s rank %d dX vs %d x single-process dX' % (name, rank, c))
        # (the factor is not a formality: without it the same comparison fails)
        assert float((dx - want / c).abs().max()) > 0.25 * float(want.abs().max())
        assert same_grads, 'rank %d: requires_grad on the features changed the averaged parameter gradients' % rank
        assert same_params, 'rank %d: requires_grad on the features changed the step' % rank
        # ... and these are the gradients the ranks are meant to have: the single process's on the whole batch
        g = torch.from_numpy(g)
        tol = 1e-6 + 1e-4 * g_ref.abs() + 6e-5 * float(g_ref.abs().max())
        assert ((g - g_ref).abs() <= tol).all(), ('averaged gradients differ', rank, float((g - g_ref).abs().max()))
