"""``opt.param_stats_every`` and the Python refusals of ``FusedAdam.param_stats()`` through the real Python host stack in the
library's host-side DRY RUN (tests/host_dryrun.py) -- the driver of tests/test_host_param_stats.py, run in a process of its own (the
dry run patches torch and switches the library process-wide); not a test module.  What is looked at is what the host ISSUES: the
``ops.param_stats`` calls of a short ``training()``, and the lines it prints.  Nothing is computed in a dry run: the printed numbers are
whatever the untouched host buffers hold."""
import sys
import tempfile

import host_dryrun as H

import torch  # noqa: E402

from lirec_amd import _lib, config, ops, train  # noqa: E402
from lirec_amd import model as M  # noqa: E402
from lirec_amd._lib import LirecError  # noqa: E402
from lirec_amd.config import opt  # noqa: E402
from lirec_amd.data import SyntheticMixedFeaturesDataset  # noqa: E402

DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)
CALLS, LINES = [], []


def spy():
    fn = ops.param_stats

    def wrapped(p, g, m, v, entries, out, ws):
        CALLS.append([tuple(e) for e in entries])
        out.zero_()                                  # (no launch writes it here: host() would read uninitialised memory)
        return fn(p, g, m, v, entries, out, ws)
    ops.param_stats = wrapped
    train._print = lambda *a, **k: LINES.append(' '.join(str(x) for x in a))
    train._evaluate_and_keep = lambda *a, **k: None        # (the evaluation behind epoch 0 divides by counts nothing has counted)
    # (the loop marks each loss value with an event on the stream: host tensors pass for device tensors here)
    torch.cuda.Event = type('Event', (), {'record': lambda self, *a: None, 'synchronize': lambda self: None, 'query': lambda self: True})


def make(tmp, epochs, **flags):
    config.reset()
    config.recipe('int_rel_ch', joint_dim=16, batch_size=4, num_workers=0, epochs=epochs, test_fr=1000, store_root=tmp, rels_n_clips=3,
                  dropout=0.3, dropout_seed=5, save_model=False, **DIMS)
    opt.device = 'cpu'
    opt.wgrad_side_stream = False
    for k, v in flags.items():
        setattr(opt, k, v)
    kw = dict(T=6, R=3, n_classes=11, n_rels=5, n_mgd=11, soft_gt=opt.soft_gt, **DIMS)
    model, loss, optim = M.create_model(11, n_rels=5)
    return SyntheticMixedFeaturesDataset('int_rel_ch', 9, seed=1, **kw), model, loss, optim


def wiring():
    """0 (the default) issues no lirec_param_stats call over a short training(); 1 exactly one per epoch, 2 one every second epoch --
    each ONE call over all the parameters, a line per parameter printed; with a ``grad_sync`` of world 2 (a stub) both calls raise
    LirecError and issue nothing"""
    with tempfile.TemporaryDirectory() as tmp:
        assert config.defaults()['param_stats_every'] == 0
        for every, epochs, want in ((0, 2, 0), (1, 2, 2), (2, 3, 1)):
            ds, model, loss, optim = make(tmp, epochs, param_stats_every=every)
            del CALLS[:], LINES[:]
            train.training(ds, model=model, loss=loss, optimizer=optim)
            names = [n for n, _ in model.named_parameters()]
            assert len(CALLS) == want, (every, len(CALLS))
            heads = [i for i, l in enumerate(LINES) if l.startswith('parameter statistics')]
            assert len(heads) == want, (every, LINES)
            for c, at in zip(CALLS, heads):
                assert [(e[0], e[1]) for e in c] == [tuple(model._offsets[n]) for n in names]
                assert all(e[2] == 7 for e in c), 'every parameter trains and has been updated'
                assert [l.split()[0] for l in LINES[at + 1:at + 1 + len(names)]] == names
        # data parallelism: refused
        ds, model, loss, optim = make(tmp, 1, param_stats_every=1)
        model.grad_sync = type('Sync', (), {'world': 2})()
        del CALLS[:], LINES[:]
        try:
            optim.param_stats()
            raise AssertionError('param_stats() under data parallelism was not refused')
        except LirecError as e:
            assert 'data parallelism' in str(e) and 'collectives' in str(e)
        for call in (optim.nonfinite_params,):
            try:
                call()
                raise AssertionError('nonfinite_params() under data parallelism was not refused')
            except LirecError:
                pass
        assert not CALLS
    print('wiring ok')


def refusals():
    """while a step is being recorded: RuntimeError, nothing issued; outside: one call, update=False asks for no update column"""
    with tempfile.TemporaryDirectory() as tmp:
        ds, model, loss, optim = make(tmp, 1)
        ops.CommandList.begin()
        try:
            for call in (optim.param_stats, optim.nonfinite_params):
                try:
                    call()
                    raise AssertionError('%s while recording was not refused' % call.__name__)
                except RuntimeError as e:
                    assert 'recorded' in str(e)
        finally:
            ops.CommandList.end().destroy()
        assert not CALLS
        st = optim.param_stats()                     # before any step: no update column
        assert len(CALLS) == 1 and all(e[2] == 3 for e in CALLS[0]) and st.names == [n for n, _ in model.named_parameters()]
        assert tuple(st.table.shape) == (len(st.names), 9) and st.table.dtype == torch.float64
        next(iter(model.parameters())).requires_grad_(False)
        optim.param_stats(update=False)
        assert [e[2] for e in CALLS[1]] == [2] + [3] * (len(st.names) - 1)
    print('refusals ok')


def main(what):
    L = _lib.lib()
    assert L.lirec_debug_set(H.DRY, -1) == 0
    H.patch()
    spy()
    ops.set_gemm_mode(2)
    {'wiring': wiring, 'refusals': refusals}[what]()
    config.reset()
    assert L.lirec_debug_set(0, -1) == 0


if __name__ == '__main__':
    main(sys.argv[1])
