"""training(resume=...) on the host: the train state's round trip and refusals, the order a resumed epoch draws its batches in
(and that no sample of a batch passed over is fetched), the ModelSaver's state, the atomic rolling file, the unchanged default
key set, and -- with the stand-in model of test_parallel_cpu -- whole runs cut at an epoch boundary and inside an epoch, in one
process and on two gloo ranks.  Equality is bit equality throughout."""
import os
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from lirec_amd import config
from lirec_amd.config import opt
from lirec_amd.loader import ThreadedLoader
from lirec_amd.util import ModelSaver, load_train_state, save_checkpoint

from test_parallel_cpu import _AveragingSGD, _StandIn, _free_port, _train_setup


def _state(tmp_path, n=22, **over):
    from lirec_amd.train import TrainState
    from lirec_amd.util import Averaging
    mk, model, loss, optim = _train_setup(str(tmp_path))
    ds = mk(n, 1)
    losses = Averaging()
    losses.update(0.25, 4)
    kw = dict(epoch=1, batches_done=2, steps_taken=7, seen=8, losses=losses, epoch_rng=torch.get_rng_state(), start='20240101-000000')
    kw.update(over)
    return TrainState.capture(ds, model, loss, optim, None, ModelSaver(path=str(tmp_path)), **kw), ds, model, loss, optim


def test_train_state_round_trip_and_refusals(tmp_path):
    from lirec_amd.train import TrainState
    st, ds, model, loss, optim = _state(tmp_path)
    path = str(tmp_path / 'ck.pth.tar')
    save_checkpoint(path, 0, model, optim, train_state=st.as_dict())
    ck, ts = load_train_state(path)
    assert set(ck) == {'epoch', 'state_dict', 'optimizer', 'train_state'}
    back = TrainState.from_dict(ts)
    assert (back.version, back.epoch, back.batches_done, back.steps_taken, back.seen) == (1, 1, 2, 7, 8)
    assert (back.loss_sum, back.loss_count, back.start) == (1.0, 4, '20240101-000000')
    assert back.fingerprint == st.fingerprint and back.saver == st.saver and back.scheduler is None
    assert torch.equal(back.rng['torch'], st.rng['torch']) and torch.equal(back.epoch_rng, st.epoch_rng)
    assert back.rng['python'] == st.rng['python']
    assert all(np.array_equal(a, b) for a, b in zip(back.rng['numpy'], st.rng['numpy']))
    back.check(ds, model, optim)                                    # (the same run: nothing to name)
    assert load_train_state(ck)[1] is ck['train_state']             # (an already loaded dict)
    # refused in words: a plain checkpoint, an unknown version
    plain = str(tmp_path / 'plain.pth.tar')
    save_checkpoint(plain, 0, model, optim)
    with pytest.raises(ValueError, match='holds no train state'):
        load_train_state(plain)
    with pytest.raises(ValueError, match='version 2'):
        TrainState.from_dict(dict(ts, version=2))


class _Longer(torch.utils.data.Dataset):
    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds) + 1


@pytest.mark.parametrize('field', ['batch_size', 'dropout', 'dropout_seed', 'accumulate_steps', 'opt.margin', 'opt.tr_cat_distr',
                                   'optimizer', 'len(train_dataset)', 'parameter names'])
def test_each_fingerprint_field_is_named(field, tmp_path):
    st, ds, model, loss, optim = _state(tmp_path)
    if field == 'batch_size':
        opt.batch_size += 1
    elif field == 'dropout':
        opt.dropout = 0.5
    elif field == 'dropout_seed':
        opt.dropout_seed += 1
    elif field == 'accumulate_steps':
        optim.accumulate_steps = 2
    elif field == 'opt.margin':
        opt.margin = 0.2
    elif field == 'opt.tr_cat_distr':
        opt.tr_cat_distr = not opt.tr_cat_distr
    elif field == 'optimizer':
        optim.param_groups[0]['weight_decay'] = 0.5
    elif field == 'len(train_dataset)':
        ds = _Longer(ds)
    else:
        model.extra = torch.nn.Parameter(torch.zeros(1))
    with pytest.raises(ValueError) as e:
        st.check(ds, model, optim)
    assert str(e.value).startswith('training(resume=): %s differs' % field), str(e.value)


def test_loop_fields_are_not_in_the_fingerprint(tmp_path):
    """what the two halves may differ in: the number of epochs, where the files go, how often a checkpoint is written"""
    st, ds, model, loss, optim = _state(tmp_path)
    opt.set(epochs=99, store_root='/elsewhere', checkpoint_every=3, save_train_state=True, test_fr=5, num_workers=2,
            resume_str='x', resume_train=True, tr_sum_max_flag=not opt.tr_sum_max_flag)
    optim.param_groups[0]['lr'] = 0.5                # (the scheduler moves it; the checkpoint's is loaded)
    st.check(ds, model, optim)


class _Counting(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n, self.fetched, self.lock = n, [], threading.Lock()

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        with self.lock:
            self.fetched.append(int(i))
        return torch.tensor(int(i))


@pytest.mark.parametrize('kind', ['threaded-0', 'threaded-2', 'stock'])
def test_resumed_epoch_draws_the_uncut_order_and_fetches_nothing_skipped(kind):
    from lirec_amd.train import _iter_from
    n, bs, done = 23, 4, 2

    def loader(ds):
        if kind == 'stock':
            return torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=True, num_workers=0)
        return ThreadedLoader(ds, batch_size=bs, shuffle=True, num_workers=int(kind[-1]))
    # the uncut run: three epochs, something else drawing from the RNG between the batches
    torch.manual_seed(5)
    ld, epochs = loader(_Counting(n)), []
    for ep in range(3):
        if ep == 1:
            epoch_rng = torch.get_rng_state()
        out = []
        for i, b in enumerate(iter(ld)):
            if ep == 1 and i == done:
                cut_rng = torch.get_rng_state()
            out.append(b.tolist())
            torch.rand(3)
        epochs.append(out)
    assert sorted(sum(epochs[1], [])) == list(range(n)) and epochs[0] != epochs[1] != epochs[2]
    # the run cut in epoch 1 after `done` batches, continued by a fresh loader
    torch.manual_seed(1234)
    ds = _Counting(n)
    ld = loader(ds)
    torch.set_rng_state(epoch_rng)
    it = _iter_from(ld, done)
    torch.set_rng_state(cut_rng)
    rest = []
    for b in it:
        rest.append(b.tolist())
        torch.rand(3)
    later = []
    for b in iter(ld):
        later.append(b.tolist())
        torch.rand(3)
    assert rest == epochs[1][done:]
    assert later == epochs[2]
    assert sorted(ds.fetched) == sorted(sum(rest, []) + sum(later, []))       # (no sample of a skipped batch)
    assert len(ld) == len(epochs[0])


def test_model_saver_state_gives_the_same_verdicts_and_evictions(tmp_path):
    seq = [{'a': 0.5, 'b': 0.1}, {'a': 0.5, 'b': 0.3}, {'a': 0.2, 'b': 0.3}, {'a': 0.5, 'b': 0.0},        # ties in both metrics
           {'a': 0.5, 'b': 0.3}, {'a': 0.1, 'b': 0.0}, {'a': 0.6, 'b': 0.3}, {'a': 0.5, 'b': 0.3}, {'a': 0.7, 'b': 0.4}]

    def feed(s, vals, at, log):
        for ep, v in enumerate(vals, at):
            keep = s.check(v)
            if keep:
                s.update(v, {'epoch': ep}, ep)
            log.append((keep, {k: dict(d) for k, d in s.eval.items()}))
    one, log1 = ModelSaver(n=2, path=str(tmp_path / 'one')), []
    feed(one, seq, 0, log1)
    for cut in (3, 5):
        first, log2 = ModelSaver(n=2, path=str(tmp_path / ('first%d' % cut))), []
        feed(first, seq[:cut], 0, log2)
        first.save()
        sd = torch.load(_saved(tmp_path, first.state_dict()), weights_only=False)
        second = ModelSaver(n=4, path=str(tmp_path / ('first%d' % cut)))
        second.load_state_dict(sd)
        assert second.n == 2 and second.saved == first.saved
        feed(second, seq[cut:], cut, log2)
        assert log2 == log1
        assert [list(d.items()) for d in second.eval.values()] == [list(d.items()) for d in one.eval.values()]      # (the order ties go by)
        second.save()             # (entries kept from before the cut are in their files; the new ones are written)
        for key, d in second.eval.items():
            assert sorted(os.listdir(os.path.join(second.path, key))) == sorted('v%.4f_ep%d.pth.tar' % (v, ep) for ep, v in d.items())


def _saved(tmp_path, sd):
    p = str(tmp_path / 'saver_state.pt')
    torch.save(sd, p)
    return p


def test_rolling_file_survives_an_interrupted_write(tmp_path, monkeypatch):
    mk, model, loss, optim = _train_setup(str(tmp_path))
    path = str(tmp_path / 'last.pth.tar')
    save_checkpoint(path, 3, model, optim, train_state={'version': 1, 'epoch': 4}, atomic=True)
    before = open(path, 'rb').read()
    real = torch.save

    def torn(obj, f, *a, **k):
        with open(f, 'wb') as out:
            out.write(b'half a checkpoint')
        raise OSError('interrupted')
    monkeypatch.setattr(torch, 'save', torn)
    with pytest.raises(OSError, match='interrupted'):
        save_checkpoint(path, 5, model, optim, train_state={'version': 1, 'epoch': 6}, atomic=True)
    monkeypatch.setattr(torch, 'save', real)
    assert open(path, 'rb').read() == before
    ck, ts = load_train_state(path)
    assert ck['epoch'] == 3 and ts['epoch'] == 4
    assert os.listdir(str(tmp_path)) == ['last.pth.tar']           # (no temporary file left behind)


def test_default_key_set_is_unchanged(tmp_path):
    mk, model, loss, optim = _train_setup(str(tmp_path))
    path = str(tmp_path / 'plain.pth.tar')
    save_checkpoint(path, 0, model, optim)
    assert set(torch.load(path, weights_only=False)) == {'epoch', 'state_dict', 'optimizer'}
    assert opt.save_train_state is False and opt.checkpoint_every == 0 and opt.resume_train is False


# ---------------------------------------------------------------------------
# whole runs with the stand-in model (float64 parameters, stock SGD, the stock DataLoader)
# ---------------------------------------------------------------------------

class _Cut(Exception):
    pass


def _cut_after(monkeypatch, n):
    """the interruption: an exception out of the n-th ``_Stepper.step`` call, after that step was taken"""
    from lirec_amd import train as T
    real, calls = T._Stepper.step, [0]

    def step(self, i, batch):
        out = real(self, i, batch)
        calls[0] += 1
        if calls[0] == n:
            raise _Cut()
        return out
    monkeypatch.setattr(T._Stepper, 'step', step)
    return lambda: monkeypatch.setattr(T._Stepper, 'step', real)


def _run(store, epochs, capsys=None, resume=None, n=22, **over):
    from lirec_amd.train import training
    mk, model, loss, optim = _train_setup(store)
    opt.set(batch_size=4, epochs=epochs, **over)
    torch.manual_seed(7)
    np.random.seed(7)
    sched = torch.optim.lr_scheduler.LambdaLR(optim, lambda s: 1.0 / (1.0 + 0.1 * s))
    kw = dict(model=model, loss=loss, optimizer=optim, val_dataset=mk(10, 2), test_dataset=mk(9, 3), scheduler=sched)
    if resume is not None:
        kw['resume'] = resume
    try:
        training(mk(n, 1), **kw)
    finally:
        out = capsys.readouterr().out if capsys is not None else ''
    return model, optim, sched, [l for l in out.splitlines() if l.startswith('loss: ')]


def _same_run(a, b):
    (m1, o1, s1, l1), (m2, o2, s2, l2) = a, b
    assert torch.equal(m1.w, m2.w) and torch.equal(m1.wr, m2.wr)
    assert o1.param_groups[0]['lr'] == o2.param_groups[0]['lr'] and s1.last_epoch == s2.last_epoch


def test_boundary_resume_on_the_host(tmp_path, capsys):
    uncut = _run(str(tmp_path / 'uncut'), 4, capsys)
    _run(str(tmp_path / 'cut'), 2, capsys, save_train_state=True)
    ck = torch.load(str(tmp_path / 'cut' / '1.pth.tar'), weights_only=False)
    assert ck['epoch'] == 1 and (ck['train_state']['epoch'], ck['train_state']['batches_done']) == (2, 0)
    assert any(f.startswith('v') for _, _, fs in os.walk(str(tmp_path / 'cut')) for f in fs), 'the kept checkpoints were not written'
    resumed = _run(str(tmp_path / 'cut'), 4, capsys, resume=str(tmp_path / 'cut' / '1.pth.tar'), save_train_state=True)
    _same_run(uncut, resumed)
    assert resumed[3] == uncut[3][2:] and len(resumed[3]) == 2
    a = torch.load(str(tmp_path / 'uncut' / '3.pth.tar'), weights_only=False)
    b = torch.load(str(tmp_path / 'cut' / '3.pth.tar'), weights_only=False)
    assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])
    assert set(a) == {'epoch', 'state_dict', 'optimizer'} and set(b) == set(a) | {'train_state'}
    # today's way -- load_state_dict and training() again -- starts at epoch 0 with step 0's permutations: other parameters
    mk, model, loss, optim = _train_setup(str(tmp_path / 'old'))
    opt.set(batch_size=4, epochs=2)
    model.load_state_dict(ck['state_dict'])
    optim.load_state_dict(ck['optimizer'])
    from lirec_amd.train import training
    torch.manual_seed(7)
    training(mk(22, 1), model=model, loss=loss, optimizer=optim, val_dataset=mk(10, 2), test_dataset=mk(9, 3))
    assert not torch.equal(model.w, uncut[0].w)
    # opt.resume_train with opt.resume_str is the same as resume=; a finished run steps nothing and says so
    capsys.readouterr()
    again = _run(str(tmp_path / 'cut'), 4, capsys, resume_train=True, resume_str=str(tmp_path / 'cut' / '3.pth.tar'))
    assert again[3] == [] and torch.equal(again[0].w, uncut[0].w)


def test_mid_epoch_resume_on_the_host(tmp_path, capsys, monkeypatch):
    uncut = _run(str(tmp_path / 'uncut'), 3, capsys, n=18)
    undo = _cut_after(monkeypatch, 5 + 3)                # (five batches an epoch: the third step of epoch 1)
    with pytest.raises(_Cut):
        _run(str(tmp_path / 'cut'), 3, capsys, n=18, checkpoint_every=2)
    undo()
    last = str(tmp_path / 'cut' / 'last.pth.tar')
    ts = torch.load(last, weights_only=False)['train_state']
    assert (ts['epoch'], ts['batches_done'], ts['steps_taken']) == (1, 2, 7)
    resumed = _run(str(tmp_path / 'cut'), 3, capsys, n=18, resume=last, checkpoint_every=2)
    _same_run(uncut, resumed)
    assert resumed[3] == uncut[3][1:] and len(resumed[3]) == 2           # (the cut epoch's loss line is the uncut one's)
    ts = torch.load(last, weights_only=False)['train_state']
    assert (ts['epoch'], ts['batches_done']) == (3, 0)


def _rank_worker(rank, world, port, root, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from lirec_amd.train import training

        def run(name, epochs, **kw):
            store = os.path.join(root, name, 'rank%d' % rank)
            mk, model, loss, optim = _train_setup(store)
            opt.set(batch_size=4, epochs=epochs, save_train_state=name != 'uncut', checkpoint_every=2)      # (the rolling file: ignored here)
            model.grad_sync = type('Sync', (), {'world': world})()
            training(mk(22, 1), model=model, loss=loss, optimizer=optim, val_dataset=mk(10, 2), test_dataset=mk(9, 3), **kw)
            files = sorted(os.path.relpath(os.path.join(d, f), store) for d, _, fs in os.walk(store) for f in fs)
            return model.w.detach().numpy().copy(), model.wr.detach().numpy().copy(), files
        uncut = run('uncut', 4)
        run('cut', 2)
        resumed = run('cut', 4, resume=os.path.join(root, 'cut', 'rank0', '1.pth.tar'))        # (rank 0's file, read by every rank)
        q.put((rank, uncut, resumed))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_resume_at_a_boundary(tmp_path):
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, uncut, resumed in res:
        assert np.array_equal(uncut[0], resumed[0]) and np.array_equal(uncut[1], resumed[1]), rank
        assert np.array_equal(uncut[0], res[0][1][0])
    assert '3.pth.tar' in res[0][2][2] and 'last.pth.tar' not in res[0][2][2]
    assert res[1][1][2] == [] and res[1][2][2] == []                 # (only rank 0 writes files)
