"""training(resume=...) on the GPU: a run cut at an epoch boundary or inside an epoch and continued by freshly built objects ends on
the BITS of the run that was never cut -- ``torch.equal`` on parameters, Adam's moments, the average, every tensor of the final
checkpoint; ``==`` on the printed ``loss:`` lines, the evaluation metrics and the host counters.  No tolerance anywhere.  The
interruption is an exception out of a wrapped ``_Stepper.step``; nothing is killed."""
import os

import numpy as np
import pytest
import torch

from lirec_amd import config, train
from lirec_amd.config import opt

pytestmark = pytest.mark.gpu
_STEP = train._Stepper.step


class _Cut(Exception):
    pass


def _watch(monkeypatch, cut_after=None):
    """what a run printed and evaluated; ``cut_after`` = n: an exception out of the n-th step call, after that step was taken"""
    seen = {'lines': [], 'metrics': [], 'calls': 0, 'recorded': False}
    monkeypatch.setattr(train, '_print', lambda *a, **k: seen['lines'].append(' '.join(str(x) for x in a)))
    from lirec_amd.test import testing as real_testing

    def testing(ds, *a, **k):
        out = real_testing(ds, *a, **k)
        seen['metrics'].append((k.get('mode'), k.get('total_iter'), {m: float(v) for m, v in out.items()}))
        return out
    monkeypatch.setattr(train, 'testing', testing)

    def step(self, i, batch):
        out = _STEP(self, i, batch)
        seen['calls'] += 1
        seen['recorded'] = seen['recorded'] or self.recorded is not None
        if cut_after is not None and seen['calls'] == cut_after:
            raise _Cut()
        return out
    monkeypatch.setattr(train._Stepper, 'step', step)
    return seen


def _result(model, optim, seen, sched=None):
    torch.cuda.synchronize()
    return {'params': model.flat_params().detach().clone(), 'm': optim._m.clone(), 'v': optim._v.clone(),
            'losses': [l for l in seen['lines'] if l.startswith('loss: ')], 'metrics': seen['metrics'], 'optim': optim, 'sched': sched,
            'last': dict(train.training.last), 'recorded': seen['recorded'], 'lines': seen['lines']}


def _same_tensors(a, b, what=''):
    """every tensor of two checkpoint trees equal, everything else equal too (``train_state`` and file paths aside)"""
    if isinstance(a, dict):
        assert set(a) == set(b), (what, set(a) ^ set(b))
        for k in a:
            _same_tensors(a[k], b[k], '%s/%s' % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tensors(x, y, '%s[%d]' % (what, i))
    elif torch.is_tensor(a):
        assert torch.equal(a, b), what
    else:
        assert a == b, (what, a, b)


def _same_checkpoint(pa, pb):
    a, b = torch.load(pa, weights_only=False), torch.load(pb, weights_only=False)
    a.pop('train_state', None), b.pop('train_state', None)
    _same_tensors(a, b)


def _same(uncut, resumed, n_epochs, evaluated=True):
    """parameters, moments, the loss lines and the evaluations of the last ``n_epochs`` epochs"""
    for k in ('params', 'm', 'v'):
        assert torch.equal(uncut[k], resumed[k]), (k, int((uncut[k] != resumed[k]).sum()))
    assert len(resumed['losses']) == n_epochs and resumed['losses'] == uncut['losses'][-n_epochs:], (resumed['losses'], uncut['losses'])
    first = len(uncut['losses']) - n_epochs
    want = [m for m in uncut['metrics'] if m[1] >= first]
    assert resumed['metrics'] == want and bool(want) == evaluated, (resumed['metrics'], want)


# ---------------------------------------------------------------------------------------------------------------------------
# A - C, F: the reduced shapes of tests/test_gpu_loops.py
# ---------------------------------------------------------------------------------------------------------------------------
def _small(monkeypatch, tmp_path, kind, epochs, n_train=10, resume=None, cut_after=None, make_optim=None, make_sched=None,
           wrap=lambda ds: ds, **over):
    from test_gpu_loops import _setup
    torch.manual_seed(3)
    late = {k: over.pop(k) for k in ('batch_size', 'test_fr') if k in over}          # (what _setup fixes itself: set behind it)
    mk, model, loss, optim = _setup(kind, tmp_path, dropout_seed=77, **over)
    opt.set(epochs=epochs, **late)
    if make_optim is not None:
        optim = make_optim(model)
    else:
        optim.param_groups[0]['lr'] = 1e-3
    sched = make_sched(optim) if make_sched is not None else None
    seen = _watch(monkeypatch, cut_after)
    torch.manual_seed(7)
    kw = dict(model=model, loss=loss, optimizer=optim, val_dataset=mk(8, 2), test_dataset=mk(7, 3))
    if sched is not None:
        kw['scheduler'] = sched
    if resume is not None:
        kw['resume'] = resume
    try:
        train.training(wrap(mk(n_train, 1)), **kw)
    except _Cut:
        assert cut_after is not None
    return _result(model, optim, seen, sched)


@pytest.mark.parametrize('kind', ['modalties', 'int_rels', 'int_ch', 'int_rel_ch'])
def test_boundary_resume_all_four_recipes(kind, monkeypatch, tmp_path):
    """A. 4 epochs uncut against 2 epochs + fresh objects + training(resume=) for 2 more; today's way -- load_state_dict and
    training() again -- does not give those parameters (the counters, the epoch and the RNG start over)."""
    over = dict(tr_cat_distr=True) if kind == 'int_rel_ch' else {}            # (the track sampler's counter is state too)
    uncut = _small(monkeypatch, tmp_path / 'uncut', kind, 4, **over)
    assert len(uncut['losses']) == 4 and torch.isfinite(uncut['params']).all()
    half = _small(monkeypatch, tmp_path / 'cut', kind, 2, save_train_state=True, **over)
    assert half['losses'] == uncut['losses'][:2]
    path = str(tmp_path / 'cut' / '1.pth.tar')
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {'epoch', 'state_dict', 'optimizer', 'train_state'} and ck['epoch'] == 1
    ts = ck['train_state']
    assert (ts['version'], ts['epoch'], ts['batches_done'], ts['steps_taken'], ts['dropout_calls']) == (1, 2, 0, 6, 6)
    resumed = _small(monkeypatch, tmp_path / 'cut', kind, 4, resume=path, save_train_state=True, **over)
    _same(uncut, resumed, 2)
    _same_checkpoint(str(tmp_path / 'uncut' / '3.pth.tar'), str(tmp_path / 'cut' / '3.pth.tar'))
    # the control: model.load_state_dict + optimizer.load_state_dict, then training() for the two epochs that are left
    from test_gpu_loops import _setup
    torch.manual_seed(3)
    mk, model, loss, optim = _setup(kind, tmp_path / 'old', dropout_seed=77, **over)
    model.load_state_dict(ck['state_dict'])
    optim.load_state_dict(ck['optimizer'])
    seen = _watch(monkeypatch)
    torch.manual_seed(7)
    train.training(mk(10, 1), model=model, loss=loss, optimizer=optim, val_dataset=mk(8, 2), test_dataset=mk(7, 3))
    old = _result(model, optim, seen)
    assert not torch.equal(old['params'], uncut['params'])


class _PoisonedInEpoch(torch.utils.data.Dataset):
    """the dataset with a NaN in one clip's features while ``epoch`` is ``when``"""

    def __init__(self, ds, idx, when):
        self.ds, self.idx, self.when, self.epoch = ds, idx, when, 0
        self.n_classes, self.n_rels, self.interidx2mgdidx = ds.n_classes, ds.n_rels, ds.interidx2mgdidx

    def __getattr__(self, name):          # (whatever else the loop asks a dataset for)
        return getattr(self.ds, name)

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        s = dict(self.ds[i])
        if i == self.idx and self.epoch == self.when:
            f = s['features'].clone() if torch.is_tensor(s['features']) else np.array(s['features'], copy=True)
            f[(0,) * (f.ndim - 1) + (5,)] = float('nan')
            s['features'] = f
        return s


def test_everything_the_optimiser_can_carry_at_once(monkeypatch, tmp_path):
    """B. two AdamW groups with device_hyper, clip, the guard with a NaN batch before the cut (epoch 1), the average, a per-step
    LambdaLR, and accumulate_steps=2 over three micro-batches an epoch -- cut after THREE epochs, nine micro-batches, so that the
    window is open at the boundary (after two it would be closed) -- against five epochs uncut."""
    from lirec_amd.optim import FusedAdam

    def make_optim(model):
        names = [n for n, _ in model.named_parameters()]
        return FusedAdam(model, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True, device_hyper=True, max_grad_norm=0.5,
                         skip_nonfinite=True, ema_decay=0.9, accumulate_steps=2,
                         param_groups=[{'params': names[::2]}, {'params': names[1::2], 'lr': 5e-4, 'weight_decay': 0.0}])
    make_sched = lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda s: 1.0 / (1.0 + 0.25 * s))
    kw = dict(make_optim=make_optim, make_sched=make_sched, wrap=lambda ds: _PoisonedInEpoch(ds, 4, 1), test_fr=1000)
    uncut = _small(monkeypatch, tmp_path / 'uncut', 'int_rel_ch', 5, **kw)
    assert uncut['optim'].skipped_total() == 1 and torch.isfinite(uncut['params']).all()
    half = _small(monkeypatch, tmp_path / 'cut', 'int_rel_ch', 3, save_train_state=True, **kw)
    path = str(tmp_path / 'cut' / '2.pth.tar')
    ts = torch.load(path, weights_only=False)['train_state']
    assert ts['window']['phase'] == 1 and ts['window']['k'] == 2 and ts['window']['grads'] is not None
    assert ts['skipped_total'] == 1 and ts['scheduler']['last_epoch'] == 4            # (four windows closed, one of them skipped: the scheduler counts them as issued)
    resumed = _small(monkeypatch, tmp_path / 'cut', 'int_rel_ch', 5, resume=path, save_train_state=True, **kw)
    _same(uncut, resumed, 2, evaluated=False)
    a, b = uncut['optim'], resumed['optim']
    assert torch.equal(a.ema, b.ema) and a.ema_updates() == b.ema_updates() > 0
    assert a.accum_phase == b.accum_phase and a.skipped_total() == b.skipped_total() == 1
    assert [g['lr'] for g in a.param_groups] == [g['lr'] for g in b.param_groups]
    assert uncut['sched'].last_epoch == resumed['sched'].last_epoch
    _same_checkpoint(str(tmp_path / 'uncut' / '4.pth.tar'), str(tmp_path / 'cut' / '4.pth.tar'))
    # the window mattered: dropped at the cut, the run ends elsewhere
    dropped = dict(torch.load(path, weights_only=False))
    dropped['train_state'] = dict(dropped['train_state'], window={'phase': 0, 'k': 2, 'grads': None})
    other = _small(monkeypatch, tmp_path / 'other', 'int_rel_ch', 5, resume=dropped, **kw)
    assert not torch.equal(other['params'], uncut['params'])


def test_mid_epoch_resume(monkeypatch, tmp_path):
    """C. 18 clips in batches of 4 (five batches an epoch), the rolling file every 2 taken steps; cut inside epoch 1 after its third
    step: the file says epoch 1, two batches done"""
    kw = dict(n_train=18, tr_cat_distr=True)
    uncut = _small(monkeypatch, tmp_path / 'uncut', 'int_rel_ch', 3, **kw)
    _small(monkeypatch, tmp_path / 'cut', 'int_rel_ch', 3, cut_after=5 + 3, checkpoint_every=2, **kw)
    last = str(tmp_path / 'cut' / 'last.pth.tar')
    ck = torch.load(last, weights_only=False)
    ts = ck['train_state']
    assert (ck['epoch'], ts['epoch'], ts['batches_done'], ts['steps_taken'], ts['seen']) == (1, 1, 2, 7, 8)
    assert not os.path.exists(str(tmp_path / 'cut' / '2.pth.tar'))
    resumed = _small(monkeypatch, tmp_path / 'cut', 'int_rel_ch', 3, resume=last, checkpoint_every=2, save_train_state=True, **kw)
    _same(uncut, resumed, 2)                                      # (the cut epoch's loss line is the uncut one's)
    assert [l for l in resumed['lines'] if l in ('18', '8', '10')] == ['18', '18']         # (and its clip count)
    _same_checkpoint(str(tmp_path / 'uncut' / '2.pth.tar'), str(tmp_path / 'cut' / '2.pth.tar'))
    ts = torch.load(last, weights_only=False)['train_state']
    assert (ts['epoch'], ts['batches_done']) == (3, 0)


def test_refusals_and_the_finished_run(monkeypatch, tmp_path):
    """F. a plain checkpoint, a changed batch size, and a resume whose epoch is already opt.epochs"""
    half = _small(monkeypatch, tmp_path, 'int_ch', 2, save_train_state=True)
    path = str(tmp_path / '1.pth.tar')
    ck = torch.load(path, weights_only=False)
    plain = {k: v for k, v in ck.items() if k != 'train_state'}
    with pytest.raises(ValueError, match='holds no train state'):
        _small(monkeypatch, tmp_path, 'int_ch', 4, resume=plain)
    with pytest.raises(ValueError, match='batch_size differs'):
        _small(monkeypatch, tmp_path, 'int_ch', 4, resume=path, batch_size=5)
    with pytest.raises(ValueError, match='version 7'):
        _small(monkeypatch, tmp_path, 'int_ch', 4, resume=dict(ck, train_state=dict(ck['train_state'], version=7)))
    done = _small(monkeypatch, tmp_path, 'int_ch', 2, resume=path)
    assert done['losses'] == [] and done['metrics'] == [] and any('nothing to do' in l for l in done['lines'])
    assert torch.equal(done['params'], half['params'])           # (the model that is returned holds the checkpoint's weights)


# ---------------------------------------------------------------------------------------------------------------------------
# D: full width, block store, recorded
# ---------------------------------------------------------------------------------------------------------------------------
def _block(monkeypatch, tmp_path, mode, epochs, resume=None, cut_after=None, save_model=False, **over):
    from lirec_amd import blockstore as BS
    from lirec_amd.data import SyntheticMixedFeaturesDataset
    from test_gpu_blockstore_recorded import _model
    model, loss, optim = _model('int_rels', 18, batch_size=5, num_workers=0, epochs=epochs, test_fr=1000, store_root=str(tmp_path),
                                record_block_store=mode, save_model=save_model, **over)
    ds = BS.ResidentBlockDataset(SyntheticMixedFeaturesDataset('int_rels', 24, seed=31, soft_gt=opt.soft_gt, R=18))
    seen = _watch(monkeypatch, cut_after)
    torch.manual_seed(7)
    try:
        train.training(ds, model=model, loss=loss, optimizer=optim, **({} if resume is None else {'resume': resume}))
    except _Cut:
        assert cut_after is not None
    return _result(model, optim, seen)


@pytest.mark.parametrize('mode', ['bind', 'list'])
def test_block_store_recorded_run_resumes_at_a_boundary_and_inside_an_epoch(mode, monkeypatch, tmp_path):
    """D. int_rels, R = 18, 24 clips in batches of 5, D = 6912: four epochs uncut (the step recorded on epoch 0's fourth batch, four
    replays an epoch from then on) against a cut after epoch 1 and against a cut inside epoch 2 after two replays.  The recorded
    step is not in a checkpoint: the resumed half steps eagerly and records again on the fourth batch of its layout -- after the
    boundary cut in epoch 2, replaying in epoch 3 (under 'list' those draw their own ids at the loader's cursor); after the cut
    inside epoch 2, whose three remaining batches are too few, in epoch 3."""
    from lirec_amd.loader import BlockLoader
    uncut = _block(monkeypatch, tmp_path / 'uncut', mode, 4)
    assert uncut['last']['replays'] == 12 and isinstance(uncut['last']['loader'], BlockLoader) and len(uncut['losses']) == 4
    # at the boundary
    _block(monkeypatch, tmp_path / 'b', mode, 2, save_train_state=True, save_model=True)
    resumed = _block(monkeypatch, tmp_path / 'b', mode, 4, resume=str(tmp_path / 'b' / '1.pth.tar'))
    for k in ('params', 'm', 'v'):
        assert torch.equal(uncut[k], resumed[k]), (mode, 'boundary', k, int((uncut[k] != resumed[k]).sum()))
    assert resumed['losses'] == uncut['losses'][2:]
    assert resumed['last']['replays'] == 4 and resumed['last']['input_copies'] == 0
    assert resumed['last']['loader'].n_in_list == (4 if mode == 'list' else 0)
    assert not [l for l in resumed['lines'] if 'not used' in l]
    # inside epoch 2: two replays taken, the file written behind them, the cut after the third
    cut = _block(monkeypatch, tmp_path / 'm', mode, 4, cut_after=5 + 5 + 3, checkpoint_every=2)
    assert cut['last']['replays'] == 4 + 3
    last = str(tmp_path / 'm' / 'last.pth.tar')
    ts = torch.load(last, weights_only=False)['train_state']
    assert (ts['epoch'], ts['batches_done'], ts['steps_taken'], ts['dropout_calls']) == (2, 2, 12, 12)
    resumed = _block(monkeypatch, tmp_path / 'm', mode, 4, resume=last)
    for k in ('params', 'm', 'v'):
        assert torch.equal(uncut[k], resumed[k]), (mode, 'inside', k, int((uncut[k] != resumed[k]).sum()))
    assert resumed['losses'] == uncut['losses'][2:]
    assert resumed['recorded'] and not [l for l in resumed['lines'] if 'not used' in l]


# ---------------------------------------------------------------------------------------------------------------------------
# E: the resident piece store, collated on the device, context redrawn per epoch
# ---------------------------------------------------------------------------------------------------------------------------
def _pieces(monkeypatch, tmp_path, epochs, resume=None, **over):
    from lirec_amd import features as F
    from test_pieces_entry import R, _fresh
    world = F.synthetic_world(3)
    torch.manual_seed(0)
    model, loss, optim = _fresh(world)
    # (opt.test off: the train set is evaluated after every epoch, no best checkpoints of the full-width model are kept)
    opt.set(store_root=str(tmp_path), batch_size=5, num_workers=1, epochs=epochs, device_collate=True, save_model=True, test=False, **over)
    optim.param_groups[0]['lr'] = 1e-3
    ds = F.PiecesDataset(world, R, resident=True, context_draw='random', context_seed=0x5eed00000007)
    val = F.PiecesDataset(F.synthetic_world(8), R, n_classes=ds.n_classes, resident=True)
    seen = _watch(monkeypatch)
    torch.manual_seed(99)
    train.training(ds, model=model, loss=loss, optimizer=optim, val_dataset=val, **({} if resume is None else {'resume': resume}))
    return _result(model, optim, seen), ds


def test_resident_piece_store_with_random_context_resumes_at_a_boundary(monkeypatch, tmp_path):
    """E. ``opt.device_collate`` over a ``PiecesDataset(context_draw='random')`` of the synthetic world's defaults: the restored epoch
    number gives the uncut run's draws"""
    from lirec_amd.loader import ResidentLoader
    try:
        uncut, ds = _pieces(monkeypatch, tmp_path / 'uncut', 4)
        assert isinstance(uncut['last']['loader'], ResidentLoader) and uncut['last']['replays'] > 0
        _pieces(monkeypatch, tmp_path / 'cut', 2, save_train_state=True)
        resumed, ds = _pieces(monkeypatch, tmp_path / 'cut', 4, resume=str(tmp_path / 'cut' / '1.pth.tar'))
        _same(uncut, resumed, 2)
        assert resumed['last']['replays'] > 0
        if ds.slot_dst.size:
            assert resumed['last']['loader'].n_draw == 2           # (epochs 2 and 3: the restored epoch number keys the draw)
    finally:
        config.reset()
