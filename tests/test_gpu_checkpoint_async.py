"""Asynchronous rolling checkpoints on the GPU (``opt.checkpoint_async``, ``lirec_amd.util.AsyncCheckpointer``, ``lirec_snapshot``;
DESIGN 4.j2).  Bit equality throughout: the snapshot kernel against numpy, the asynchronously written file against the file the
synchronous path writes at the same cut, the state in the file against the state at the cut while the loop has moved on, and a
run continued from the asynchronous file against the run that was never cut.  Nothing here is timed."""
import os
import shutil
import threading

import numpy as np
import pytest
import torch

from lirec_amd import ops, train
from lirec_amd.config import opt
from test_gpu_resume import _Cut, _PoisonedInEpoch, _block, _same, _small

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
# The grid is ceil(words / 1024) workgroups of 256 threads (a word: 16 bytes), 2048 at the most; a thread takes four words a
# round of the unrolled loop, spaced by the grid's 524 288 threads, then single words.  4 197 379 floats (tests/test_gpu_optim.py's
# large size) are 1 049 344 words and three floats: 1025 workgroups, under the cap -- one unrolled round or up to three single
# words a thread, and the three-word tail.  WRAPS is the size that goes round the CAPPED grid: 4 719 360 words and three floats --
# two unrolled rounds of all 2048 workgroups (2 x 2 097 152 words), one round of single words, 768 words of another, the tail.
SMALL = (0, 1, 3, 4, 5, 1023, 1024, 1025)
LARGE = 4197379
WRAPS = 4 * (2 * 2048 * 1024 + 2048 * 256 + 768) + 3
GUARD = 0x5A5A5A5A
_WORDS = {}


def _words():
    """the source words, drawn once: every bit pattern is fair (NaNs, infinities and denormals of fp32 among them)"""
    if not _WORDS:
        rng = np.random.default_rng(20240607)
        host = rng.integers(0, 2 ** 32, size=8 * (LARGE + 8), dtype=np.uint64).astype(np.uint32)
        _WORDS['host'] = host
        _WORDS['dev'] = torch.from_numpy(host.view(np.int32)).cuda()
    return _WORDS['host'], _WORDS['dev']


def _snap(sizes):
    """one call over ranges of ``sizes`` floats: every source at its own 16-byte aligned place in the word pool, every destination
    between guard words in one buffer.  Returns (digests of two calls, numpy's digests, the destination buffer, its expectation)"""
    host, dev = _words()
    up = lambda n: (n + 3) // 4 * 4
    src_at, dst_at, a, d = [], [], 0, 8
    for n in sizes:
        src_at.append(a)
        dst_at.append(d)
        a += up(n) + 4
        d += up(n) + 8                                    # (at least eight guard words between two destinations)
    out = torch.full((d,), GUARD, dtype=torch.int32, device='cuda')
    want = np.full(d, GUARD, dtype=np.uint32)
    pairs = []
    for n, s, t in zip(sizes, src_at, dst_at):
        pairs.append((dev[s:s + n].view(torch.float32), out[t:t + n].view(torch.float32)))
        want[t:t + n] = host[s:s + n]
    dig = torch.full((len(sizes) + 1,), -1, dtype=torch.int64, device='cuda')          # (the call zeroes its words itself)
    ops.snapshot(pairs, dig)
    first = dig.cpu().numpy().view(np.uint64).copy()
    ops.snapshot(pairs, dig)
    second = dig.cpu().numpy().view(np.uint64).copy()
    ref = np.array([host[s:s + n].sum(dtype=np.uint64) for n, s in zip(sizes, src_at)], dtype=np.uint64)
    return first, second, ref, out.cpu().numpy().view(np.uint32), want


@pytest.mark.parametrize('n', [1, 2, 8])
def test_snapshot_copies_bit_for_bit_between_guards_and_leaves_numpys_digests(n):
    every = SMALL + (LARGE,)
    if n == 1:
        calls = [(s,) for s in every + (WRAPS,)]
    elif n == 2:
        calls = [(every[i], every[(i + 1) % len(every)]) for i in range(len(every))] + [(LARGE, LARGE), (WRAPS, 1025)]
    else:
        calls = [SMALL, (LARGE,) + SMALL[1:], SMALL[:7] + (LARGE,), (1025, LARGE, 0, 5, LARGE, 1023, 3, LARGE),
                 (3, WRAPS, 0, 1024, 5, 1, 1023, LARGE)]
    for sizes in calls:
        first, second, ref, got, want = _snap(sizes)
        assert np.array_equal(got, want), (sizes, int((got != want).sum()))            # the copies AND every guard word
        assert np.array_equal(first[:len(sizes)], ref), (sizes, first, ref)
        assert np.array_equal(second, first), sizes                                     # two calls, the same digests
        assert first[len(sizes)] == np.uint64(2 ** 64 - 1), 'a digest word behind the call\'s n was written'
        assert all(ref[i] == 0 for i, s in enumerate(sizes) if s == 0)


def test_snapshot_refuses_overlap_through_the_wrapper():
    from lirec_amd._lib import LirecError
    buf = torch.zeros(256, device='cuda')
    dig = torch.zeros(2, dtype=torch.int64, device='cuda')
    with pytest.raises(LirecError):
        ops.snapshot([(buf[:64], buf[32:96])], dig)
    with pytest.raises(LirecError):
        ops.snapshot([(buf[:32], buf[64:96]), (buf[128:160], buf[80:112])], dig)
    with pytest.raises(LirecError):
        ops.snapshot([(buf[1:33], buf[64:96])], dig)


# ---------------------------------------------------------------------------------------------------------------------------
# helpers: trees, twins
# ---------------------------------------------------------------------------------------------------------------------------
def _tree_same(a, b, what='ck'):
    """every key, every tensor ``torch.equal`` (numpy arrays: equal), every other value ``==``"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (what, set(a) ^ set(b))
        for k in a:
            _tree_same(a[k], b[k], '%s/%s' % (what, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _tree_same(x, y, '%s[%d]' % (what, i))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), what
    else:
        assert type(a) is type(b) and a == b, (what, a, b)


def _load(path):
    return torch.load(path, map_location='cpu', weights_only=False)


class _Clock:
    """``training()``'s start string, the same in both twins"""
    @staticmethod
    def now():
        import datetime
        return datetime.datetime(2024, 1, 1)


def _everything(model):
    from lirec_amd.optim import FusedAdam
    names = [n for n, _ in model.named_parameters()]
    return FusedAdam(model, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True, device_hyper=True, skip_nonfinite=True,
                     ema_decay=0.9, accumulate_steps=3,
                     param_groups=[{'params': names[::2]}, {'params': names[1::2], 'lr': 5e-4, 'weight_decay': 0.0}])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the file is the synchronous file
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('recipe', ['plain', 'everything'])
def test_the_asynchronous_file_is_the_synchronous_file(recipe, monkeypatch, tmp_path):
    """twin runs, the same seeds, 18 clips in batches of 4 (five an epoch), the rolling file every 2 taken steps, cut after the
    third step of epoch 1: the last write stands behind step 7 -- epoch 1, two batches done.  'everything': two AdamW groups in
    device tables, the average, the guard with a NaN batch in epoch 0 (one skipped window by the cut) and accumulate_steps = 3,
    seven micro-steps in: phase 1, the window's gradients in the file -- every range the snapshot can carry."""
    monkeypatch.setattr(train, 'datetime', _Clock)
    kw = dict(n_train=18, tr_cat_distr=True, cut_after=5 + 3, checkpoint_every=2)
    if recipe == 'everything':
        kw.update(make_optim=_everything, wrap=lambda ds: _PoisonedInEpoch(ds, 4, 0), test_fr=1000)
    root = tmp_path / 'run'
    _small(monkeypatch, root, 'int_rel_ch', 3, **kw)
    shutil.copy(str(root / 'last.pth.tar'), str(tmp_path / 'sync.pth.tar'))
    shutil.rmtree(str(root))
    before = threading.active_count()
    on = _small(monkeypatch, root, 'int_rel_ch', 3, checkpoint_async=True, **kw)
    assert threading.active_count() == before
    a, b = _load(str(tmp_path / 'sync.pth.tar')), _load(str(root / 'last.pth.tar'))
    ts = b['train_state']
    assert (b['epoch'], ts['epoch'], ts['batches_done'], ts['steps_taken']) == (1, 1, 2, 7)
    assert on['last']['checkpoint_writes'] == 4 and on['last']['checkpoint_save_s'] > 0.0        # steps 2, 4, the epoch's end, step 7
    if recipe == 'everything':
        assert set(b) == {'epoch', 'state_dict', 'optimizer', 'param_group_names', 'ema', 'train_state'}
        assert ts['skipped_total'] == 1 and ts['window']['phase'] == 1 and ts['window']['k'] == 3
        assert ts['window']['grads'] is not None and bool(ts['window']['grads'].abs().sum() > 0)
    else:
        assert set(b) == {'epoch', 'state_dict', 'optimizer', 'train_state'}
        assert ts['skipped_total'] == 0 and ts['window'] == {'phase': 0, 'k': 1, 'grads': None}
    assert list(a) == list(b) and list(a['state_dict']) == list(b['state_dict'])
    _tree_same(a, b)
    assert not [f for f in os.listdir(str(root)) if '.tmp.' in f]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. isolation, without timing
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_file_holds_the_cut_while_the_loop_moves_on(monkeypatch, tmp_path):
    """34 clips in batches of 4, the rolling file every 4 steps: the writer's ``torch.save`` of the first write blocks on an event;
    the loop takes steps 5 .. 8 behind it, which move every parameter, and only then is the event set (and the run cut, before a
    second write is due).  The file is the state behind step 4, and the loop never waited.  Nothing here depends on how long
    anything takes: a writer that is never released fails the test after a minute."""
    gate, real_save, blocked = threading.Event(), torch.save, []

    def held(obj, f, *a, **k):
        if threading.current_thread().name == 'lirec-checkpoint-writer':
            blocked.append(f)
            assert gate.wait(timeout=60), 'the writer was never released'
        return real_save(obj, f, *a, **k)
    monkeypatch.setattr(torch, 'save', held)
    step, at = train._Stepper.step, {}

    def watched(self, i, batch):
        out = step(self, i, batch)
        n = at['calls'] = at.get('calls', 0) + 1
        if n in (4, 8):
            torch.cuda.synchronize()
            o = self.optimizer
            at[n] = {'params': self.model.flat_params().detach().clone(), 'm': o._m.clone(), 'v': o._v.clone()}
        if n == 8:
            assert len(blocked) == 1 and not os.path.exists(str(tmp_path / 'last.pth.tar')), 'the first write is still held'
            names = [k for k, _ in self.model.named_parameters()]
            moved = [bool((at[8]['params'][off:off + k] != at[4]['params'][off:off + k]).any())
                     for off, k in (self.model._offsets[x] for x in names)]
            assert all(moved), [x for x, m in zip(names, moved) if not m]
            gate.set()
            raise _Cut()
        return out
    try:
        from test_gpu_loops import _setup
        torch.manual_seed(3)
        mk, model, loss, optim = _setup('int_rel_ch', tmp_path, dropout_seed=77)
        opt.set(epochs=1, checkpoint_every=4, checkpoint_async=True)
        optim.param_groups[0]['lr'] = 1e-3
        monkeypatch.setattr(train._Stepper, 'step', watched)
        monkeypatch.setattr(train, '_print', lambda *a, **k: None)
        before = threading.active_count()
        torch.manual_seed(7)
        with pytest.raises(_Cut):
            train.training(mk(34, 1), model=model, loss=loss, optimizer=optim, val_dataset=mk(8, 2))
    finally:
        gate.set()
    assert threading.active_count() == before
    last = train.training.last
    assert last['checkpoint_waits'] == 0 and last['checkpoint_writes'] == 1
    ck = _load(str(tmp_path / 'last.pth.tar'))
    assert ck['train_state']['steps_taken'] == 4
    for name, (off, k) in model._offsets.items():
        cut, later = at[4]['params'][off:off + k].cpu(), at[8]['params'][off:off + k].cpu()
        assert torch.equal(ck['state_dict'][name].reshape(-1), cut) and not torch.equal(ck['state_dict'][name].reshape(-1), later), name
    number = {n: i for i, n in enumerate(n for n, _ in model.named_parameters())}
    for name, (off, k) in model._offsets.items():
        st = ck['optimizer']['state'][number[name]]
        assert torch.equal(st['exp_avg'].reshape(-1), at[4]['m'][off:off + k].cpu()), name
        assert torch.equal(st['exp_avg_sq'].reshape(-1), at[4]['v'][off:off + k].cpu()) and float(st['step']) == 4.0, name


# ---------------------------------------------------------------------------------------------------------------------------
# 4. a side stream that is late
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_snapshot_right_behind_a_replay_with_a_late_side_stream_is_the_synchronised_state(tmp_path):
    """the recorded step leaves bucket 0's update running on lane 0 (the deferred join exists at the headline's shape only, so this
    one test runs there, as tests/test_gpu_recorded_bench_shape.py does); that stream is held back ~2 ms per step (lirec_debug_set
    bit 131072).  ``save()`` right behind the last replay joins what ``state_dict()`` joins: the file is the state after a full
    synchronise."""
    from lirec_amd import _lib
    from lirec_amd.data import to_device_batch
    from lirec_amd.graph import RecordedTrainStep
    from lirec_amd.util import AsyncCheckpointer
    from test_gpu_recorded_bench_shape import B, R, T, _fresh, host_batch
    model, loss, optim = _fresh(False)
    batch = to_device_batch(host_batch(B, T, R, 'survey'), 'cuda')
    lane = model._wgrad_lane()
    assert lane is not None
    with lane[1]:
        _lib.lib().lirec_debug_set(131072, -1)
    ck = AsyncCheckpointer(model, optim)
    try:
        g = RecordedTrainStep(model, loss, optim, batch, warmup=2)
        assert g.defer
        for _ in range(3):
            g.step()
        assert model.lanes.unjoined
        ck.save(str(tmp_path / 'last.pth.tar'), 0)
        ck.close()
        torch.cuda.synchronize()
    finally:
        with lane[1]:
            _lib.lib().lirec_debug_set(0, -1)
        ck.close()
    got = _load(str(tmp_path / 'last.pth.tar'))
    assert set(got) == {'epoch', 'state_dict', 'optimizer'}
    want = {'epoch': 0, 'state_dict': dict(model.state_dict()), 'optimizer': optim.state_dict()}
    want = torch.utils._pytree.tree_map(lambda x: x.cpu() if torch.is_tensor(x) else x, want)
    _tree_same(want, dict(got, state_dict=dict(got['state_dict'])))
    assert ck.stats['writes'] == 1 and ck.stats['waits'] == 0
    g.release()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. resume
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_run_continued_from_the_asynchronous_file_ends_on_the_uncut_bits_eager(monkeypatch, tmp_path):
    """tests/test_gpu_resume.py C with the flag on in the cut half (and off in the continued one: a loop field)"""
    kw = dict(n_train=18, tr_cat_distr=True)
    uncut = _small(monkeypatch, tmp_path / 'uncut', 'int_rel_ch', 3, **kw)
    cut = _small(monkeypatch, tmp_path / 'cut', 'int_rel_ch', 3, cut_after=5 + 3, checkpoint_every=2, checkpoint_async=True, **kw)
    assert cut['last']['checkpoint_writes'] == 4
    last = str(tmp_path / 'cut' / 'last.pth.tar')
    ts = _load(last)['train_state']
    assert (ts['epoch'], ts['batches_done'], ts['steps_taken'], ts['seen']) == (1, 2, 7, 8)
    resumed = _small(monkeypatch, tmp_path / 'cut', 'int_rel_ch', 3, resume=last, save_train_state=True, **kw)
    _same(uncut, resumed, 2)


def test_a_run_continued_from_the_asynchronous_file_ends_on_the_uncut_bits_block_store_bind(monkeypatch, tmp_path):
    """tests/test_gpu_resume.py D, 'bind', inside epoch 2: the snapshots are taken between replays of the recorded step"""
    uncut = _block(monkeypatch, tmp_path / 'uncut', 'bind', 4)
    cut = _block(monkeypatch, tmp_path / 'm', 'bind', 4, cut_after=5 + 5 + 3, checkpoint_every=2, checkpoint_async=True)
    assert cut['last']['replays'] == 4 + 3 and cut['last']['checkpoint_writes'] == 3 + 3 + 1
    last = str(tmp_path / 'm' / 'last.pth.tar')
    ts = _load(last)['train_state']
    assert (ts['epoch'], ts['batches_done'], ts['steps_taken'], ts['dropout_calls']) == (2, 2, 12, 12)
    resumed = _block(monkeypatch, tmp_path / 'm', 'bind', 4, resume=last, checkpoint_async=True, checkpoint_every=2)
    for k in ('params', 'm', 'v'):
        assert torch.equal(uncut[k], resumed[k]), (k, int((uncut[k] != resumed[k]).sum()))
    assert resumed['losses'] == uncut['losses'][2:] and resumed['recorded']


# ---------------------------------------------------------------------------------------------------------------------------
# 6. back-pressure and failure
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_write_after_every_step_loses_none_and_ends_on_the_synchronous_file(monkeypatch, tmp_path):
    """30 clips in batches of 4, a write after every step, cut after the seventh step before its write: six writes, each waiting
    for the one before it when that is still running; the file is the synchronous twin's"""
    monkeypatch.setattr(train, 'datetime', _Clock)
    kw = dict(n_train=30, cut_after=7, checkpoint_every=1)
    root = tmp_path / 'run'
    _small(monkeypatch, root, 'int_rel_ch', 1, **kw)
    shutil.copy(str(root / 'last.pth.tar'), str(tmp_path / 'sync.pth.tar'))
    shutil.rmtree(str(root))
    on = _small(monkeypatch, root, 'int_rel_ch', 1, checkpoint_async=True, **kw)
    assert on['last']['checkpoint_writes'] == 6 and 0 <= on['last']['checkpoint_waits'] <= 5
    a, b = _load(str(tmp_path / 'sync.pth.tar')), _load(str(root / 'last.pth.tar'))
    assert b['train_state']['steps_taken'] == 6
    _tree_same(a, b)


def test_a_failed_write_surfaces_keeps_the_earlier_file_and_leaves_no_thread(monkeypatch, tmp_path):
    """the store stops taking writes behind the first one (a directory sits where the temporary file goes: ``torch.save`` cannot
    open it -- the same for every user): ``save()`` itself returns, the error is raised by ``close()`` -- or by the next
    ``save()`` --, the first file is there bit for bit, the writer is gone.  Then through ``training()``: the loop ends with the
    writer's error, no thread survives it."""
    from lirec_amd.util import AsyncCheckpointer
    from test_gpu_loops import _setup
    torch.manual_seed(3)
    mk, model, loss, optim = _setup('int_rel_ch', tmp_path, dropout_seed=77)
    path = str(tmp_path / 'last.pth.tar')
    before = threading.active_count()
    ck = AsyncCheckpointer(model, optim)
    ck.save(path, 0)
    ck.wait()
    first = open(path, 'rb').read()
    os.mkdir('%s.tmp.%d' % (path, os.getpid()))
    model.flat_params().data.add_(1.0)
    ck.save(path, 1)                                       # (returns: the failure is the writer's)
    with pytest.raises(OSError):
        ck.save(path, 2)
    ck.save(path, 3)
    with pytest.raises(OSError):
        ck.close()
    ck.close()                                             # (idempotent; the error was handed over once)
    with pytest.raises(RuntimeError, match='closed'):
        ck.save(path, 4)
    assert open(path, 'rb').read() == first and ck.stats['writes'] == 1
    assert threading.active_count() == before
    # through training(): every rolling write fails
    monkeypatch.setattr(train, '_print', lambda *a, **k: None)
    opt.set(epochs=1, checkpoint_every=2, checkpoint_async=True)
    with pytest.raises(OSError):
        train.training(mk(18, 1), model=model, loss=loss, optimizer=optim, val_dataset=mk(8, 2))
    assert threading.active_count() == before and train.training.last['checkpoint_writes'] == 0
    assert open(path, 'rb').read() == first
