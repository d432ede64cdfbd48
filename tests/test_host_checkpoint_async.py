"""Asynchronous rolling checkpoints without a GPU: the export and every refusal of lirec_snapshot before any device
call under the library's host-side dry run, what an accepted call records; the builders a checkpoint is made with -- from flat
buffers given from outside and the host integers of a cut -- against ``state_dict()``, ``ema_entry`` and ``window_state()`` of the
same optimiser; and ``training()`` with the flag off, and with no rolling file to write, making neither a checkpointer nor a
snapshot."""
import copy
import ctypes as C
import threading

import pytest
import torch

from lirec_amd import _lib, config, ops
from lirec_amd.config import opt

DRY = 4194304
EINVAL = _lib.LIREC_EINVAL
SRC, DST, DIG = 0x20000000, 0x30000000, 0x40000000       # fake, aligned, never dereferenced device addresses


@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def _call(L, src, dst, nbytes, n=None, dig=DIG):
    n = len(src) if n is None else n
    m = max(len(src), 1)
    return L.lirec_snapshot((C.c_void_p * m)(*src), (C.c_void_p * m)(*dst), (C.c_int64 * m)(*nbytes), n, dig, None)


def test_the_export_and_the_abi_number():
    L = _lib.lib()
    assert 'lirec_snapshot' in _lib.EXPORTS and hasattr(L, 'lirec_snapshot')
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert ops.SNAPSHOT_MAX_RANGES == 8


def test_snapshot_refusals_before_any_device_call(dry):
    L = dry
    step = 0x100000
    ok = lambda n: ([SRC + i * step for i in range(n)], [DST + i * step for i in range(n)], [4096 + 4 * i for i in range(n)])
    for n in (1, 2, 8):
        assert _call(L, *ok(n)) == 0
    assert _call(L, [SRC], [DST], [0]) == 0 and _call(L, [SRC, SRC], [DST, DST], [0, 0]) == 0      # empty ranges share nothing
    assert _call(L, [SRC, SRC], [DST, DST + step], [64, 64]) == 0                                  # one source twice: only read
    assert _call(L, [SRC], [SRC + 64], [64]) == 0                                                  # adjacent, not overlapping
    s9 = ok(8)
    assert _call(L, *ok(1), n=0) == EINVAL and _call(L, *ok(1), n=-1) == EINVAL                    # n outside 1 .. 8
    assert _call(L, s9[0] + [SRC + 9 * step], s9[1] + [DST + 9 * step], s9[2] + [16], n=9) == EINVAL
    assert L.lirec_snapshot(None, (C.c_void_p * 1)(DST), (C.c_int64 * 1)(16), 1, DIG, None) == EINVAL        # null arrays
    assert L.lirec_snapshot((C.c_void_p * 1)(SRC), None, (C.c_int64 * 1)(16), 1, DIG, None) == EINVAL
    assert L.lirec_snapshot((C.c_void_p * 1)(SRC), (C.c_void_p * 1)(DST), None, 1, DIG, None) == EINVAL
    assert _call(L, [SRC], [DST], [16], dig=None) == EINVAL and _call(L, [SRC], [DST], [16], dig=DIG + 4) == EINVAL
    assert _call(L, [None], [DST], [16]) == EINVAL and _call(L, [SRC], [None], [16]) == EINVAL     # a null pointer
    assert _call(L, [None], [DST], [0]) == EINVAL                                                  # ... of an empty range too
    assert _call(L, [SRC, None], [DST, DST + step], [16, 16]) == EINVAL
    for off in (4, 8, 12, 1):                                                                      # off a 16-byte boundary
        assert _call(L, [SRC + off], [DST], [16]) == EINVAL and _call(L, [SRC], [DST + off], [16]) == EINVAL
    for bad in (-4, -1, 1, 2, 3, 5, 18):                                                           # negative / no multiple of 4
        assert _call(L, [SRC], [DST], [bad]) == EINVAL
    assert _call(L, [SRC, SRC + step], [DST, DST + step], [16, 6]) == EINVAL
    # a destination that shares a byte with a source, with another destination, with the digest words
    assert _call(L, [SRC], [SRC], [64]) == EINVAL and _call(L, [SRC], [SRC + 48], [64]) == EINVAL
    assert _call(L, [SRC + 48], [SRC], [64]) == EINVAL
    assert _call(L, [SRC, SRC + step], [DST, SRC], [64, 64]) == EINVAL                             # dst[1] on src[0]
    assert _call(L, [SRC, SRC + step], [DST, DST + 48], [64, 64]) == EINVAL                        # dst[1] on dst[0]
    assert _call(L, [SRC, SRC + step], [DST, DST], [64, 64]) == EINVAL
    assert _call(L, [SRC], [DIG], [16]) == EINVAL and _call(L, [SRC, SRC + step], [DST, DIG - 16], [16, 32]) == EINVAL


def test_an_accepted_call_records_its_one_kernel_launch_behind_the_digest_memset(dry):
    """the call zeroes the digest words itself -- a memset on the stream -- and issues ONE kernel launch for all ranges, however
    many: two commands of kind 0 (launch / memset) on the call's stream, replayable; a refused call records nothing"""
    L = dry
    for n in (1, 3, 8):
        assert L.lirec_record_begin() == 0
        assert L.lirec_record_mark() == 0
        assert _call(L, [SRC + i * 0x100000 for i in range(n)], [DST + i * 0x100000 for i in range(n)], [1 << 20] * n) == 0
        assert L.lirec_record_mark() == 2
        assert _call(L, [SRC], [SRC], [64]) == EINVAL and L.lirec_record_mark() == 2
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0 and L.lirec_cmdlist_size(h) == 2
        for i in range(2):
            s, k = C.c_void_p(), C.c_int32()
            assert L.lirec_cmdlist_command(h, i, C.byref(s), C.byref(k)) == 0 and k.value == 0 and not s.value
        assert L.lirec_cmdlist_replay(h, 0, -1) == 0 and L.lirec_cmdlist_destroy(h) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------------
def _tree_equal(a, b, what=''):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (what, list(a), list(b))
        for k in a:
            _tree_equal(a[k], b[k], '%s/%s' % (what, k))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _tree_equal(x, y, '%s[%d]' % (what, i))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    else:
        assert type(a) is type(b) and a == b, (what, a, b)


def _optimiser(everything):
    from lirec_amd import model as M
    from lirec_amd.optim import FusedAdam
    config.recipe('int_rel_ch', joint_dim=16, dropout=0.3, dropout_seed=5, text_dim=24, visual_dim=32, track_dim=32, rels_n_clips=3)
    opt.device = 'cpu'
    torch.manual_seed(11)
    model, _, optim = M.create_model(11, n_rels=5)
    if everything:
        names = [n for n, _ in model.named_parameters()]
        optim = FusedAdam(model, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True, device_hyper=True, max_grad_norm=0.5,
                          skip_nonfinite=True, ema_decay=0.9, accumulate_steps=3,
                          param_groups=[{'params': names[::2]}, {'params': names[1::2], 'lr': 5e-4, 'weight_decay': 0.0}])
    optim._ensure_state()
    g = torch.Generator().manual_seed(5)
    optim._m.copy_(torch.randn(optim._m.shape, generator=g))
    optim._v.copy_(torch.rand(optim._v.shape, generator=g))
    optim._step = 9
    if everything:
        optim.ema.copy_(torch.randn(optim.ema.shape, generator=g))
        optim._ema_calls, optim._ema_done, optim._ema_skip_base = 7, 1, 1
        model._plist[3].requires_grad_(False)
        optim._lag = {optim._names[3]: 4, optim._names[5]: 1}
        optim._clip_buffers()
        optim._skipped_dev.fill_(2)                      # two guarded steps skipped since the fold ...
        optim._guard_flags = optim._flags()
        optim._skipped_folded = 1                        # ... and one before it
        model.flat_grads(attach=True).copy_(torch.randn(optim._m.shape, generator=g))
        optim._accum_phase = 1
    return model, optim


@pytest.mark.parametrize('everything', [False, True], ids=['plain', 'everything'])
def test_the_builders_over_outside_buffers_give_the_state_dicts_of_the_optimiser(everything):
    from lirec_amd.train import TrainState  # noqa: F401  (the module that fills the two device-side fields in)
    from lirec_amd.util import checkpoint_dict, ema_entry, ema_entry_from
    model, optim = _optimiser(everything)
    # (deep copies: the live state_dict()s are views of the buffers that move on below)
    want_sd, want_osd, want_ema, want_win = copy.deepcopy((model.state_dict(), optim.state_dict(), ema_entry(optim), optim.window_state()))
    want_skipped = optim.skipped_total()
    # the cut: host integers now, copies of the buffers, the count word read from ITS copy
    cut, model_layout, state_layout = optim.host_cut(), model.state_dict_layout(), optim.state_layout()
    flat, m, v = model.flat_params().detach().clone(), optim._m.clone(), optim._v.clone()
    ema = optim.ema.clone() if everything else None
    grads = model.flat_grads(attach=True).detach().clone() if everything else None
    word = int(optim._skipped_dev.clone()[0]) if everything else 0
    assert (cut['guard_flags'] is not None) == everything
    # ... after which the live optimiser moves on: nothing built below may look at it
    optim._m.add_(1.0), optim._v.mul_(2.0), model.flat_params().data.add_(1.0)
    optim._step += 3
    for grp in optim.param_groups:
        grp['lr'] *= 0.5
    if everything:
        optim.ema.add_(1.0), optim._skipped_dev.add_(1), model.flat_grads(attach=True).add_(1.0)
        optim._ema_calls += 3
        optim._accum_phase = 2
    sd = model.state_dict_from(flat, layout=model_layout)
    _tree_equal(dict(sd), dict(model.state_dict_from(flat)))
    _tree_equal(dict(want_sd), dict(sd))
    assert list(sd) == list(want_sd) and getattr(sd, '_metadata', None) == getattr(want_sd, '_metadata', None)
    assert all(t.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for t in sd.values())     # views, not copies
    osd = optim.state_dict_from(m, v, optim.steps_at(cut, word), cut['param_groups'], layout=state_layout)
    _tree_equal(osd, optim.state_dict_from(m, v, optim.steps_at(cut, word), cut['param_groups']))
    _tree_equal(want_osd, osd)
    assert all(e['exp_avg'].untyped_storage().data_ptr() == m.untyped_storage().data_ptr() for e in osd['state'].values())
    assert optim.skipped_total_at(cut, word) == want_skipped == (3 if everything else 0)
    _tree_equal(want_win, optim.window_state_from(cut['window']['phase'], cut['window']['k'], grads))
    if everything:
        assert want_win['phase'] == 1 and want_win['grads'] is not None
        assert sorted({float(e['step']) for e in osd['state'].values()}) == [5.0, 6.0, 7.0]       # 9 - 4 frozen; 9 - 1 - 2 skipped; 9 - 2 skipped
        got = ema_entry_from(cut['ema']['decay'], optim.ema_updates_at(cut, word), optim.ema_state_dict_from(ema, sd, model._offsets))
        _tree_equal({k: (dict(x) if k == 'state_dict' else x) for k, x in want_ema.items()},
                    {k: (dict(x) if k == 'state_dict' else x) for k, x in got.items()})
        assert got['updates'] == 1 + 7 - (3 - 1)
    else:
        assert want_ema is None and want_win == {'phase': 0, 'k': 1, 'grads': None}
        assert optim.window_state_from(0, 1, torch.zeros(3))['grads'] is None                     # (no window open: no gradients kept)
    ck = checkpoint_dict(4, sd, osd, optim.group_names() if everything else None, want_ema, {'version': 1})
    assert list(ck) == ['epoch', 'state_dict', 'optimizer'] + (['param_group_names', 'ema'] if everything else []) + ['train_state']


def test_the_existing_methods_go_through_the_builders(monkeypatch):
    """state_dict(), ema_entry and window_state() of the live objects are the builders over the live buffers: one path"""
    from lirec_amd.optim import FusedAdam
    from lirec_amd.util import ema_entry
    model, optim = _optimiser(True)
    seen = []
    for cls, name in ((type(model), 'state_dict_from'), (FusedAdam, 'state_dict_from'), (FusedAdam, 'ema_state_dict_from'),
                      (FusedAdam, 'steps_at'), (FusedAdam, 'ema_updates_at')):
        real = getattr(cls, name)
        real = real.__func__ if hasattr(real, '__func__') else real

        def spy(*a, _real=real, _name=name, _cls=cls, **k):
            seen.append((_cls.__name__, _name))
            return _real(*a, **k)
        monkeypatch.setattr(cls, name, classmethod(spy) if name == 'steps_at' else
                            (staticmethod(spy) if name in ('ema_updates_at', 'ema_state_dict_from') else spy))
    monkeypatch.setattr(FusedAdam, 'window_state_from', staticmethod(lambda *a: seen.append(('FusedAdam', 'window_state_from')) or {}))
    model.state_dict(), optim.state_dict(), ema_entry(optim), optim.window_state()
    assert {n for _, n in seen} == {'state_dict_from', 'ema_state_dict_from', 'steps_at', 'ema_updates_at', 'window_state_from'}
    assert (type(model).__name__, 'state_dict_from') in seen and ('FusedAdam', 'state_dict_from') in seen


def test_capture_without_device_reads_leaves_the_two_device_fields_open(tmp_path):
    from test_host_resume import _state
    full = _state(tmp_path)[0].as_dict()
    held = _state(tmp_path, device_reads=False)[0].as_dict()
    assert list(full) == list(held) and held['skipped_total'] is None and held['window'] is None
    assert full['skipped_total'] == 0 and {k for k in full if full[k] is None and k not in ('scheduler', 'window')} == set()
    assert held['fingerprint'] == full['fingerprint'] and held['steps_taken'] == full['steps_taken']


# ---------------------------------------------------------------------------------------------------------------------------
# training(): off is off
# ---------------------------------------------------------------------------------------------------------------------------
def _forbid(monkeypatch):
    from lirec_amd import train, util
    made = []

    def refuse(*a, **k):
        made.append(a)
        raise AssertionError('an AsyncCheckpointer was made / a snapshot was issued')
    monkeypatch.setattr(train, 'AsyncCheckpointer', refuse)
    monkeypatch.setattr(util, 'AsyncCheckpointer', refuse)
    monkeypatch.setattr(ops, 'snapshot', refuse)
    return made


def _run(tmp_path, **over):
    from lirec_amd.train import training
    from test_parallel_cpu import _train_setup
    mk, model, loss, optim = _train_setup(str(tmp_path))
    opt.set(batch_size=4, epochs=2, save_model=False, **over)
    torch.manual_seed(7)
    before = threading.active_count()
    training(mk(18, 1), model=model, loss=loss, optimizer=optim, val_dataset=mk(10, 2))
    assert threading.active_count() == before
    return dict(training.last), model


def test_the_default_and_the_loop_field():
    from lirec_amd.train import _LOOP_FIELDS
    assert opt.checkpoint_async is False and 'checkpoint_async' in _LOOP_FIELDS


def test_flag_off_makes_no_checkpointer_and_issues_no_snapshot(monkeypatch, tmp_path):
    made = _forbid(monkeypatch)
    last, _ = _run(tmp_path, checkpoint_every=2)
    assert not made and (tmp_path / 'last.pth.tar').exists()
    assert not {'checkpoint_writes', 'checkpoint_waits', 'checkpoint_save_s'} & set(last)
    assert not [f for f in tmp_path.iterdir() if '.tmp.' in f.name]


def test_with_no_rolling_file_the_flag_is_inert(monkeypatch, tmp_path):
    made = _forbid(monkeypatch)
    last, a = _run(tmp_path / 'on', checkpoint_every=0, checkpoint_async=True)
    assert not made and not (tmp_path / 'on' / 'last.pth.tar').exists()
    assert not {'checkpoint_writes', 'checkpoint_waits', 'checkpoint_save_s'} & set(last)
    config.reset()
    _, b = _run(tmp_path / 'off', checkpoint_every=0)
    assert torch.equal(a.w, b.w)


def test_the_flag_on_reaches_the_checkpointer_and_is_drained_whatever_ends_the_loop(monkeypatch, tmp_path):
    """with a rolling file due, the flag makes ONE checkpointer, hands it every rolling write with a train state whose device
    fields are left open, and closes it in the loop's ``finally`` -- also when a step raises"""
    from lirec_amd import train
    log = []

    class Fake:
        stats = {'writes': 0, 'waits': 0, 'save_s': 0.0}

        def __init__(self, model, optimizer):
            log.append('made')

        def save(self, path, epoch, train_state=None):
            assert train_state['skipped_total'] is None and train_state['window'] is None and train_state['version'] == 1
            log.append(('save', train_state['epoch'], train_state['batches_done']))
            self.stats['writes'] += 1

        def close(self):
            log.append('closed')
    monkeypatch.setattr(train, 'AsyncCheckpointer', Fake)
    last, _ = _run(tmp_path, checkpoint_every=2, checkpoint_async=True)
    assert log[0] == 'made' and log[-1] == 'closed' and log.count('made') == 1 and log.count('closed') == 1
    assert [x for x in log if isinstance(x, tuple)] == [('save', 0, 2), ('save', 0, 4), ('save', 1, 0),
                                                          ('save', 1, 2), ('save', 1, 4), ('save', 2, 0)]
    assert last['checkpoint_writes'] == 6 and last['checkpoint_waits'] == 0 and last['checkpoint_save_s'] == 0.0
    del log[:]
    Fake.stats = {'writes': 0, 'waits': 0, 'save_s': 0.0}
    real = train._Stepper.step

    def third_raises(self, i, batch, _n=[0]):
        _n[0] += 1
        if _n[0] == 3:
            raise KeyError('stop')
        return real(self, i, batch)
    monkeypatch.setattr(train._Stepper, 'step', third_raises)
    config.reset()
    with pytest.raises(KeyError):
        _run(tmp_path / 'b', checkpoint_every=2, checkpoint_async=True)
    assert log == ['made', ('save', 0, 2), 'closed']


def test_the_checkpointer_refuses_what_it_cannot_snapshot(tmp_path):
    from lirec_amd.util import AsyncCheckpointer
    from test_parallel_cpu import _train_setup
    mk, model, loss, optim = _train_setup(str(tmp_path))
    with pytest.raises(TypeError, match='FusedAdam'):
        AsyncCheckpointer(model, optim)
