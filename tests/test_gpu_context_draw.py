"""lirec_draw_context, ``ResidentLoader`` over a ``PiecesDataset(context_draw='random')`` and ``training()`` on one, on the GPU.
Everything is exact, and every expected side is the CPU statement of the rule (``features.draw_context``, itself held against an
independent restatement in tests/test_host_context_draw.py) or the host collate of a twin dataset -- never a run of the kernel."""
import numpy as np
import pytest
import torch

import context_draw_cases as DC
from lirec_amd import features as F
from lirec_amd import ops

pytestmark = pytest.mark.gpu
GUARD = 64                                      # int32 words behind the table, to be found untouched
SEED = 0x5eed00000007


class Run:
    """one case's tables on the device; the index table is filled with the sentinel, a guard of the same behind it"""

    def __init__(self, case):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.case = case
        self.dst, self.off, self.pool = up(case['slot_dst']), up(case['slot_off']), up(case['pool_rows'])
        self.shape = (case['N'], case['T'], case['R'] + 1, 3)
        self.buf = torch.empty(int(np.prod(self.shape)) + GUARD, dtype=torch.int32, device='cuda')
        self.table = self.buf[:-GUARD].view(self.shape)
        self.fill()

    def fill(self):
        self.buf.fill_(DC.SENTINEL)

    def go(self, seed, epoch):
        ops.draw_context(self.dst, self.off, self.pool, self.table, self.case['R'], seed, epoch)

    def check(self, seed, epoch, what):
        c = self.case
        want = F.draw_context(c['slot_dst'], c['slot_off'], c['pool_rows'], DC.sentinel_table(c), c['R'], seed, epoch)
        got = self.buf.cpu().numpy()
        assert (got[-GUARD:] == DC.SENTINEL).all(), (what, 'written past the table')
        got = got[:-GUARD].reshape(self.shape)
        outside = ~DC.slot_rows_mask(c)
        assert (got[outside] == DC.SENTINEL).all(), (what, 'an element outside rows 1 .. R of the slots was written')
        assert np.array_equal(got, want), what


@pytest.mark.parametrize('name,k', DC.RUNS)
def test_every_case_through_the_c_abi_and_twice_the_same(name, k):
    case = DC.CASES[name]
    seed, epoch = case['runs'][k]
    run = Run(case)
    run.go(seed, epoch)
    run.check(seed, epoch, name)
    run.go(seed, epoch)                                        # over its own output: the same bytes
    run.check(seed, epoch, (name, 'again'))


def test_successive_epochs_in_place_leave_the_last_epochs_draw():
    """what the loader does: the table is never restored between draws"""
    run = Run(DC.CASES['lengths_R18'])
    for epoch in (0, 1, 5):
        run.go(SEED, epoch)
    run.check(SEED, 5, 'third draw in place')


def test_a_recorded_call_replays_to_the_same_bytes():
    run = Run(DC.CASES['slots_300'])
    ops.CommandList.begin()
    run.go(SEED, 1 << 31)
    cmds = ops.CommandList.end()
    assert cmds.size == 1
    run.check(SEED, 1 << 31, 'recorded')
    run.fill()                                                 # the same buffer (its address is in the list), emptied
    cmds.replay()
    run.check(SEED, 1 << 31, 'replayed')
    cmds.destroy()


# ---- the loader -----------------------------------------------------------------------------------------------------------
def _same_batch(got, host, store, what):
    """a ResidentLoader batch against ``batch_to_device`` of the twin's host batch, key for key and bit for bit"""
    want = dict(F.batch_to_device(host, 'cuda'), _layout=host['_layout'])
    assert set(got) == set(want) - {'piece_counts'}, (what, set(got) ^ set(want))
    for k, v in want.items():
        if k in ('piece_counts', '_dev_blob'):                 # (the bytes between the parts of the buffer belong to nobody)
            continue
        if torch.is_tensor(v):
            assert got[k].is_cuda and got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(got[k], v), (what, k)
        elif k == '_layout':
            assert tuple(got[k]) == tuple(v), what
        else:
            assert k == 'piece_store' and got[k] is store, (what, k)


def test_resident_loader_batches_equal_the_host_collate_of_a_twin_at_every_epoch():
    from lirec_amd.loader import ResidentLoader
    world = F.synthetic_world(**DC.WORLD)
    mk = lambda: F.PiecesDataset(world, DC.WORLD_R, resident=True, context_draw='random', context_seed=SEED)
    ds, twin = mk(), mk()
    assert len(ds) == 72 and ds.slot_dst.size >= 10
    rl = ResidentLoader(ds, batch_size=16, device='cuda')
    first = {}
    for epoch in (0, 1, 2):
        ds.epoch = twin.epoch = epoch
        got, ids = list(rl), rl.epoch_ids()
        assert [len(i) for i in ids] == [16, 16, 16, 16, 8] and len(got) == 5
        for k, (g, idx) in enumerate(zip(got, ids)):
            _same_batch(g, twin.collate_fn([twin[i] for i in idx]), ds.store, (epoch, k))
        first[epoch] = got[0]['feature_index'].clone()
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])
    assert rl.n_draw == 3 and ds.device_tables('cuda')['drawn_epoch'] == 2
    list(rl)                                                   # the same epoch again, and another loader over the dataset: no launch
    other = ResidentLoader(ds, batch_size=7, device='cuda')
    list(other)
    assert rl.n_draw == 3 and other.n_draw == 0
    # bound: a batch of the bound layout is written into the bound buffer, and holds the epoch's draw
    ds.epoch = twin.epoch = 3
    layout, nbytes = rl.layout(16)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    rl.bind(layout, blob)
    before = rl.n_in_place
    for k, (g, idx) in enumerate(zip(rl, rl.epoch_ids())):     # (checked batch by batch: the next one overwrites the buffer)
        assert (g['_dev_blob'] is blob) == (len(idx) == 16)
        _same_batch(g, twin.collate_fn([twin[i] for i in idx]), ds.store, ('bound', k))
        if len(idx) == 16:
            assert torch.equal(F.layout_views(blob, layout)['feature_index'], g['feature_index'])
            assert g['feature_index'].data_ptr() == blob.data_ptr()
    rl.unbind()
    assert rl.n_in_place == before + 4 and rl.n_draw == 4


# ---- the entry point ------------------------------------------------------------------------------------------------------
def test_training_on_a_random_dataset_is_the_same_with_device_collate_on_and_off_and_differs_from_strided(tmp_path, capsys):
    """the model and flags of tests/test_gpu_collate.py's training test; three epochs, shuffled, batches of 5 over 54 clips whose
    world has 42 over-long lists at R = 18.  Device collate on (the index redrawn on the device, batches written into the recorded
    step's inputs) and off (the draw made on the host, loader threads): the same parameters and Adam moments bit for bit, with
    replays in both; the strided dataset trains to other parameters."""
    from lirec_amd import config
    from lirec_amd.config import opt
    from lirec_amd.loader import ResidentLoader, ThreadedLoader
    from lirec_amd.train import training
    from test_gpu_collate import _same_tree
    from test_pieces_entry import R, _fresh, _world
    world = _world(3, n_scenes=9, per_scene=6, n_chars=3, n_rel_names=2)
    res = {}
    try:
        for name, flag, draw in (('on', True, 'random'), ('off', False, 'random'), ('strided', True, 'strided')):
            model, loss, optim = _fresh(world)
            opt.store_root = str(tmp_path / name)
            opt.batch_size, opt.num_workers, opt.epochs, opt.device_collate = 5, 1, 3, flag
            optim.param_groups[0]['lr'] = 1e-3
            ds = F.PiecesDataset(world, R, resident=True, context_draw=draw, context_seed=SEED)
            val = F.PiecesDataset(_world(8), R, n_classes=ds.n_classes, resident=True)
            torch.manual_seed(99)
            training(ds, model=model, loss=loss, optimizer=optim, val_dataset=val)
            torch.cuda.synchronize()
            printed = capsys.readouterr().out
            assert 'recorded train step not used' not in printed, printed
            res[name] = (model.flat_params().detach().cpu().clone(), optim.state_dict(), dict(training.last), optim._step)
        assert len(ds) == 54
        on, off, st = res['on'], res['off'], res['strided']
        assert isinstance(on[2]['loader'], ResidentLoader) and isinstance(off[2]['loader'], ThreadedLoader)
        assert on[3] == off[3] == st[3] == 3 * 11
        assert on[2]['replays'] == off[2]['replays'] >= 1 and on[2]['input_copies'] == 0
        # one draw launch per epoch from the training loader; the evaluation of the train set after each epoch reads the same draw
        assert on[2]['loader'].n_draw == 3 and st[2]['loader'].n_draw == 0
        assert torch.equal(on[0].view(torch.int32), off[0].view(torch.int32))
        _same_tree(on[1], off[1], 'optimizer')
        assert not torch.equal(on[0].view(torch.int32), st[0].view(torch.int32))
    finally:
        config.reset()
