"""lirec_collate_resident, lirec_amd.loader.ResidentLoader and opt.device_collate on the GPU.  Everything is exact: the expected
side is ``features._dedup`` / ``features.collate`` + ``batch_to_device`` (tests/collate_cases.py), never a run of the kernel, and
every comparison is equality of every element."""
import numpy as np
import pytest
import torch

import collate_cases as CC
from lirec_amd import features as F
from lirec_amd import ops

pytestmark = pytest.mark.gpu
R = 18
GUARD = 64                                      # bytes behind every output, to be found untouched

_expected = {}


def expected(name):
    if name not in _expected:
        _expected[name] = CC.expected(CC.CASES[name])
    return _expected[name]


class Run:
    """one case's device inputs and outputs (the field destinations back to back in one buffer); ``go`` issues the call"""

    def __init__(self, case, workspace=None):
        dev = 'cuda'
        self.case, B, E = case, case['B'], case['E']
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.ids, self.rows = up(case['ids']), up(case['index_rows'])
        self.n_c, self.n_t = CC.list_lengths(B, E, case['n_clip_all'], case['n_track_all'])
        self.srcs = [up(f) for f in case['fields']]
        self.ws = ops.collate_workspace(case['n_clip_all'], case['n_track_all'], dev) if workspace is None else workspace
        assert self.ws.numel() >= CC.workspace_bytes(case['n_clip_all'], case['n_track_all'])
        self.reset()

    def reset(self):
        """outputs of sentinels with a guard behind each; (a fresh workspace is garbage: the caller promises nothing)"""
        B, E = self.case['B'], self.case['E']
        g = GUARD // 4
        i32 = lambda n: torch.full((n + g,), -77, dtype=torch.int32, device='cuda')
        self.fi, self.cr, self.tr, self.cnt = i32(B * E * 3), i32(self.n_c), i32(self.n_t), i32(2)
        total = sum(B * rb for rb in CC.FIELD_BYTES)
        self.fbuf = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device='cuda')
        self.dsts, at = [], 0
        for rb in CC.FIELD_BYTES:
            self.dsts.append(self.fbuf[at:at + B * rb].view(B, rb))
            at += B * rb

    def go(self):
        B, E, g = self.case['B'], self.case['E'], GUARD // 4
        ops.collate_resident(self.ids, self.rows, self.case['n_clip_all'], self.case['n_track_all'], self.fi[:-g].view(B, E, 3),
                             self.cr[:-g], self.tr[:-g], self.cnt[:-g], list(zip(self.srcs, self.dsts)), self.ws)

    def check(self, want, what):
        g = GUARD // 4
        for k, t in (('feature_index', self.fi), ('clip_rows', self.cr), ('track_rows', self.tr), ('counts', self.cnt)):
            got = t.cpu().numpy()
            assert (got[-g:] == -77).all(), (what, k, 'written past its end')
            assert np.array_equal(got[:-g].reshape(want[k].shape), want[k]), (what, k)
        fb = self.fbuf.cpu().numpy()
        assert (fb[-GUARD:] == 0xAB).all(), (what, 'fields written past their end')
        for f, (d, w) in enumerate(zip(self.dsts, want['fields'])):
            assert np.array_equal(d.cpu().numpy(), w), (what, 'field', CC.FIELD_BYTES[f])


@pytest.mark.parametrize('name', sorted(CC.CASES))
def test_every_case_through_the_c_abi(name):
    run = Run(CC.CASES[name])
    run.ws.fill_(0xFF)
    run.go()
    run.check(expected(name), name)


def test_two_batches_back_to_back_on_one_workspace_then_the_first_again():
    a, b = CC.CASES['real_T20_R18'], CC.CASES['n16384']
    need = max(CC.workspace_bytes(c['n_clip_all'], c['n_track_all']) for c in (a, b))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device='cuda')
    ra, rb, ra2 = Run(a, ws), Run(b, ws), Run(a, ws)
    ra.go()
    rb.go()
    ra2.go()                                                   # (nothing in between: one stream orders them)
    ra.check(expected('real_T20_R18'), 'first')
    rb.check(expected('n16384'), 'second')
    ra2.check(expected('real_T20_R18'), 'first again')
    # the same outputs written twice: the second call finds its own marks and ranks in the workspace
    ra.go()
    ra.check(expected('real_T20_R18'), 'written again')


def test_a_recorded_call_replays_to_the_same_bytes():
    run = Run(CC.CASES['n1025'])
    ops.CommandList.begin()
    run.go()
    cmds = ops.CommandList.end()
    assert cmds.size == 4
    run.check(expected('n1025'), 'recorded')
    g = GUARD // 4
    for t in (run.fi, run.cr, run.tr, run.cnt):                # the same buffers (their addresses are in the list), emptied
        t[:-g].fill_(-5)
    run.fbuf[:-GUARD].fill_(0)
    run.ws.fill_(0x5A)
    cmds.replay()
    run.check(expected('n1025'), 'replayed')
    cmds.destroy()


# ---- the loader -----------------------------------------------------------------------------------------------------------
def _same_batch(got, host, what):
    """a ResidentLoader batch against ``batch_to_device`` of the host batch ``host`` (+ the host batch's ``_layout``)"""
    want = dict(F.batch_to_device(host, 'cuda'), _layout=host['_layout'])
    assert 'piece_counts' in want and '_blob' not in want and '_slots' not in want
    assert set(got) == set(want) - {'piece_counts'}, (what, set(got) ^ set(want))
    for k, v in want.items():
        if k == 'piece_counts':
            continue
        if torch.is_tensor(v):
            if k == '_dev_blob':                               # (the bytes between the parts belong to nobody)
                assert got[k].shape == v.shape and got[k].dtype == v.dtype and got[k].is_cuda
                continue
            assert got[k].is_cuda and got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(got[k], v), (what, k)
        elif k == '_layout':
            assert tuple(got[k]) == tuple(v), what
        else:
            assert got[k] is v, (what, k)


def test_resident_loader_batches_equal_the_host_collate_and_threaded_loaders_order():
    from lirec_amd.loader import ResidentLoader, ThreadedLoader
    world = F.synthetic_world(31, n_scenes=6, per_scene=4)
    ds = F.PiecesDataset(world, R, resident=True)
    assert len(ds) % 5 != 0
    rl = ResidentLoader(ds, batch_size=5, shuffle=True, device='cuda')
    tl = ThreadedLoader(ds, batch_size=5, shuffle=True, num_workers=1, collate_fn=ds.collate_fn)
    for epoch in range(2):
        torch.manual_seed(40 + epoch)
        ids = rl.epoch_ids()
        torch.manual_seed(40 + epoch)
        got = list(rl)
        torch.manual_seed(40 + epoch)
        ref = list(tl)
        assert len(got) == len(ref) == len(ids) == len(rl) and len(ids[-1]) == len(ds) % 5
        for k, (g, r, idx) in enumerate(zip(got, ref, ids)):
            _same_batch(g, r, (epoch, k))                                           # ThreadedLoader's order, its values
            _same_batch(g, ds.collate_fn([ds[i] for i in idx]), (epoch, k, 'by ids'))
    assert rl.n_collate == 2 * len(rl) and rl.n_in_place == 0


# ---- the entry points -----------------------------------------------------------------------------------------------------
def _same_tree(a, b, what='state'):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), what
    elif isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same_tree(a[k], b[k], '%s.%s' % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, '%s[%d]' % (what, k))
    else:
        assert a == b, (what, a, b)


def test_training_with_the_flag_on_equals_the_flag_off_and_copies_nothing(tmp_path, capsys):
    """two epochs over a resident store, shuffled, batches of 5 (ten whole ones and a short one per epoch): the recorded step
    engages on the fourth batch either way.  Same seed -> the same parameters, Adam moments and printed epoch losses bit for bit;
    with the flag on every replayed batch was written into the step's input buffer by its collate call and nothing was copied."""
    from lirec_amd import config
    from lirec_amd.config import opt
    from lirec_amd.loader import ResidentLoader, ThreadedLoader
    from lirec_amd.train import training
    from test_pieces_entry import _fresh, _world
    world = _world(21, n_scenes=9, per_scene=6)                 # 54 clips
    res = {}
    try:
        for flag in (True, False):
            model, loss, optim = _fresh(world)
            opt.store_root = str(tmp_path / str(flag))
            opt.batch_size, opt.num_workers, opt.epochs, opt.device_collate = 5, 1, 2, flag
            optim.param_groups[0]['lr'] = 1e-3
            ds = F.PiecesDataset(world, R, resident=True)
            val = F.PiecesDataset(_world(8), R, n_classes=ds.n_classes, resident=True)
            torch.manual_seed(99)
            training(ds, model=model, loss=loss, optimizer=optim, val_dataset=val)
            torch.cuda.synchronize()
            printed = capsys.readouterr().out
            assert 'recorded train step not used' not in printed, printed
            losses = [float(l.split('loss:')[1]) for l in printed.splitlines() if l.startswith('loss:')]
            last = dict(training.last)
            res[flag] = (model.flat_params().detach().cpu().clone(), optim.state_dict(), losses, last, optim._step)
        steps = 2 * ((len(ds) + 4) // 5)
        on, off = res[True], res[False]
        assert len(on[2]) == len(off[2]) == 2 and on[2] == off[2], (on[2], off[2])
        assert on[4] == off[4] == steps
        assert torch.equal(on[0].view(torch.int32), off[0].view(torch.int32))
        _same_tree(on[1], off[1], 'optimizer')
        # the recorded branch: 11 batches an epoch, three eager + the recording, then replays; the short batch is eager
        replays = (10 - 4) + 10
        assert isinstance(on[3]['loader'], ResidentLoader) and isinstance(off[3]['loader'], ThreadedLoader)
        assert on[3]['replays'] == off[3]['replays'] == replays
        assert off[3]['input_copies'] == replays and on[3]['input_copies'] == 0
        assert on[3]['loader'].n_collate == steps and on[3]['loader'].n_in_place == replays
    finally:
        config.reset()


def _eval_both_ways(ds, model, loss):
    import lirec_amd
    from lirec_amd.config import opt
    from lirec_amd.test import testing
    out = {}
    for flag in (False, True):
        opt.device_collate = flag
        res = testing(ds, model, loss, mode='test', verbose=False)
        last = dict(testing.last)
        prec = {k: v for k, v in vars(last['precision']).items() if isinstance(v, (int, float))}
        pred = lirec_amd.predict(ds, model, top_k=5)
        out[flag] = (res, prec, last['loss'], last['n_clips'], np.array(last['conf_mat']), last['metrics_on_device'],
                     {k: getattr(pred, k) for k in pred.fields}, pred.n_clips, pred.pairs)
    a, b = out[False], out[True]
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]
    assert a[7] == b[7] == len(ds) and a[1]['total'] > 0
    for k in a[6]:
        assert (a[6][k] is None) == (b[6][k] is None), k
        assert a[6][k] is None or (a[6][k].dtype == b[6][k].dtype and np.array_equal(a[6][k], b[6][k], equal_nan=True)), k
    assert (a[8] is None) == (b[8] is None)
    if a[8] is not None:
        assert list(a[8]) == list(b[8]) and all(np.array_equal(a[8][h][1], b[8][h][1]) for h in a[8])
    return out


def test_testing_and_predict_are_the_same_with_the_flag_on_int_rel_ch():
    from lirec_amd import config
    from lirec_amd.config import opt
    from lirec_amd import loader as LD
    from test_pieces_entry import _fresh, _world
    world = _world(21, n_scenes=5, per_scene=5)
    try:
        model, loss, optim = _fresh(world)
        opt.batch_size = 4                                       # 25 clips: six batches of 4 and a single clip
        ds = F.PiecesDataset(world, R, resident=True)
        used = []
        real = LD.ResidentLoader.collate_ids
        LD.ResidentLoader.collate_ids = lambda self, ids, B: (used.append(B), real(self, ids, B))[1]
        try:
            _eval_both_ways(ds, model, loss)
        finally:
            LD.ResidentLoader.collate_ids = real
        assert used == [4] * 6 + [1] + [4] * 6 + [1], used       # testing() and predict() with the flag on, and only then
    finally:
        config.reset()


def test_testing_and_predict_are_the_same_with_the_flag_on_int_rels(tmp_path):
    """int_rels runs on the tiled block, not on a resident store: the flag falls back to the loader it had, without complaint"""
    from lirec_amd import config
    from test_gpu_loops import _setup
    try:
        mk, model, loss, optim = _setup('int_rels', tmp_path)
        _eval_both_ways(mk(23, 4), model, loss)
    finally:
        config.reset()
