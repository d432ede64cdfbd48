"""The recorded train step over resident block-store batches (``opt.record_block_store`` = 'bind' / 'list'; lirec_collate_fields_at).
The criterion is BIT IDENTITY with the eager loop over the same store (``opt.record_block_store = ''``): ``torch.equal`` on
parameters, Adam's moments, per-clip losses and the printed epoch losses; the new launch against ``torch.index_select`` byte for
byte.  Shapes are those of tests/test_gpu_blockstore.py: 24 samples of the real feature width, batches of 5 (a short last batch every
epoch: release, eager step, resume)."""
import numpy as np
import pytest
import torch

from lirec_amd import _lib, blockstore as BS, config, ops, train
from lirec_amd.config import opt
from lirec_amd.data import SyntheticMixedFeaturesDataset
from lirec_amd.loader import BlockLoader
from oracle import lirec_oracle as O

pytestmark = pytest.mark.gpu
MODES = ('', 'bind', 'list')
RECIPES = {'int_rels': (dict(R=18), 18), 'modalties': ({}, 0), 'int_ch': (dict(T=7), 0)}


def _model(recipe, R, **over):
    from lirec_amd import model as M
    config.recipe(recipe, dropout=0.3, dropout_seed=77, **({} if recipe == 'modalties' else {'rels_n_clips': R}), **over)
    opt.device = 'cuda'
    opt.layer1_planes = True
    opt.compact_ctx_rows = True
    torch.manual_seed(11)                  # (modalties keeps create_model's initial parameters: the same ones in every run)
    model, loss, optim = M.create_model(101, n_rels=15)
    if recipe != 'modalties':
        cfg = O.OracleCfg(tr_maximize=recipe != 'int_rels', ctx=0 if recipe == 'int_ch' else 1, gates=0 if recipe == 'int_ch' else 1,
                          rels_multitask=recipe != 'int_ch')
        model.load_state_dict(O.fill_params(O.param_shapes(cfg, 101, 15 if recipe != 'int_ch' else 0), 5), strict=True)
    return model, loss, optim


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the launch
# ---------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 4, 8, 16, 24)          # bytes a row: every move width; 24 = 16 + 8 is no multiple of 16 (8-byte moves)


@pytest.mark.parametrize('B', [1, 5, 64])
def test_collate_fields_at_bytes_equal_index_select(B):
    """cursor 0, an odd offset and the last B ids of the buffer, duplicate ids among them; the cursor is moved by the launch behind
    (lirec_counter_add) and by nothing else; the 256-byte padding between the fields keeps its sentinel"""
    N, n_ids = 37, 3 * 64 + 7
    g = torch.Generator().manual_seed(2)
    ids_host = torch.randint(0, N, (n_ids,), generator=g, dtype=torch.int32)
    ids_host[:4] = torch.tensor([36, 0, 5, 5], dtype=torch.int32)           # the last row, the first, a duplicate
    ids_base = ids_host.cuda()
    tabs = [torch.randint(0, 256, (N, rb), dtype=torch.uint8, generator=g).cuda() for rb in WIDTHS]
    for cur in (0, 3, n_ids - B):
        cursor = torch.tensor([cur, -1], dtype=torch.int64, device='cuda')
        blob = torch.full((1 << 14,), 0xA5, dtype=torch.uint8, device='cuda')
        pairs, spans, at = [], [], 0
        for src, rb in zip(tabs, WIDTHS):
            at = (at + 255) // 256 * 256
            pairs.append((src, blob[at:at + B * rb].view(B, rb)))
            spans.append((at, B * rb, src))
            at += B * rb
        ops.collate_fields_at(ids_base, cursor, B, pairs)
        torch.cuda.synchronize()
        assert cursor.tolist() == [cur, -1]                                 # the collate launch does not move it
        ops.counter_add(cursor, [B])
        torch.cuda.synchronize()
        assert cursor.tolist() == [cur + B, -1]
        want = torch.full_like(blob, 0xA5)
        take = ids_base[cur:cur + B].long()
        for at, n, src in spans:
            want[at:at + n] = src.index_select(0, take).reshape(-1)
        assert torch.equal(blob, want), (B, cur)                            # the rows, and not a byte beside them
    # a misaligned destination takes the narrower moves: the same bytes
    blob = torch.full((4096,), 0xA5, dtype=torch.uint8, device='cuda')
    cursor = torch.tensor([3], dtype=torch.int64, device='cuda')
    ops.collate_fields_at(ids_base, cursor, B, [(tabs[5], blob[4:4 + B * 24].view(B, 24))])
    assert torch.equal(blob[4:4 + B * 24], tabs[5].index_select(0, ids_base[3:3 + B].long()).reshape(-1))
    assert bool((blob[:4] == 0xA5).all()) and bool((blob[4 + B * 24:] == 0xA5).all())


def test_collate_fields_at_refuses_seventeen_fields():
    ids_base = torch.zeros(8, dtype=torch.int32, device='cuda')
    cursor = torch.zeros(1, dtype=torch.int64, device='cuda')
    src = torch.zeros(4, 8, dtype=torch.uint8, device='cuda')
    dsts = [torch.full((2, 8), 7, dtype=torch.uint8, device='cuda') for _ in range(17)]
    arr = (_lib.CollateField * 17)()
    for f, d in enumerate(dsts):
        arr[f].src, arr[f].row_bytes, arr[f].dst = src.data_ptr(), 8, d.data_ptr()
    rc = _lib.lib().lirec_collate_fields_at(ids_base.data_ptr(), cursor.data_ptr(), 2, arr, 17, None)
    torch.cuda.synchronize()
    assert rc == _lib.LIREC_EINVAL and all(bool((d == 7).all()) for d in dsts) and int(cursor) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. - 4. training() under the three values of the flag
# ---------------------------------------------------------------------------------------------------------------------------
class _UpdatingSampler(torch.utils.data.Sampler):
    """a shuffled sampler with a fixed generator seed; ``between`` runs in front of the second epoch's draw"""

    def __init__(self, n, between=None):
        self.n, self.g, self.between, self.epochs = n, torch.Generator().manual_seed(123), between, 0

    def __len__(self):
        return self.n

    def __iter__(self):
        if self.epochs == 1 and self.between is not None:
            self.between()
        self.epochs += 1
        return iter(torch.randperm(self.n, generator=self.g).tolist())


_STEP = train._Stepper.step


class _ClipLabels(SyntheticMixedFeaturesDataset):
    """one interaction label per clip, what MultiTaskCrossEntropyLoss reads (mlp/model.py:371)"""

    def __getitem__(self, idx):
        s = dict(super().__getitem__(idx))
        s['labels'] = np.asarray(s['labels']).reshape(-1)[0]
        return s


def _train(monkeypatch, tmp_path, mode, recipe='int_rels', weights=False, update=False, ce=False):
    """training() for 3 epochs over the store under ``opt.record_block_store = mode``: everything the modes are compared on"""
    kw, R = RECIPES[recipe]
    model, loss, optim = _model(recipe, R, batch_size=5, num_workers=0, epochs=3, test_fr=1000, store_root=str(tmp_path),
                                save_model=False, record_block_store=mode, use_ce_loss=ce)
    ds = BS.ResidentBlockDataset((_ClipLabels if ce else SyntheticMixedFeaturesDataset)(recipe, 24, seed=31, soft_gt=opt.soft_gt, **kw))
    if ce:
        # (the periodic evaluation counts track-level hits from per-track labels: not what this loss's batches carry)
        monkeypatch.setattr(train, '_evaluate_and_keep', lambda *a, **k: None)
    if weights:
        ds.set_clip_weights(np.linspace(0.25, 2.0, 24))
        loss.keep_clip_losses = True
    between = None
    if update:
        new = torch.from_numpy(np.random.default_rng(9).standard_normal((2,) + ds.block_store.feature_shape))
        between = lambda: ds.update([23, 4], new)
    lines, clip, rec = [], [], {}
    monkeypatch.setattr(train, '_print', lambda *a, **k: lines.append(' '.join(str(x) for x in a)))

    def noting(self, i, batch):
        before = self.stats['replays']
        out = _STEP(self, i, batch)
        if weights:
            if self.recorded is not None and 'buf' not in rec:
                rec['buf'] = self.loss.last_clip_losses          # (the recording step's: every replay writes it again)
            clip.append((rec['buf'] if self.stats['replays'] > before else self.loss.last_clip_losses).clone())
        return out
    monkeypatch.setattr(train._Stepper, 'step', noting)
    train.training(ds, model=model, loss=loss, optimizer=optim, sampler=_UpdatingSampler(24, between))
    torch.cuda.synchronize()
    last = train.training.last
    return {'params': model.flat_params().clone(), 'm': optim._m.clone(), 'v': optim._v.clone(),
            'losses': [l for l in lines if l.startswith('loss: ')], 'clip': clip, 'replays': last['replays'],
            'copies': last['input_copies'], 'loader': last['loader'], 'said': [l for l in lines if 'not used' in l]}


def _compare(runs, with_clip=False, list_draws=True):
    """three epochs of five batches, the last one short: epoch 0 steps eagerly on three and records on the fourth; epochs 1 and 2
    replay four each, so the cursor is written at an epoch's start both behind a short batch alone and behind in-list batches and a
    short batch.  ``list_draws`` False: 'list' was expected to record as 'bind' does."""
    ref = runs['']
    assert isinstance(ref['loader'], BlockLoader) and ref['replays'] == 0 and ref['loader'].n_collate == 15 and ref['loader'].n_in_list == 0
    assert len(ref['losses']) == 3 and torch.isfinite(ref['params']).all()
    for mode in ('bind', 'list'):
        r, ld = runs[mode], runs[mode]['loader']
        assert not r['said'], r['said']
        assert r['replays'] == 8 and r['copies'] == 0, (mode, r['replays'], r['copies'])
        if mode == 'bind' or not list_draws:
            assert ld.n_in_place == 8 and ld.n_collate == 15 and ld.n_in_list == 0
        else:
            assert ld.n_in_list == 8 and ld.n_collate == 7 and ld.n_in_place == 0      # (the eager interludes alone are collated by the host's call)
        for k in ('params', 'm', 'v'):
            assert torch.equal(r[k], ref[k]), (mode, k, int((r[k] != ref[k]).sum()))
        assert r['losses'] == ref['losses'], (mode, r['losses'], ref['losses'])
        if with_clip:
            assert len(r['clip']) == len(ref['clip']) == 15
            for i, (a, b) in enumerate(zip(r['clip'], ref['clip'])):
                assert torch.equal(a, b), (mode, 'per-clip losses of step', i)


def test_cross_entropy_loss_is_bit_identical_under_the_three_modes(monkeypatch, tmp_path):
    """``opt.use_ce_loss``: the loss converts the batch's labels to int32 on the host's side in front of every replay
    (``before_replay``) -- before a list would have drawn the batch -- so 'list' records as 'bind' does: the loader's call writes
    the batch, then the labels are converted, then the list runs"""
    from lirec_amd.graph import RecordedTrainStep
    runs = {mode: _train(monkeypatch, tmp_path, mode, ce=True) for mode in MODES}
    _compare(runs, list_draws=False)
    margin = _train(monkeypatch, tmp_path, '')
    assert not torch.equal(margin['params'], runs['']['params']), 'the other loss was meant to run'
    # asked for directly, the in-list draw under such a loss is refused before anything is recorded
    model, loss, optim = _model('int_rels', 18, use_ce_loss=True)
    model.train()
    loader = BlockLoader(BS.ResidentBlockDataset(_ClipLabels('int_rels', 24, seed=31, R=18)), batch_size=5)
    batch = _bound_batch(loader, [3, 20, 7, 7, 0])
    _eager_step(model, loss, optim, batch)
    assert loss.needs_before_replay()
    with pytest.raises(_lib.LirecError, match='before_replay'):
        RecordedTrainStep(model, loss, optim, batch, warmup=0, draw=lambda: None)
    assert model._seed_dev is None and optim._step_dev is None


@pytest.mark.parametrize('recipe', sorted(RECIPES))
def test_training_is_bit_identical_under_the_three_modes(monkeypatch, tmp_path, recipe):
    _compare({mode: _train(monkeypatch, tmp_path, mode, recipe) for mode in MODES})


def test_training_with_clip_weights_and_kept_clip_losses(monkeypatch, tmp_path):
    runs = {mode: _train(monkeypatch, tmp_path, mode, weights=True) for mode in MODES}
    _compare(runs, with_clip=True)
    plain = _train(monkeypatch, tmp_path, '')
    assert not torch.equal(plain['params'], runs['']['params']), 'the weights were meant to matter'


def test_store_update_between_two_epochs_of_a_recorded_run(monkeypatch, tmp_path):
    runs = {mode: _train(monkeypatch, tmp_path, mode, update=True) for mode in MODES}
    _compare(runs)
    plain = _train(monkeypatch, tmp_path, '')
    assert not torch.equal(plain['params'], runs['']['params']), 'the update was meant to matter'


# ---------------------------------------------------------------------------------------------------------------------------
# 5. - 7. RecordedTrainStep on block-store batches
# ---------------------------------------------------------------------------------------------------------------------------
def _store(n=24):
    return BS.ResidentBlockDataset(SyntheticMixedFeaturesDataset('int_rels', n, seed=31, R=18))


def _bound_batch(loader, ids):
    """a batch in a buffer of its own that later ``collate_ids`` calls of the same size can be bound to"""
    layout, nbytes = loader.layout(len(ids))
    blob = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    loader.bind(layout, blob)
    return loader.collate_ids(torch.tensor(ids, dtype=torch.int32, device='cuda'), len(ids))


def _eager_step(model, loss, optim, batch):
    optim.zero_grad()
    lv = loss(model(dict(batch)), batch)
    lv.backward()
    optim.step()


def test_replay_under_other_flags_raises_and_launches_nothing():
    from lirec_amd.graph import RecordedTrainStep
    model, loss, optim = _model('int_rels', 18)
    model.train()
    loader = BlockLoader(_store(), batch_size=5)
    batch = _bound_batch(loader, [3, 20, 7, 7, 0])
    g = RecordedTrainStep(model, loss, optim, batch, warmup=0)
    g.step()
    torch.cuda.synchronize()

    def refused():
        ops.CommandList.begin()
        try:
            with pytest.raises(RuntimeError):
                g.step()
        finally:
            cl = ops.CommandList.end()
        n = cl.size
        cl.destroy()
        assert n == 0, 'a refused replay launched %d commands' % n

    mode = ops.get_gemm_mode()
    try:
        for m in (0, 1, 3):
            ops.set_gemm_mode(m)
            refused()
    finally:
        ops.set_gemm_mode(mode)
    opt.layer1_planes = False
    try:
        refused()
    finally:
        opt.layer1_planes = True
    calls = model._fwd_train_calls
    g.step()                                          # everything set back: the list is valid again
    torch.cuda.synchronize()
    assert model._fwd_train_calls == calls + 1
    g.release()


def test_clip_ids_outside_the_batch_buffer_are_refused():
    from lirec_amd.graph import RecordedTrainStep
    model, loss, optim = _model('int_rels', 18)
    model.train()
    ds = _store()
    loader = BlockLoader(ds, batch_size=5)
    batch = _bound_batch(loader, [3, 20, 7, 7, 0])
    loose = dict(batch)
    loose['features'] = ds.block_store.features_of(batch['features'].clip_ids.clone(), 5)
    other = _bound_batch(loader, [23, 1, 2, 9, 9])
    calls, steps = model._fwd_train_calls, optim._step
    ops.CommandList.begin()
    try:
        with pytest.raises(_lib.LirecError, match='clip_ids'):
            RecordedTrainStep(model, loss, optim, loose, warmup=0)
        # the input-pipeline form is not built over block-store batches: refused the same way
        with pytest.raises(_lib.LirecError, match='next_batch'):
            RecordedTrainStep(model, loss, optim, batch, warmup=0, next_batch=other)
    finally:
        cl = ops.CommandList.end()
    n = cl.size
    cl.destroy()
    assert n == 0
    # as release() leaves it: the counters by value, no deferral, nothing counted
    assert model._seed_dev is None and optim._step_dev is None and model.lanes.step_side_dev is None and not model.lanes.defer_join
    assert (model._fwd_train_calls, optim._step) == (calls, steps)
    _eager_step(model, loss, optim, batch)            # the eager step still runs
    torch.cuda.synchronize()
    assert torch.isfinite(model.flat_params()).all()
