"""The recorded evaluation and prediction steps over a resident block store (``opt.record_eval``; lirec_amd.graph.RecordedEvalStep).
The criterion is BIT IDENTITY with the eager loop over the same store (the flag off): the returned dicts, every counter, the
confusion matrix, the loss and the per-pair relationship sums of ``testing()``; every field of ``predict()``; the three new launches
against the launches they stand for (``lirec_predict_clips`` into a slice, a torch row copy, torch's ``+=``), with a sentinel
outside the rows they own.  Stores are those of tests/test_gpu_blockstore_recorded.py: the real feature width, 24 / 25 clips in
batches of 5 (a short tail of 4), 6 (no tail) and 6 again over 25 (a singleton tail, which ``testing()`` skips)."""
import numpy as np
import pytest
import torch

from lirec_amd import _lib, blockstore as BS, config, ops
from lirec_amd.config import opt
from lirec_amd.data import SyntheticMixedFeaturesDataset
from lirec_amd.loader import BlockLoader
from lirec_amd.predict import predict
from lirec_amd.test import testing as evaluate
from oracle import lirec_oracle as O

pytestmark = pytest.mark.gpu
RECIPES = ('modalties', 'int_rels', 'int_ch')
SHAPES = ((24, 5), (24, 6), (25, 6))                 # (clips, batch): a short tail of 4, no tail, a singleton tail


def _model(recipe, **over):
    from lirec_amd import model as M
    config.recipe(recipe, dropout=0.3, dropout_seed=77, num_workers=0, **({} if recipe == 'modalties' else {'rels_n_clips': 18}), **over)
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


_STORES = {}


def _store(recipe, n, cls=SyntheticMixedFeaturesDataset):
    """the resident store of (recipe, n): made once, shared by the tests, never written"""
    key = (recipe, n, cls.__name__)
    if key not in _STORES:
        _STORES[key] = BS.ResidentBlockDataset(cls(recipe, n, seed=31, soft_gt=recipe == 'modalties', R=18))
    return _STORES[key]


def _full(n, bs):
    return n // bs


def _testing_result(model, loss, ds):
    out = evaluate(ds, model, loss, verbose=False)
    torch.cuda.synchronize()
    last = evaluate.last
    rel = last['relationships']
    return {'out': out, 'counters': last['precision'].counters(), 'conf': np.array(last['conf_mat']), 'loss': float(last['loss']),
            'n_clips': last['n_clips'], 'pairs': None if rel is None else {h: (np.array(s), rel._gt[h]) for h, s in rel._scores.items()},
            'recorded': last['recorded_steps']}


def _assert_same_evaluation(on, off):
    assert on['out'] == off['out'] and on['counters'] == off['counters'] and on['n_clips'] == off['n_clips']
    assert np.array_equal(on['conf'], off['conf']) and on['loss'] == off['loss'] and np.isfinite(off['loss'])
    assert (on['pairs'] is None) == (off['pairs'] is None)
    if off['pairs'] is not None:
        assert list(on['pairs']) == list(off['pairs']) and len(off['pairs']) > 0
        for h, (s, g) in off['pairs'].items():
            assert np.array_equal(on['pairs'][h][0], s) and on['pairs'][h][1] == g, h


# ---------------------------------------------------------------------------------------------------------------------------
# 1. testing(), the flag on against off
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,bs', SHAPES)
@pytest.mark.parametrize('recipe', RECIPES)
def test_testing_is_bit_identical_with_the_flag_on(recipe, n, bs):
    runs = {}
    for flag in (False, True):
        model, loss, _ = _model(recipe, batch_size=bs, record_eval=flag)
        runs[flag] = _testing_result(model, loss, _store(recipe, n))
    _assert_same_evaluation(runs[True], runs[False])
    assert runs[False]['recorded'] == 0
    assert runs[True]['recorded'] == _full(n, bs) - 2          # one full batch ran eagerly, one was recorded: the rest are replays
    assert runs[False]['n_clips'] == n - (1 if n % bs == 1 else 0)      # (testing() skips a singleton batch)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. predict(), the flag on against off
# ---------------------------------------------------------------------------------------------------------------------------
def _assert_same_predictions(on, off):
    assert on.n_clips == off.n_clips
    for k in on.fields:
        a, b = getattr(on, k), getattr(off, k)
        assert (a is None) == (b is None), k
        if b is not None:
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), k
    assert (on.pairs is None) == (off.pairs is None)
    if off.pairs is not None:
        assert list(on.pairs) == list(off.pairs) and len(off.pairs) > 0
        for h, (order, s) in off.pairs.items():
            assert np.array_equal(on.pairs[h][0], order) and np.array_equal(on.pairs[h][1], s), h


@pytest.mark.parametrize('n,bs,top_k', [(24, 5, 5), (24, 6, 5), (25, 6, 5)])
@pytest.mark.parametrize('recipe', RECIPES)
def test_predict_is_bit_identical_with_the_flag_on(recipe, n, bs, top_k):
    _predict_pair(recipe, n, bs, top_k)


def test_predict_is_bit_identical_with_sixteen_top_entries():
    _predict_pair('int_rels', 24, 5, 16)


def _predict_pair(recipe, n, bs, top_k):
    runs, replayed = {}, {}
    for flag in (False, True):
        model, _, _ = _model(recipe, batch_size=bs, record_eval=flag)
        runs[flag] = predict(_store(recipe, n), model, top_k=top_k)
        replayed[flag] = predict.last['recorded_steps']
    _assert_same_predictions(runs[True], runs[False])
    assert runs[False].n_clips == n and runs[False].top_cls.shape == (n, top_k)
    assert replayed == {False: 0, True: _full(n, bs) - 2}
    if recipe == 'int_rels':
        assert runs[False].pairs is not None


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the parameters change between two evaluations: the second one reads what an eager forward at that moment reads
# ---------------------------------------------------------------------------------------------------------------------------
def test_an_optimiser_step_between_two_evaluations_reaches_the_second_one():
    ds = _store('int_rels', 24)
    second, first = {}, {}
    for flag in (False, True):
        model, loss, optim = _model('int_rels', batch_size=5, record_eval=flag)
        first[flag] = _testing_result(model, loss, ds)
        model.train()
        batch = next(iter(BlockLoader(ds, batch_size=5)))
        for _ in range(3):                                    # (eager train steps on the q32b kernels: shadow and staged weights in play)
            optim.zero_grad()
            lv = loss(model(dict(batch)), batch)
            lv.backward()
            optim.step()
        second[flag] = _testing_result(model, loss, ds)
    _assert_same_evaluation(second[True], second[False])
    _assert_same_evaluation(first[True], first[False])
    assert second[True]['recorded'] == first[True]['recorded'] == 2
    assert second[False]['loss'] != first[False]['loss'], 'the steps were meant to matter'


# ---------------------------------------------------------------------------------------------------------------------------
# 4. lirec_predict_clips_at
# ---------------------------------------------------------------------------------------------------------------------------
N_ROWS, C_, NR_, K_ = 12, 101, 15, 5


def _sentinel_bufs(n, T, K, with_rels):
    bufs = ops.predict_buffers(n, T, K, 'cuda', with_rels=with_rels)
    for t in bufs.values():
        t.view(torch.uint8).fill_(0xA5)
    return bufs


def _logits(B, T, with_rels, masked, seed):
    g = torch.Generator().manual_seed(seed)
    ints = torch.randn(B * T, C_, generator=g).cuda()
    rels = torch.randn(B * T, NR_, generator=g).cuda() if with_rels else None
    mem = None
    if masked:
        mem = torch.ones(B, T, dtype=torch.float64)
        mem[:, T - 1] = 0                                      # a padded track in every clip
        mem[B - 1] = 0                                         # ... and one clip without a valid track
        mem = mem.cuda()
    return ints, rels, mem


@pytest.mark.parametrize('with_rels', [False, True], ids=['ints', 'ints+rels'])
@pytest.mark.parametrize('T,masked', [(1, False), (4, True)], ids=['T1', 'T4-masked'])
@pytest.mark.parametrize('B', [1, 5])
def test_predict_clips_at_writes_the_rows_the_cursor_names_and_no_other(B, T, masked, with_rels):
    ints, rels, mem = _logits(B, T, with_rels, masked, seed=3 + B + T)
    for subset in (None, ('trk', 'top_cls_p')):               # every output; the optional ones NULL
        for cur in (0, 3, N_ROWS - B):
            cursor = torch.tensor([cur, -1], dtype=torch.int64, device='cuda')
            got, want = _sentinel_bufs(N_ROWS, T, K_, with_rels), _sentinel_bufs(N_ROWS, T, K_, with_rels)
            if subset is not None:
                got, want = {k: got[k] for k in subset}, {k: want[k] for k in subset}
            ops.predict_clips_at(ints, rels, mem, cursor, got, B=B, T=T, K=K_, loader_types=True)
            ops.predict_clips(ints, rels, mem, B=B, T=T, K=K_, loader_types=True, out={k: v[cur:cur + B] for k, v in want.items()})
            torch.cuda.synchronize()
            assert cursor.tolist() == [cur, -1]                # the launch does not move it
            for k in want:
                if k in ('top_rel', 'top_rel_p') and not with_rels:
                    continue
                # byte for byte: the rows inside equal lirec_predict_clips into the slice, the rows outside keep the sentinel
                assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), (k, cur, subset)
                inside = got[k][cur:cur + B].reshape(-1).view(torch.uint8)
                assert not bool((inside.reshape(-1, got[k].element_size()) == 0xA5).all(1).any()), (k, cur)


def test_predict_clips_at_replayed_from_a_command_list_follows_the_cursor():
    B, T = 5, 4
    ints, rels, mem = _logits(B, T, True, True, seed=9)
    got = _sentinel_bufs(N_ROWS, T, K_, True)
    cursor = torch.tensor([1], dtype=torch.int64, device='cuda')
    ops.CommandList.begin()
    try:
        ops.predict_clips_at(ints, rels, mem, cursor, got, B=B, T=T, K=K_, loader_types=True)
        ops.counter_add(cursor, [B])
    finally:
        cl = ops.CommandList.end()
    assert cl.size == 2
    ints.copy_(torch.randn(B * T, C_, generator=torch.Generator().manual_seed(10)))      # another batch in the same buffers
    cl.replay(0, -1)                                           # rows 6 .. 10
    torch.cuda.synchronize()
    assert int(cursor) == 11
    want = _sentinel_bufs(N_ROWS, T, K_, True)
    ops.predict_clips(ints, rels, mem, B=B, T=T, K=K_, loader_types=True, out={k: v[6:11] for k, v in want.items()})
    for k in want:
        assert torch.equal(got[k][6:].view(torch.uint8), want[k][6:].view(torch.uint8)), k
        assert bool((got[k][:1].view(torch.uint8) == 0xA5).all()) and bool((got[k][11:].view(torch.uint8) == 0xA5).all()), k
    cursor.fill_(0)                                            # moved by the host between two replays
    cl.replay(0, 1)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k][:5].view(torch.uint8), want[k][6:11].view(torch.uint8)), k
    cl.destroy()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. lirec_rows_copy_at
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cols', [15, 101])
@pytest.mark.parametrize('rows', [1, 5])
def test_rows_copy_at_copies_a_strided_view_to_the_rows_the_cursor_names(rows, cols):
    g = torch.Generator().manual_seed(rows * 7 + cols)
    block = torch.randn(rows * 19, cols, generator=g).cuda()
    src = block.reshape(rows, -1, cols)[:, 0]                  # row 0 of each clip's group of 19 rows, in place
    assert rows == 1 or not src.is_contiguous()
    for cur in (0, 3, N_ROWS - rows):
        cursor = torch.tensor([cur], dtype=torch.int64, device='cuda')
        dst = torch.empty(N_ROWS, cols, device='cuda')
        dst.view(torch.int32).fill_(0x7FC0DEAD)
        want = dst.clone()
        want[cur:cur + rows].copy_(src)
        ops.rows_copy_at(src, dst, cursor)
        torch.cuda.synchronize()
        assert int(cursor) == cur and torch.equal(dst.view(torch.int32), want.view(torch.int32)), (rows, cols, cur)
    # int64 rows moved as fp32 pairs, bit for bit (what the loops keep of a batch's labels and pair hashes)
    vals = torch.tensor([-1, 2 ** 40 + 3, -2 ** 62, 0x7FC00000_00000001, 7][:rows], dtype=torch.int64, device='cuda')
    keep = torch.zeros(N_ROWS, 2, device='cuda')
    ops.rows_copy_at(vals.reshape(rows, 1).view(torch.float32), keep, torch.tensor([2], dtype=torch.int64, device='cuda'))
    assert torch.equal(keep[2:2 + rows].view(torch.int64).reshape(-1), vals)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. lirec_scalar_accumulate
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'float64'])
def test_scalar_accumulate_equals_torch_in_place_add(dtype):
    vals = torch.tensor([0.1, 3.0e7, -1.25e-6, 12345.678, -2.9999999e7], dtype=torch.float32, device='cuda')
    got, want = torch.zeros(1, dtype=dtype, device='cuda'), torch.zeros(1, dtype=dtype, device='cuda')
    for i in range(5):
        ops.scalar_accumulate(got, vals[i:i + 1])
        want += vals[i:i + 1]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (dtype, i)
    assert float(want) != 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 7. fallbacks: today's loop, today's result, no complaint
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_dataset_without_a_block_store_keeps_the_eager_loop():
    ds = SyntheticMixedFeaturesDataset('int_rels', 24, seed=31, R=18)
    runs = {}
    for flag in (False, True):
        model, loss, _ = _model('int_rels', batch_size=5, record_eval=flag)
        runs[flag] = _testing_result(model, loss, ds)
        p = predict(ds, model)
        assert p.n_clips == 24 and predict.last['recorded_steps'] == 0
    _assert_same_evaluation(runs[True], runs[False])
    assert runs[True]['recorded'] == 0


class _ClipLabels(SyntheticMixedFeaturesDataset):
    """one interaction label per clip, what MultiTaskCrossEntropyLoss reads (mlp/model.py:371)"""

    def __getitem__(self, idx):
        s = dict(super().__getitem__(idx))
        s['labels'] = np.asarray(s['labels']).reshape(-1)[0]
        return s


def test_the_cross_entropy_loss_keeps_the_eager_loop():
    """the loss copies the batch's labels on the host's side in every call: a list would read the recording batch's"""
    ds = _store('int_rels', 24, _ClipLabels)
    runs = {}
    for flag in (False, True):
        model, loss, _ = _model('int_rels', batch_size=5, record_eval=flag, use_ce_loss=True)
        runs[flag] = _testing_result(model, loss, ds)
    _assert_same_evaluation(runs[True], runs[False])
    assert runs[True]['recorded'] == 0


def test_a_recording_that_raises_leaves_the_eager_loop_and_its_result(monkeypatch):
    ds = _store('int_rels', 24)
    model, loss, _ = _model('int_rels', batch_size=5, record_eval=False)
    want = _testing_result(model, loss, ds)
    model, loss, _ = _model('int_rels', batch_size=5, record_eval=True)
    calls = []

    def boom(acc, v):
        calls.append(1)
        raise _lib.LirecError('no accumulate today')
    monkeypatch.setattr(ops, 'scalar_accumulate', boom)
    got = _testing_result(model, loss, ds)
    assert calls == [1]                                        # tried once, on the second full batch; not again
    _assert_same_evaluation(got, want)
    assert got['recorded'] == 0
