"""The resident block store on the GPU (lirec_amd.blockstore, lirec_amd.loader.BlockLoader; include/lirec_hip.h: lirec_set_feature_rows,
lirec_q32b_write_rows, lirec_collate_fields).  The criterion throughout is BIT IDENTITY with the path the store replaces: the same
samples collated on the host and stored as a per-batch q32b block (``to_device_batch(collate(samples), feature_dtype='q32')``) --
``torch.equal`` on logits, loss, gradients and parameters; no tolerance anywhere.  Real feature width (D = 6912, J = 512): the
gathered q32b path has divisibility conditions; clip counts are tiny."""
import numpy as np
import pytest
import torch

from lirec_amd import _lib, blockstore as BS, config
from lirec_amd.config import opt
from lirec_amd.data import SyntheticMixedFeaturesDataset, WeightedDataset, collate, to_device_batch
from lirec_amd.loader import BlockLoader, make_loader
from oracle import lirec_oracle as O

pytestmark = pytest.mark.gpu
SMALL = dict(text_dim=32, visual_dim=32, track_dim=32)          # D = 128: loader tests that run no model


class _Holder:
    """a list of samples with a block store: what BlockLoader asks of a dataset"""

    def __init__(self, samples, **kw):
        self.samples, self.block_store = samples, BS.BlockStore(samples, 'cuda', **kw)

    def __len__(self):
        return self.block_store.n

    def __getitem__(self, i):
        return self.samples[i]


def _model(recipe, R, compact=True, planes=True, **over):
    from lirec_amd import model as M
    config.recipe(recipe, dropout=0.3, dropout_seed=77, **({} if recipe == 'modalties' else {'rels_n_clips': R}), **over)
    opt.device = 'cuda'
    opt.layer1_planes = planes
    opt.compact_ctx_rows = compact
    model, loss, optim = M.create_model(101, n_rels=15)
    if recipe != 'modalties':
        cfg = O.OracleCfg(tr_maximize=recipe != 'int_rels', ctx=0 if recipe == 'int_ch' else 1, gates=0 if recipe == 'int_ch' else 1,
                          rels_multitask=recipe != 'int_ch')
        model.load_state_dict(O.fill_params(O.param_shapes(cfg, 101, 15 if recipe != 'int_ch' else 0), 5), strict=True)
    return model, loss, optim


def _step(model, loss, optim, batch, train=True):
    """(logits, loss, gradients) of one training step on ``batch`` from the model's first dropout key, or the eval-mode logits"""
    if not train:
        model.eval()
        with torch.no_grad():
            out = model(dict(batch))
        torch.cuda.synchronize()
        assert model.last_layer1_planes, 'the gathered q32b path was meant to run'
        return {k: v.detach().clone() for k, v in out.items() if v is not None}, None, {}
    model.train()
    model._fwd_train_calls = 0
    optim.zero_grad()
    out = model(dict(batch))
    pre = {k: v.detach().clone() for k, v in out.items() if v is not None}
    lv = loss(out, batch)
    lv.backward()
    torch.cuda.synchronize()
    assert model.last_layer1_planes, 'the gathered q32b path was meant to run'
    return pre, lv.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _same(a, b, what):
    assert set(a[0]) == set(b[0]) and a[0], what
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), (what, 'logits', k)
    if a[1] is not None:
        assert torch.equal(a[1], b[1]), (what, 'loss')
        assert torch.isfinite(a[1]).all()
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), (what, 'grad', k)


def _batches(samples, ids, **store_kw):
    """(the store's batch for ``ids``, the parent path's batch for the same samples)"""
    holder = _Holder(samples, **store_kw)
    loader = BlockLoader(holder, batch_size=len(ids))
    dev_ids = torch.tensor(ids, dtype=torch.int32, device='cuda')
    got = loader.collate_ids(dev_ids, len(ids))
    want = to_device_batch(collate([samples[i] for i in ids]), 'cuda', feature_dtype='q32')
    return got, want, holder


def _assert_batch_equal(got, want):
    """key for key, dtype for dtype, value for value (+ ``_layout`` and ``_dev_blob``); the features by what they name"""
    assert [k for k in got if not k.startswith('_')] == list(want)
    assert '_layout' in got and '_dev_blob' in got
    for k, v in want.items():
        if k == 'features':
            assert got[k].shape == v.shape and got[k].dtype == v.dtype == 'q32' and got[k].x_q32 == 1
            continue
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and got[k].is_cuda and torch.equal(got[k], v), k


CASES = {
    'modalties': ('modalties', 5, {}, 0, True),
    'int_rels': ('int_rels', 5, dict(R=18), 18, True),
    'int_rels-uncompacted': ('int_rels', 5, dict(R=18), 18, False),
    'int_ch': ('int_ch', 3, dict(T=7), 0, True),
    'int_rel_ch': ('int_rel_ch', 3, dict(T=7, R=18), 18, True),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_store_batches_are_bit_identical_to_per_batch_blocks(case):
    """7 samples resident, ids out of order with the last sample and a duplicate: training step (dropout 0.3) and eval logits"""
    recipe, B, kw, R, compact = CASES[case]
    ds = SyntheticMixedFeaturesDataset(recipe, 7, seed=11, **kw)
    samples = [ds[i] for i in range(7)]
    ids = [6, 2, 0, 2, 4][:B] if B == 5 else [6, 2, 2]
    got, want, holder = _batches(samples, ids)
    _assert_batch_equal(got, want)
    st = holder.block_store
    assert got['features'].data.data_ptr() == st.data.data_ptr() and st.rows_per_clip == int(np.prod(st.feature_shape[:-1]))
    assert got['features'].clip_ids.tolist() == ids
    model, loss, optim = _model(recipe, R, compact)
    _same(_step(model, loss, optim, got), _step(model, loss, optim, want), case + ' train')
    _same(_step(model, loss, optim, got, train=False), _step(model, loss, optim, want, train=False), case + ' eval')


@pytest.mark.parametrize('src_dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
def test_write_rows_bytes_equal_to_q32b_of_the_assembled_matrix(src_dtype):
    from lirec_amd import ops
    D, rows32 = 6912, 96
    g = torch.Generator(device='cuda').manual_seed(5)
    base = torch.randn(rows32, D, device='cuda', generator=g)
    pattern = ops.to_q32b(base).data[:rows32 * D * 4].clone()
    for row0 in (0, 1, 19, 31, 32, 33):
        for rows in (1, 19, 32, 45):
            src = torch.randn(rows, D, device='cuda', generator=g, dtype=src_dtype)
            src[0, :8] = torch.tensor([0.0, -0.0, 1e-40, 3.0e38, -1.0000001, 65504.0, 2.0 ** -126, 1.0 / 3.0], dtype=src_dtype)
            dst = pattern.clone()
            ops.q32b_write_rows(src, dst, row0, rows32)
            want = base.clone()
            want[row0:row0 + rows] = src if src_dtype == torch.float32 else ops.cast_f64_f32(src)
            ref = ops.to_q32b(want).data[:rows32 * D * 4]
            assert torch.equal(dst, ref), (row0, rows)      # (outside the written rows the reference IS the pattern: nothing moved)


def test_store_bytes_equal_to_q32b_of_the_whole_dataset(monkeypatch):
    """filled in chunks (three samples a chunk here), float64 samples, tail rows zeroed: the bytes lirec_to_q32b gives for all rows"""
    from lirec_amd import ops
    ds = SyntheticMixedFeaturesDataset('int_rels', 7, seed=3, R=4, **SMALL)
    samples = [ds[i] for i in range(7)]
    monkeypatch.setattr(BS, 'CHUNK_BYTES', 3 * samples[0]['features'].nbytes)
    st = BS.BlockStore(samples, 'cuda')
    allf = torch.from_numpy(np.stack([s['features'] for s in samples])).to('cuda', torch.float32)
    ref = ops.to_q32b(allf.contiguous())
    assert st.store_rows == 64 and st.n * st.rows_per_clip == 35
    assert torch.equal(st.data[:64 * 128 * 4], ref.data[:64 * 128 * 4])
    # update(): two samples rewritten in place, nothing else moves
    new = torch.randn(2, 5, 128, dtype=torch.float64)
    st.update([6, 1], new)
    allf[6], allf[1] = new[0].to('cuda', torch.float32), new[1].to('cuda', torch.float32)
    assert torch.equal(st.data[:64 * 128 * 4], ops.to_q32b(allf.contiguous()).data[:64 * 128 * 4])


def test_collate_fields_bytes_equal_index_select():
    from lirec_amd import ops
    N = 37
    g = torch.Generator().manual_seed(2)
    for B, ids in ((6, [36, 0, 5, 5, 17, 1]), (1, [36]), (0, [])):
        dev_ids = torch.tensor(ids, dtype=torch.int32, device='cuda')
        blob = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device='cuda')
        pairs, spans, at = [], [], 0
        for f, rb in enumerate((1, 4, 8, 808, 13, 16, 12)):
            src = torch.randint(0, 256, (N, rb), dtype=torch.uint8, generator=g).cuda()
            at = (at + 255) // 256 * 256 + (0, 1, 4, 8, 3, 0, 2)[f]           # misaligned destinations: every move width
            dst = blob[at:at + B * rb].view(B, rb)
            pairs.append((src, dst))
            spans.append((at, B * rb, src))
            at += B * rb
        ops.collate_fields(dev_ids, pairs)
        torch.cuda.synchronize()
        want = torch.full_like(blob, 0xA5)
        for at, n, src in spans:
            want[at:at + n] = src.index_select(0, dev_ids.long()).reshape(-1)
        assert torch.equal(blob, want), B                                      # the rows, and not a byte beside them
    # typed tables as the loader hands them over (a 0-d field per sample, int64 / float64 / bool)
    tabs = [torch.arange(N, device='cuda') * 3, torch.rand(N, 101, dtype=torch.float64, device='cuda'), torch.rand(N, device='cuda') > 0.5]
    dev_ids = torch.tensor([3, 36, 3], dtype=torch.int32, device='cuda')
    outs = [torch.empty((3,) + tuple(t.shape[1:]), dtype=t.dtype, device='cuda') for t in tabs]
    ops.collate_fields(dev_ids, list(zip(tabs, outs)))
    for t, o in zip(tabs, outs):
        assert torch.equal(o, t[dev_ids.long()])


@pytest.mark.parametrize('kind', ['modalties', 'int_rels', 'int_ch', 'int_rel_ch'])
def test_loader_batches_equal_the_host_collate(kind):
    """make_loader picks BlockLoader; sequential batches (a short last one) key for key against default_collate + to_device_batch"""
    kw = {'modalties': {}, 'int_rels': dict(R=4), 'int_ch': dict(T=3), 'int_rel_ch': dict(T=3, R=4)}[kind]
    config.recipe(kind)
    opt.device = 'cuda'
    ds = SyntheticMixedFeaturesDataset(kind, 7, seed=5, **SMALL, **kw)
    rds = BS.ResidentBlockDataset(ds)
    assert len(rds) == 7 and rds.n_classes == ds.n_classes and rds.n_rels == ds.n_rels and rds.rels_list == ds.rels_list
    assert rds.interidx2mgdidx == ds.interidx2mgdidx and set(rds[3]) == set(ds[3])
    rds.epoch = 4
    assert ds.epoch == 4 and rds.epoch == 4
    loader = make_loader(rds, 3)
    assert isinstance(loader, BlockLoader) and len(loader) == 3
    order = [[0, 1, 2], [3, 4, 5], [6]]
    for got, idx in zip(loader, order):
        _assert_batch_equal(got, to_device_batch(collate([ds[i] for i in idx]), 'cuda', feature_dtype='q32'))
        assert got['features'].clip_ids.tolist() == idx
    assert loader.n_collate == 3 and loader.n_in_place == 0
    assert set(rds.device_tables()) == set(ds[0]) - {'features'} | {BS.IDS_KEY}
    # bind: a batch of the bound layout is written into the given buffer, any other into one of its own
    layout, nbytes = loader.layout(3)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    loader.bind(layout, blob)
    b = [x for x in loader]
    assert b[0]['_dev_blob'] is blob and b[1]['_dev_blob'] is blob and b[2]['_dev_blob'] is not blob and loader.n_in_place == 2
    loader.unbind()
    assert next(iter(loader))['_dev_blob'] is not blob


def test_loader_with_replacement_and_clip_weights_equals_the_stock_loader():
    """a sampler that draws with replacement (duplicate ids inside a batch) and a dataset whose samples carry ``clip_weight``: the
    same generator seed gives the stock DataLoader's batches"""
    config.recipe('int_rels')
    opt.device, opt.num_workers = 'cuda', 0
    ds = SyntheticMixedFeaturesDataset('int_rels', 6, seed=9, R=4, **SMALL)
    w = np.linspace(0.5, 2.0, 6)
    wds = WeightedDataset(ds, w)
    mk = lambda d: torch.utils.data.RandomSampler(d, replacement=True, num_samples=11, generator=torch.Generator().manual_seed(4))
    rds = BS.ResidentBlockDataset(wds)
    got = list(make_loader(rds, 4, sampler=mk(rds)))
    want = list(torch.utils.data.DataLoader(wds, batch_size=4, sampler=mk(wds)))
    assert len(got) == len(want) == 3
    seen = []
    for g, h in zip(got, want):
        _assert_batch_equal(g, to_device_batch(h, 'cuda', feature_dtype='q32'))
        assert g['clip_weight'].dtype == torch.float64
        seen += g['features'].clip_ids.tolist()
    assert len(set(seen)) < len(seen) == 11
    # weights handed to the store itself ride along the same way; wrapped AROUND the store they would be lost: refused
    r2 = BS.ResidentBlockDataset(ds)
    r2.set_clip_weights(w)
    g2 = next(iter(make_loader(r2, 6)))
    assert torch.equal(g2['clip_weight'].cpu(), torch.from_numpy(w)) and r2[2]['clip_weight'] == w[2]
    with pytest.raises(_lib.LirecError, match='per-clip weights'):
        make_loader(WeightedDataset(BS.ResidentBlockDataset(ds), w), 4)
    # a sample id outside the store
    with pytest.raises(IndexError):
        list(BlockLoader(rds, batch_size=2, sampler=[0, 6]))


def test_rows_beyond_4_gib_are_addressed_with_64_bits():
    """an int_rels store of 8 200 slots (155 800 rows of 27 648 B: 4.3 GB); two samples at ids 0 and 1, two past byte 2^32 -- the
    smallest shape at which a 32-bit row offset would show.  One batch of the four, forward and backward."""
    ds = SyntheticMixedFeaturesDataset('int_rels', 4, seed=21, R=18)
    samples = [ds[i] for i in range(4)]
    holder = _Holder(samples[:2], capacity=8200)
    st = holder.block_store
    assert st.store_rows == 155808 and 8177 * st.rows_per_clip * 27648 > 2 ** 32 > 8176 * st.rows_per_clip * 27648
    rest = collate(samples[2:])
    st.update([8177, 8199], rest.pop('features'), rest)
    where = {8199: 3, 0: 0, 8177: 2, 1: 1}
    ids = list(where)
    got = BlockLoader(holder, batch_size=4).collate_ids(torch.tensor(ids, dtype=torch.int32, device='cuda'), 4)
    want = to_device_batch(collate([samples[where[i]] for i in ids]), 'cuda', feature_dtype='q32')
    _assert_batch_equal(got, want)
    model, loss, optim = _model('int_rels', 18)
    _same(_step(model, loss, optim, got), _step(model, loss, optim, want), 'beyond 4 GiB')
    del got, holder, st
    torch.cuda.empty_cache()


class _PerBatchQ32(SyntheticMixedFeaturesDataset):
    """the parent's path with the features converted per batch: the stock loader's batch, stored as a q32b block on the device"""

    @staticmethod
    def to_device(batch):
        return to_device_batch(batch, 'cuda', feature_dtype='q32')


def test_training_testing_and_predict_over_the_store(tmp_path):
    """training() for 2 epochs (shuffled, the same sampler seed), then testing() and predict(): parameters bit-identical, results
    equal.  The recorded step is not built for these batches (DESIGN): the loop steps eagerly and says so in ``training.last``."""
    from lirec_amd.predict import predict
    from lirec_amd.test import testing
    from lirec_amd.train import training

    def run(resident):
        model, loss, optim = _model('int_rels', 18, batch_size=5, num_workers=0, epochs=2, test_fr=1, store_root=str(tmp_path),
                                    save_model=False)
        opt.layer1_planes_eval = True          # (the plain dataset's fp32 eval block staged as q32b: the store's bits, not the on-the-fly kernel's)
        plain = _PerBatchQ32('int_rels', 24, seed=31, R=18)
        ds = BS.ResidentBlockDataset(plain) if resident else plain
        sampler = torch.utils.data.RandomSampler(ds, generator=torch.Generator().manual_seed(123))
        training(ds, model=model, loss=loss, optimizer=optim, sampler=sampler)
        last = dict(training.last)
        res = testing(ds, model, loss, mode='test', verbose=False)
        pred = predict(ds, model)
        opt.layer1_planes_eval = False
        return model.flat_params().clone(), last, res, testing.last['loss'], pred

    pa, la, ra, lossa, preda = run(True)
    pb, lb, rb, lossb, predb = run(False)
    assert isinstance(la['loader'], BlockLoader) and la['loader'].n_collate > 0 and not isinstance(lb['loader'], BlockLoader)
    assert la['replays'] == 0 and la['input_copies'] == 0
    assert torch.isfinite(pa).all() and torch.equal(pa, pb)
    assert ra == rb and lossa == lossb
    assert preda.n_clips == predb.n_clips == 24
    for k in preda.fields:
        a, b = getattr(preda, k), getattr(predb, k)
        assert (a is None and b is None) or np.array_equal(a, b), k
    assert set(preda.pairs) == set(predb.pairs) and preda.pairs
    for h in preda.pairs:
        assert all(np.array_equal(x, y) for x, y in zip(preda.pairs[h], predb.pairs[h])), h


def test_refused_configurations_raise_and_launch_nothing():
    from lirec_amd import ops
    ds = SyntheticMixedFeaturesDataset('int_rels', 3, seed=2, R=18)
    samples = [ds[i] for i in range(3)]
    got, want, holder = _batches(samples, [2, 0, 2])

    def refused(model, batch, match):
        ops.CommandList.begin()
        try:
            with pytest.raises(_lib.LirecError, match=match):
                model(dict(batch))
        finally:
            cl = ops.CommandList.end()
        n = cl.size
        cl.destroy()
        assert n == 0, 'a refused forward launched %d commands' % n

    model, loss, optim = _model('int_rels', 18, planes=False)          # opt.layer1_planes off: no gathered path
    model.train()
    refused(model, got, 'layer1_planes')
    model.eval()
    refused(model, got, 'layer1_planes')
    model, loss, optim = _model('int_rels', 18)
    mode = ops.get_gemm_mode()
    try:
        for m in (0, 1, 3):                                            # the other GEMM cores have no gathered q32b kernels
            ops.set_gemm_mode(m)
            model.train()
            refused(model, got, 'gemm mode 2')
    finally:
        ops.set_gemm_mode(mode)
    # the library's own refusal (the model's checks bypassed): an armed call that would leave the gathered path
    model.train()
    _same(_step(model, loss, optim, got), _step(model, loss, optim, want), 'after the refusals')
    # a store that does not fit: refused before any device memory is taken
    before = torch.cuda.memory_allocated()
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(_lib.LirecError, match='MARGIN_BYTES'):
        BS.BlockStore(samples, 'cuda', capacity=free // (19 * 27648) + 1)
    assert torch.cuda.memory_allocated() == before
