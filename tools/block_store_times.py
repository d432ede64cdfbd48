#!/usr/bin/env python
"""A tiled dataset resident in a block store (``lirec_amd.blockstore.ResidentBlockDataset``, drawn by ``BlockLoader``) against the
parent's path for the same dataset -- the stock ``DataLoader`` over the tiled float64 samples, one host-to-device copy and one cast
per batch -- for the three entry points, and one ``lirec_collate_fields`` call against the copy it replaces.

Usage:  python tools/block_store_times.py [--pairs 3 --epochs 3 --launches 200 --clips-modalties 16384 --clips-int-rels 1024
                                            --clips-int-ch 1024 --unique 64 --out profiles/block_store.json]

``modalties``, ``int_rels`` and ``int_ch`` (T = 20) over the synthetic tiled dataset at the real feature width (``--unique`` samples
repeated, the loader in the calling process), batch 64, ``opt.layer1_planes`` on in both arms so that both run the q32b layer-1
kernels.  ``training()``: shuffled, clips/s as ``training()`` prints it, the median of the epochs from the second on; ``testing()`` /
``predict()``: host clock around a call that ends in a device synchronise.  One warm-up per arm, then ``--pairs`` alternating
loader / store pairs in one process.  The store is built once per recipe, outside the timed region; its build time and bytes are
recorded.  The call: ``--launches`` collate calls of an ``int_rels`` batch, and as many copies of the same buffer from page-locked
memory, each between two device events, alternated, the median per call.  One JSON document, printed and written; figures only.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lirec_amd import config, ops            # noqa: E402
from lirec_amd import features as FA         # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.blockstore import ResidentBlockDataset   # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.data import SyntheticMixedFeaturesDataset   # noqa: E402
from lirec_amd.loader import BlockLoader     # noqa: E402
from lirec_amd.predict import predict        # noqa: E402
from lirec_amd.test import testing           # noqa: E402
from lirec_amd.train import training         # noqa: E402

B = 64
ARMS = ('loader', 'store')


class Repeated(torch.utils.data.Dataset):
    """``n_clips`` clips that repeat the first ``unique`` samples of a synthetic dataset, drawn once"""

    def __init__(self, base, unique, n_clips):
        self.samples = [base[i] for i in range(unique)]
        self.n_clips, self.epoch = n_clips, 0
        self.n_classes, self.n_rels, self.rels_list, self.interidx2mgdidx = base.n_classes, base.n_rels, base.rels_list, base.interidx2mgdidx

    def __len__(self):
        return self.n_clips

    def __getitem__(self, idx):
        return self.samples[idx % len(self.samples)]


def summary(rate):
    row = {'arms': {k: {'clips_per_s': round(statistics.median(v), 1), 'pairs': [round(x, 1) for x in v]} for k, v in rate.items()}}
    row['store_over_loader'] = round(statistics.median(rate['store']) / statistics.median(rate['loader']), 3)
    row['store_over_loader_pairs'] = [round(a / b, 3) for a, b in zip(rate['store'], rate['loader'])]
    row['store_faster_in_every_pair'] = all(a > b for a, b in zip(rate['store'], rate['loader']))
    return row


def alternate(run, pairs):
    for arm in ARMS:
        run(arm)                             # warm-up
    rate = {arm: [] for arm in ARMS}
    for _ in range(pairs):
        for arm in ARMS:
            rate[arm].append(run(arm))
    return summary(rate)


def recipe_rows(kind, n_clips, unique, pairs, epochs):
    kw = dict(T=20) if kind == 'int_ch' else {}
    config.recipe(kind, batch_size=B, num_workers=0)
    opt.device = 'cuda'
    opt.set(epochs=epochs, test_fr=1000, test=False, save_model=False, layer1_planes=True)
    base = SyntheticMixedFeaturesDataset(kind, unique, seed=7, soft_gt=opt.soft_gt, **kw)
    data = {'loader': Repeated(base, unique, n_clips)}
    t0 = time.perf_counter()
    data['store'] = ResidentBlockDataset(data['loader'])
    torch.cuda.synchronize()
    built = time.perf_counter() - t0
    st = data['store'].block_store
    torch.manual_seed(1)
    model, loss, optim = M.create_model(101, n_rels=15)
    rows = {'clips': n_clips, 'batch_size': B, 'store_bytes': st.nbytes, 'store_rows': st.store_rows, 'rows_per_clip': st.rows_per_clip,
            'store_build_s': round(built, 2)}

    def train(arm):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            training(data[arm], model=model, loss=loss, optimizer=optim)
        torch.cuda.synchronize()
        rates = [float(l.split(':')[1]) for l in buf.getvalue().splitlines() if l.startswith('train clips/s')]
        assert isinstance(training.last['loader'], BlockLoader) == (arm == 'store'), training.last
        print('%s training %s: %s' % (kind, arm, [round(r) for r in rates]), file=sys.stderr, flush=True)
        return statistics.median(rates[1:])
    rows['training'] = alternate(train, pairs)
    rows['training']['what'] = 'median of the epochs from the second on, clips/s as training() prints it; %d epochs' % epochs
    for what, call in (('testing', lambda ds: testing(ds, model, loss, mode='test', verbose=False)), ('predict', lambda ds: predict(ds, model))):
        def run(arm):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(data[arm])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print('%s %s %s: %.1f clips/s' % (kind, what, arm, n_clips / dt), file=sys.stderr, flush=True)
            return n_clips / dt
        rows[what] = alternate(run, pairs)
    del data, model, loss, optim
    torch.cuda.empty_cache()
    return rows


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches              # microseconds per call


def call_rows(unique, pairs, launches):
    """one lirec_collate_fields call of an int_rels batch against the host-to-device copy of the same buffer"""
    config.recipe('int_rels', batch_size=B, num_workers=0)
    opt.device = 'cuda'
    base = SyntheticMixedFeaturesDataset('int_rels', unique, seed=7)
    ds = ResidentBlockDataset(Repeated(base, unique, 1024))
    loader = BlockLoader(ds, batch_size=B)
    layout, nbytes = loader.layout(B)
    ids = torch.randint(0, 1024, (B,), generator=torch.Generator().manual_seed(5)).int().cuda()
    blob = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    view = FA.layout_views(blob, layout)
    pairs_ = [(ds.block_store.tables[k], view[k]) for k, _, _, _, _ in layout]
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    arms = {'collate_call': lambda: ops.collate_fields(ids, pairs_), 'h2d_copy': lambda: blob.copy_(host, non_blocking=True)}
    us = {k: [] for k in arms}
    for fn in arms.values():
        timed(fn, launches)
    for _ in range(pairs):
        for k, fn in arms.items():
            us[k].append(timed(fn, launches))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {'recipe': 'int_rels', 'batch_size': B, 'fields': len(pairs_), 'buffer_bytes': nbytes, 'launches': launches,
            'what': 'microseconds per call, back-to-back calls between two device events (launch overhead included; one launch a call); the '
                    'copy moves the small fields only -- the feature block the loader path also copies (%d bytes a batch) is not in it'
                    % (B * ds.block_store.rows_per_clip * ds.block_store.D * 8),
            'us_per_call': {k: {'median': round(med[k], 2), 'pairs': [round(x, 2) for x in us[k]]} for k in arms},
            'collate_over_copy': round(med['collate_call'] / med['h2d_copy'], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--clips-modalties', type=int, default=16384)
    ap.add_argument('--clips-int-rels', type=int, default=1024)
    ap.add_argument('--clips-int-ch', type=int, default=1024)
    ap.add_argument('--unique', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'block_store.json'))
    a = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'pairs': a.pairs, 'rows': {}}
    for kind, n in (('modalties', a.clips_modalties), ('int_rels', a.clips_int_rels), ('int_ch', a.clips_int_ch)):
        res['rows'][kind] = recipe_rows(kind, n, a.unique, a.pairs, a.epochs)
    res['call'] = call_rows(a.unique, a.pairs, a.launches)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
