#!/usr/bin/env python
"""``opt.device_collate`` on against off on the same commit: the three entry points over a resident piece store with the batch
buffer written on the device (``lirec_amd.loader.ResidentLoader``, ``lirec_collate_resident``) against the parent's path --
``ThreadedLoader`` with one loader thread, the collate on the host and one host-to-device copy per batch -- and one collate call
against the copy it replaces.

Usage:  python tools/device_collate_times.py [--pairs 3 --epochs 8 --launches 200 --clips-modalties 32768 --clips-int-rels 1024 --unique 64
                                              --out profiles/device_collate.json]

``training()``: the 2 048-clip pieces world of ``bench.py`` (256 scenes of 8 clips, 101 classes, 15 relationships), resident,
batch 64, shuffled; clips/s as ``training()`` prints it, the median of the epochs from the second on.  ``testing()`` / ``predict()``:
``int_rel_ch`` over the same dataset; ``modalties`` and ``int_rels`` over the synthetic tiled dataset (``--unique`` samples repeated,
the loader in the calling process) -- they have no resident store, so the flag falls back to the loader they had and the two arms
run the same code: the rows show that, and how far two runs of the same code lie apart.  One warm-up per arm, then ``--pairs`` alternating off / on pairs in one process;
host clock around work that ends in a device synchronise.  The call: ``--launches`` collate calls, and as many copies of the same
buffer from page-locked memory, each between two device events, alternated, the median per call -- at the bench world's table
sizes and on synthetic tables of 300 000 rows per store.  One JSON document, printed and written; figures only.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lirec_amd import config, ops            # noqa: E402
from lirec_amd import features as FA         # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.data import SyntheticMixedFeaturesDataset   # noqa: E402
from lirec_amd.predict import predict        # noqa: E402
from lirec_amd.test import testing           # noqa: E402
from lirec_amd.train import training         # noqa: E402

R, B = 18, 64
STEP_MS = 0.83                               # the recorded step at the bench shape (README)


class Repeated(torch.utils.data.Dataset):
    """``n_clips`` clips that repeat the first ``unique`` samples of a synthetic dataset, drawn once"""

    def __init__(self, base, unique, n_clips):
        self.samples = [base[i] for i in range(unique)]
        self.n_clips = n_clips
        self.n_classes, self.n_rels, self.interidx2mgdidx = base.n_classes, base.n_rels, base.interidx2mgdidx

    def __len__(self):
        return self.n_clips

    def __getitem__(self, idx):
        return self.samples[idx % len(self.samples)]


def summary(rate):
    row = {'arms': {}}
    for flag, name in ((False, 'off'), (True, 'on')):
        v = rate[flag]
        row['arms'][name] = {'clips_per_s': round(statistics.median(v), 1), 'pairs': [round(x, 1) for x in v],
                             'spread': round(max(v) - min(v), 1)}
    row['on_over_off'] = round(statistics.median(rate[True]) / statistics.median(rate[False]), 4)
    row['on_over_off_pairs'] = [round(a / b, 4) for a, b in zip(rate[True], rate[False])]
    return row


def alternate(run, pairs):
    for flag in (False, True):
        run(flag)                            # warm-up
    rate = {False: [], True: []}
    for _ in range(pairs):
        for flag in (False, True):
            rate[flag].append(run(flag))
    return summary(rate)


def train_rows(ds, pairs, epochs):
    config.recipe('int_rel_ch', rels_n_clips=R, batch_size=B, num_workers=1)
    opt.device = 'cuda'
    opt.set(epochs=epochs, test_fr=1000, test=False, save_model=False, rels_dim=15)
    torch.manual_seed(1)
    model, loss, optim = M.create_model(101, n_rels=15)

    def run(flag):
        opt.device_collate = flag
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            training(ds, model=model, loss=loss, optimizer=optim)
        torch.cuda.synchronize()
        rates = [float(l.split(':')[1]) for l in buf.getvalue().splitlines() if l.startswith('train clips/s')]
        last = training.last
        assert last['replays'] > 0 and (last['input_copies'] == 0) == flag, last
        print('training flag=%s: %s' % (flag, [round(r) for r in rates]), file=sys.stderr, flush=True)
        return statistics.median(rates[1:])
    row = alternate(run, pairs)
    row.update(clips_per_epoch=len(ds), epochs=epochs, batch_size=B, loader_threads_off=1,
               what='training(): median of the epochs from the second on, clips/s as training() prints it')
    return row, (model, loss)


def eval_rows(kind, ds, pairs, model_loss=None, falls_back=False):
    if model_loss is None:
        config.recipe(kind, batch_size=B, num_workers=0)           # (the tiled loader in the calling process, as tools/predict_times.py)
        opt.device = 'cuda'
        torch.manual_seed(1)
        model, loss, _ = M.create_model(101, n_rels=15)
    else:
        model, loss = model_loss
    n = len(ds)
    out = {}
    for what, call in (('testing', lambda: testing(ds, model, loss, mode='test', verbose=False)), ('predict', lambda: predict(ds, model))):
        def run(flag):
            opt.device_collate = flag
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print('%s %s flag=%s: %.1f clips/s' % (kind, what, flag, n / dt), file=sys.stderr, flush=True)
            return n / dt
        row = alternate(run, pairs)
        row.update(clips=n, batch_size=B, flag_falls_back=falls_back)
        out[what] = row
    opt.device_collate = False
    return out


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches              # microseconds per call


def call_rows(name, tabs, n_all, layout, nbytes, n_samples, pairs, launches):
    """one collate call against the host-to-device copy of the same buffer"""
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, n_samples, (B,), generator=g).int().cuda()
    blob = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    view = FA.layout_views(blob, layout)
    ws = ops.collate_workspace(n_all[0], n_all[1], 'cuda')
    counts = torch.empty(2, dtype=torch.int32, device='cuda')
    fields = [(tabs[k], view[k]) for k in FA._FIELDS]
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    arms = {'collate_call': lambda: ops.collate_resident(ids, tabs['index_rows'], n_all[0], n_all[1], view['feature_index'],
                                                         view['clip_rows'], view['track_rows'], counts, fields, ws),
            'h2d_copy': lambda: blob.copy_(host, non_blocking=True)}
    us = {k: [] for k in arms}
    for fn in arms.values():
        timed(fn, launches)
    for _ in range(pairs):
        for k, fn in arms.items():
            us[k].append(timed(fn, launches))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {'tables': name, 'clip_rows_all': n_all[0], 'track_rows_all': n_all[1], 'batch_size': B, 'buffer_bytes': nbytes, 'launches': launches,
            'what': 'microseconds per call, back-to-back calls between two device events (launch overhead included; four commands a '
                    'collate call)',
            'us_per_call': {k: {'median': round(med[k], 2), 'pairs': [round(x, 2) for x in us[k]]} for k in arms},
            'collate_over_copy': round(med['collate_call'] / med['h2d_copy'], 3),
            'collate_share_of_the_step': round(med['collate_call'] / (STEP_MS * 1e3), 4)}


def synthetic_tables(n_all, n_samples=256, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    E = FA.T_MAX * (R + 1)
    rows = np.empty((n_samples, E, 3), dtype=np.int32)
    rows[..., 0] = rng.integers(0, n_all[0], size=(n_samples, E))
    rows[..., 1:] = rng.integers(0, n_all[1], size=(n_samples, E, 2))
    rows[rng.random(rows.shape) < 0.25] = -1
    return rows.reshape(n_samples, FA.T_MAX, R + 1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--clips-modalties', type=int, default=32768)
    ap.add_argument('--clips-int-rels', type=int, default=1024)
    ap.add_argument('--unique', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_collate.json'))
    a = ap.parse_args()
    wd = FA.synthetic_world(4321, n_scenes=256, per_scene=8, n_rel_names=15, n_inter_names=101)
    ds = FA.PiecesDataset(wd, R, 101, resident=True)
    res = {'device': torch.cuda.get_device_name(0), 'pairs': a.pairs, 'step_ms': STEP_MS, 'rows': {}}
    res['rows']['training'], model_loss = train_rows(ds, a.pairs, a.epochs)
    ev = eval_rows('int_rel_ch', ds, a.pairs, model_loss)
    res['rows']['testing_int_rel_ch'], res['rows']['predict_int_rel_ch'] = ev['testing'], ev['predict']
    # the call itself: the bench world's tables, then 300 000 rows per store
    from lirec_amd.loader import ResidentLoader
    tabs = ds.device_tables('cuda')
    layout, nbytes = ResidentLoader(ds, batch_size=B).layout(B)
    res['call'] = [call_rows('bench world', tabs, tabs['n_all'], layout, nbytes, len(ds), a.pairs, a.launches)]
    big = (300000, 300000)
    tabs_big = dict(tabs, index_rows=torch.from_numpy(synthetic_tables(big)).cuda())
    tabs_big.update({k: tabs[k][:256].contiguous() for k in FA._FIELDS})
    fields = [(k, ds._stacked[k].dtype, (B,) + ds._stacked[k].shape[1:]) for k in FA._FIELDS]
    layout_big, nbytes_big = FA.batch_layout((B, FA.T_MAX, R + 1, 3), fields, n_all=big)
    res['call'].append(call_rows('synthetic, 300 000 rows per store', tabs_big, big, layout_big, nbytes_big, 256, a.pairs, a.launches))
    del model_loss
    for kind, n_clips in (('modalties', a.clips_modalties), ('int_rels', a.clips_int_rels)):
        config.recipe(kind, batch_size=B, num_workers=0)
        base = SyntheticMixedFeaturesDataset(kind, a.unique, seed=7, soft_gt=opt.soft_gt)
        ev = eval_rows(kind, Repeated(base, a.unique, n_clips), a.pairs, falls_back=True)
        res['rows']['testing_' + kind], res['rows']['predict_' + kind] = ev['testing'], ev['predict']
    worst = min(r['on_over_off'] for r in res['rows'].values())
    res['worst_on_over_off'] = worst
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
