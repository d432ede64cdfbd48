#!/usr/bin/env python
"""``lirec_amd.test.testing`` with the clip-level evaluation counters on the device (``opt.device_metrics``) and on the host, for
the two recipes without a maximum over tracks: ``modalties`` and ``int_rels`` (512 clips per batch).

Usage:  python tools/eval_clip_times.py [--clips-modalties 32768 --clips-int-rels 16384 --unique 256 --pairs 3
                                         --out profiles/eval_clip_metrics.json]

Per recipe: the synthetic dataset at full dimensions (text 768, visual 2048, track 2048; 101 classes, 15 relationships, 18
context clips), ``--unique`` samples drawn once and repeated up to the dataset's length, so that the loop is not timed on the
random generator; the loader runs in the evaluating process (``num_workers=0``).  One warm-up evaluation per arm, then
``--pairs`` alternating on / off pairs in one process, so that drift of the box hits both arms.  The off arm is the per-batch host
path (``.item()``, ``.cpu()``, argsort in numpy), line for line what it was before the device path existed: the flag is the A/B.
Reported per arm: clips / s (median over the pairs), the pairs, their spread (max - min); per recipe the ratio on / off of the
medians and whether the two arms returned the same metrics.  One JSON document, printed and written; figures only.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lirec_amd import config                 # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.data import SyntheticMixedFeaturesDataset   # noqa: E402
from lirec_amd.test import testing           # noqa: E402


class Repeated(torch.utils.data.Dataset):
    """``n_clips`` clips that repeat the first ``unique`` samples of a synthetic dataset, drawn once"""

    def __init__(self, base, unique, n_clips):
        self.samples = [base[i] for i in range(unique)]
        self.n_clips = n_clips
        for k in ('n_classes', 'n_rels', 'rels_list', 'interidx2mgdidx'):
            setattr(self, k, getattr(base, k))

    def __len__(self):
        return self.n_clips

    def __getitem__(self, idx):
        return self.samples[idx % len(self.samples)]


def one_recipe(kind, batch_size, n_clips, unique, pairs):
    config.recipe(kind, batch_size=batch_size, num_workers=0)
    opt.device = 'cuda'
    torch.manual_seed(1)
    model, loss, _ = M.create_model(101, n_rels=15)
    ds = Repeated(SyntheticMixedFeaturesDataset(kind, unique, seed=7, soft_gt=opt.soft_gt), unique, n_clips)

    def run(on):
        opt.device_metrics = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = testing(ds, model, loss, mode='test', verbose=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert testing.last['metrics_on_device'] is on
        print('%s device_metrics=%s: %.1f clips/s' % (kind, on, n_clips / dt), file=sys.stderr, flush=True)
        return n_clips / dt, res

    results = {on: run(on)[1] for on in (True, False)}               # warm-up, and the two arms' metrics
    rate = {True: [], False: []}
    for _ in range(pairs):
        for on in (True, False):
            rate[on].append(run(on)[0])
    opt.device_metrics = True
    row = {'batch_size': batch_size, 'clips': n_clips, 'unique_samples': unique, 'batches': -(-n_clips // batch_size),
           'same_metrics': results[True] == results[False], 'arms': {}}
    for on, name in ((True, 'device'), (False, 'host')):
        v = rate[on]
        row['arms'][name] = {'clips_per_s': round(statistics.median(v), 1), 'pairs': [round(x, 1) for x in v],
                             'spread': round(max(v) - min(v), 1)}
    row['device_over_host'] = round(statistics.median(rate[True]) / statistics.median(rate[False]), 4)
    row['device_over_host_pairs'] = [round(a / b, 4) for a, b in zip(rate[True], rate[False])]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips-modalties', type=int, default=32768)
    ap.add_argument('--clips-int-rels', type=int, default=16384)
    ap.add_argument('--unique', type=int, default=256)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_clip_metrics.json'))
    a = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'pairs': a.pairs, 'num_workers': 0,
           'recipes': {'modalties': one_recipe('modalties', 64, a.clips_modalties, a.unique, a.pairs),
                       'int_rels': one_recipe('int_rels', 512, a.clips_int_rels, a.unique, a.pairs)}}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
