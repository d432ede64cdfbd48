#!/usr/bin/env python
"""The bench-shape train step with frozen parameters (``requires_grad_(False)``): what a fine-tuning step costs.

Usage:  python tools/frozen_step_times.py [--batch 64 --tracks 16 --ctx-clips 18 --steps 100 --rounds 3 --out profiles/frozen_step.json]

Arms -- nothing frozen; both first layers frozen; the embeddings frozen (heads + gate train); heads only -- each as the eager
loop and as the recorded step (lirec_amd.graph.RecordedTrainStep), on q32b feature storage.  Every arm has a model of its own;
the arms run alternately in one process (``--rounds`` rounds of ``--steps`` steps each, behind bench.py's settle and warm-up
counts), so that drift of the box hits all of them.  Reported per arm: ms / step (median over the rounds), the rounds, and their
spread (max - min); a frozen arm issues a subset of the all-trainable arm's launches and should not be slower than it by more
than that arm's own spread -- ``slower_than_all_trainable_by`` says by how much it is.  One JSON document, printed and written.
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

from lirec_amd import config                  # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.data import synthetic_batch, to_device_batch   # noqa: E402
from lirec_amd.graph import RecordedTrainStep                  # noqa: E402

ARMS = {
    'nothing_frozen': lambda g: False,
    'both_L1_frozen': lambda g: g.startswith('L1_'),
    'embeddings_frozen': lambda g: g[:2] in ('L1', 'L2'),
    'heads_only': lambda g: not g.startswith('out_'),
}
SETTLE, WARMUP = 40, 30                          # bench.py's --settle and --warmup defaults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frozen_step.json'))
    a = ap.parse_args()
    B, T, R = a.batch, a.tracks, a.ctx_clips
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    hb = synthetic_batch(1234, 'int_rel_ch', B, T=T, R=R)
    batch = to_device_batch(hb, 'cuda', feature_dtype='q32')

    def make(arm):
        torch.manual_seed(1)
        model, loss, optim = M.create_model(101, n_rels=15)
        model.train()
        for n, p in model.named_parameters():
            p.requires_grad_(not ARMS[arm](model.param_group_of(n)))
        return model, loss, optim

    runs = {}
    for arm in ARMS:
        model, loss, optim = make(arm)

        def eager(model=model, loss=loss, optim=optim):
            optim.zero_grad()
            loss(model(dict(batch)), batch).backward()
            optim.step()
        runs[('eager', arm)] = eager
        model, loss, optim = make(arm)
        g = RecordedTrainStep(model, loss, optim, batch, warmup=2)
        runs[('recorded', arm)] = g.step
    for fn in runs.values():
        for _ in range(SETTLE + WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    res = {'shape': {'B': B, 'T': T, 'R': R, 'storage': 'q32b'}, 'steps': a.steps, 'rounds': a.rounds,
           'settle_steps': SETTLE, 'warmup_steps': WARMUP, 'device': torch.cuda.get_device_name(0), 'arms': {}}
    for launch in ('eager', 'recorded'):
        base = ms[(launch, 'nothing_frozen')]
        spread = max(base) - min(base)
        res['arms'][launch] = {}
        for arm in ARMS:
            v = ms[(launch, arm)]
            res['arms'][launch][arm] = {'ms_per_step': round(statistics.median(v), 4), 'rounds': [round(x, 4) for x in v],
                                        'spread': round(max(v) - min(v), 4),
                                        'slower_than_all_trainable_by': round(statistics.median(v) - statistics.median(base), 4),
                                        'within_all_trainable_spread': bool(statistics.median(v) - statistics.median(base) <= spread)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
