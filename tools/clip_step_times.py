#!/usr/bin/env python
"""The bench-shape train step with gradient clipping by global norm (``FusedAdam(max_grad_norm=...)``): what the clip costs.

Usage:  python tools/clip_step_times.py [--batch 64 --tracks 16 --ctx-clips 18 --steps 100 --rounds 3 --out profiles/clip_step.json]

Arms, on q32b feature storage: clipping off (the eager loop and the recorded step -- the headline's form), clipping on in the eager
loop, clipping on in the recorded step (lirec_amd.graph.RecordedTrainStep).  Every arm has a model of its own; the arms run
alternately in one process (``--rounds`` rounds of ``--steps`` steps each, behind bench.py's settle and warm-up counts), so that
drift of the box hits all of them.  Reported per arm: ms / step (median over the rounds), the rounds, their spread (max - min),
and the difference to the clipping-off arm of the same launch form.  With clipping on the norm pass reads the whole gradient
buffer once more, and the step gives up what needs an update before backward has finished: the first bucket's update beside the
tail of backward and, recorded, the first-layer update folded into the weight-gradient reduce.  One JSON document, printed and
written; figures only.
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

SETTLE, WARMUP = 40, 30                          # bench.py's --settle and --warmup defaults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_step.json'))
    a = ap.parse_args()
    B, T, R = a.batch, a.tracks, a.ctx_clips
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    hb = synthetic_batch(1234, 'int_rel_ch', B, T=T, R=R)
    batch = to_device_batch(hb, 'cuda', feature_dtype='q32')

    def make(clip):
        torch.manual_seed(1)
        model, loss, optim = M.create_model(101, n_rels=15)
        model.train()
        optim.max_grad_norm = clip
        return model, loss, optim

    runs, optims = {}, {}
    for arm, clip in (('clip_off', None), ('clip_on', a.max_grad_norm)):
        model, loss, optim = make(clip)

        def eager(model=model, loss=loss, optim=optim):
            optim.zero_grad()
            loss(model(dict(batch)), batch).backward()
            optim.step()
        runs[('eager', arm)], optims[('eager', arm)] = eager, optim
        model, loss, optim = make(clip)
        g = RecordedTrainStep(model, loss, optim, batch, warmup=2)
        runs[('recorded', arm)], optims[('recorded', arm)] = g.step, optim
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
           'settle_steps': SETTLE, 'warmup_steps': WARMUP, 'max_grad_norm': a.max_grad_norm,
           'device': torch.cuda.get_device_name(0), 'arms': {}}
    for launch in ('eager', 'recorded'):
        base = ms[(launch, 'clip_off')]
        res['arms'][launch] = {}
        for arm in ('clip_off', 'clip_on'):
            v = ms[(launch, arm)]
            o = optims[(launch, arm)]
            res['arms'][launch][arm] = {'ms_per_step': round(statistics.median(v), 4), 'rounds': [round(x, 4) for x in v],
                                        'spread': round(max(v) - min(v), 4),
                                        'slower_than_clip_off_by': round(statistics.median(v) - statistics.median(base), 4),
                                        'last_grad_norm': float(o.grad_norm), 'last_clip_coef': float(o.clip_coef)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
