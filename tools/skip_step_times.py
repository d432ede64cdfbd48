#!/usr/bin/env python
"""The bench-shape train step with the non-finite-step guard (``FusedAdam(skip_nonfinite=True)``): what the guard costs.

Usage:  python tools/skip_step_times.py [--batch 64 --tracks 16 --ctx-clips 18 --steps 100 --rounds 3 --out profiles/skip_step.json]

Four arms, on q32b feature storage, each in the eager loop and as a recorded step (lirec_amd.graph.RecordedTrainStep): everything
off, ``max_grad_norm`` only, the guard only, both.  Every arm has a model of its own; the arms run alternately in one process
(``--rounds`` rounds of ``--steps`` steps each, behind bench.py's settle and warm-up counts), so that drift of the box hits all of
them.  Reported per arm: ms / step (median over the rounds), the rounds, their spread (max - min), the difference to the
everything-off arm and -- THE YARDSTICK OF THE GUARD -- to the clipping-only arm of the same launch form: the guard takes the
clipped route (the norm pass over the gradient buffer, the whole update behind backward, no folded first-layer update) and adds
one one-workgroup launch to it.  Every gradient is finite here: no step is skipped (``skipped_steps`` is reported).  One JSON
document, printed and written; figures only.
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
ARMS = (('off', False, False), ('clip_only', True, False), ('guard_only', False, True), ('both', True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skip_step.json'))
    a = ap.parse_args()
    B, T, R = a.batch, a.tracks, a.ctx_clips
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    hb = synthetic_batch(1234, 'int_rel_ch', B, T=T, R=R)
    batch = to_device_batch(hb, 'cuda', feature_dtype='q32')

    def make(clip, guard):
        torch.manual_seed(1)
        model, loss, optim = M.create_model(101, n_rels=15)
        model.train()
        optim.max_grad_norm = a.max_grad_norm if clip else None
        optim.skip_nonfinite = guard
        return model, loss, optim

    runs, optims = {}, {}
    for arm, clip, guard in ARMS:
        model, loss, optim = make(clip, guard)

        def eager(model=model, loss=loss, optim=optim):
            optim.zero_grad()
            loss(model(dict(batch)), batch).backward()
            optim.step()
        runs[('eager', arm)], optims[('eager', arm)] = eager, optim
        model, loss, optim = make(clip, guard)
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
        off, clip_only = ms[(launch, 'off')], ms[(launch, 'clip_only')]
        res['arms'][launch] = {}
        for arm, clip, guard in ARMS:
            v = ms[(launch, arm)]
            o = optims[(launch, arm)]
            row = {'ms_per_step': round(statistics.median(v), 4), 'rounds': [round(x, 4) for x in v], 'spread': round(max(v) - min(v), 4),
                   'slower_than_off_by': round(statistics.median(v) - statistics.median(off), 4),
                   'slower_than_clip_only_by': round(statistics.median(v) - statistics.median(clip_only), 4)}
            if clip or guard:
                row['last_grad_norm'], row['last_clip_coef'] = float(o.grad_norm), float(o.clip_coef)
            if guard:
                row['skipped_steps'], row['last_found_nonfinite'] = int(o.skipped_steps), float(o.found_nonfinite)
            res['arms'][launch][arm] = row
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
