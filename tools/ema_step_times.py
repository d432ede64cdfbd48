#!/usr/bin/env python
"""The bench-shape train step with the weight average (``FusedAdam(ema_decay=...)``): what the lerp launches cost, and what the
launch reaches on its own.

Usage:  python tools/ema_step_times.py [--batch 64 --tracks 16 --ctx-clips 18 --steps 100 --pairs 3 --out profiles/ema_ab_bench.json]

Two arms, on q32b feature storage, each in the eager loop and as a recorded step (lirec_amd.graph.RecordedTrainStep): the
average off and on.  Every arm has a model of its own; the arms run alternately in one process (``--pairs`` off / on pairs of
``--steps`` steps each, behind bench.py's settle and warm-up counts), so that drift of the box hits both.  Reported per arm:
ms / step (median over the pairs), the pairs, their spread (max - min) and the difference to the off arm of the same launch form.

The launch alone (``lirec_ema_step``, device events around ``--launch-reps`` back-to-back launches): over a buffer of the model's
flat size -- 221 MB of traffic, which the 256 MB last-level cache can hold in part -- and over one four times as long, which it
cannot; 12 bytes per element over the time, and that as a fraction of the 6.29 TB/s a float4 copy reaches on this chip.
One JSON document, printed and written; figures only.
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

from lirec_amd import config, ops             # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.data import synthetic_batch, to_device_batch   # noqa: E402
from lirec_amd.graph import RecordedTrainStep                  # noqa: E402

SETTLE, WARMUP = 40, 30                          # bench.py's --settle and --warmup defaults
COPY_RATE = 6.29e12                              # bytes / s of a float4 copy on an MI355X (measured; 79 % of the HBM3E peak)
ARMS = (('off', None), ('on', 0.999))


def launch_alone(n, reps, weight):
    e = torch.randn(n, dtype=torch.float32, device='cuda')
    p = e + 0.01 * torch.randn(n, dtype=torch.float32, device='cuda')
    for _ in range(5):
        ops.ema_step(e, p, weight)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        ops.ema_step(e, p, weight)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / reps
    rate = 12.0 * n / (us * 1e-6)
    return {'elements': n, 'bytes': 12 * n, 'us_per_launch': round(us, 3), 'TB_per_s': round(rate / 1e12, 4),
            'fraction_of_float4_copy_rate': round(rate / COPY_RATE, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--launch-reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema_ab_bench.json'))
    a = ap.parse_args()
    B, T, R = a.batch, a.tracks, a.ctx_clips
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    hb = synthetic_batch(1234, 'int_rel_ch', B, T=T, R=R)
    batch = to_device_batch(hb, 'cuda', feature_dtype='q32')

    def make(decay):
        torch.manual_seed(1)
        model, loss, optim = M.create_model(101, n_rels=15)
        model.train()
        optim.ema_decay = decay
        return model, loss, optim

    runs, optims, recs = {}, {}, {}
    for arm, decay in ARMS:
        model, loss, optim = make(decay)

        def eager(model=model, loss=loss, optim=optim):
            optim.zero_grad()
            loss(model(dict(batch)), batch).backward()
            optim.step()
        runs[('eager', arm)], optims[('eager', arm)] = eager, optim
        model, loss, optim = make(decay)
        g = RecordedTrainStep(model, loss, optim, batch, warmup=2)
        runs[('recorded', arm)], optims[('recorded', arm)], recs[arm] = g.step, optim, g
    n_flat = optims[('eager', 'off')].model.flat_params().numel()
    for fn in runs.values():
        for _ in range(SETTLE + WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.pairs):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    res = {'shape': {'B': B, 'T': T, 'R': R, 'storage': 'q32b'}, 'steps': a.steps, 'pairs': a.pairs,
           'settle_steps': SETTLE, 'warmup_steps': WARMUP, 'flat_elements': n_flat,
           'device': torch.cuda.get_device_name(0), 'arms': {}}
    for launch in ('eager', 'recorded'):
        off = ms[(launch, 'off')]
        res['arms'][launch] = {}
        for arm, decay in ARMS:
            v = ms[(launch, arm)]
            o = optims[(launch, arm)]
            row = {'ema_decay': decay, 'ms_per_step': round(statistics.median(v), 4), 'pairs': [round(x, 4) for x in v],
                   'spread': round(max(v) - min(v), 4), 'slower_than_off_by': round(statistics.median(v) - statistics.median(off), 4),
                   'ema_updates': o.ema_updates()}
            if launch == 'recorded':
                row['recorded_commands'] = recs[arm].cmds.size
                row['flags_overwrite_fused_defer'] = [bool(recs[arm].overwrite), bool(recs[arm].fused), bool(recs[arm].defer)]
            res['arms'][launch][arm] = row
    w = ops.ema_weight(0.999)
    res['launch_alone'] = {'model_sized': launch_alone(n_flat, a.launch_reps, w), 'four_times_that': launch_alone(4 * n_flat, a.launch_reps, w),
                           'float4_copy_rate_TB_per_s': COPY_RATE / 1e12}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
