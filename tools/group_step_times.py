#!/usr/bin/env python
"""The bench-shape train step with parameter groups and device-resident hyper-parameters (``FusedAdam(param_groups=...,
device_hyper=...)``): what reading the hyper-parameters from a table in device memory costs.

Usage:  python tools/group_step_times.py [--batch 64 --tracks 16 --ctx-clips 18 --steps 100 --rounds 3 --out profiles/group_step.json]

Arms, on q32b feature storage, each in the eager loop and as a recorded step (lirec_amd.graph.RecordedTrainStep -- the headline's
form): one group by value (the code path without the feature); one group with ``device_hyper``; three groups (all biases | the
heads' and the gate's weights | the embeddings' weights); three groups with every group's learning rate rewritten in front of every
step (one lirec_adam_hyper_write per issuing stream and step).  Every arm has a model of its own; the arms run alternately in one
process (``--rounds`` rounds of ``--steps`` steps each, behind bench.py's settle and warm-up counts), so that drift of the box hits
all of them.  Reported per arm: ms / step (median over the rounds), the rounds, their spread (max - min), and the difference to the
by-value arm of the same launch form -- the yardstick is that arm of the same run, never an absolute time.  One JSON document,
printed and written; figures only.
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
from lirec_amd.optim import FusedAdam                          # noqa: E402

SETTLE, WARMUP = 40, 30                          # bench.py's --settle and --warmup defaults
ARMS = ('by_value', 'device_hyper', 'three_groups', 'three_groups_lr_every_step')


def three_groups(model):
    names = [n for n, _ in model.named_parameters()]
    heads = ('out_ints', 'out_ctx', 'gate')
    return [dict(params=[n for n in names if n.endswith('.bias')], lr=1e-3, weight_decay=0.0),
            dict(params=[n for n in names if not n.endswith('.bias') and model.param_group_of(n) in heads], lr=3e-4),
            dict(params=[n for n in names if not n.endswith('.bias') and model.param_group_of(n) not in heads], lr=1e-5, betas=(0.8, 0.99))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'group_step.json'))
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
        if arm == 'device_hyper':
            optim = FusedAdam(model, lr=opt.lr, weight_decay=opt.weight_decay, device_hyper=True)
        elif arm != 'by_value':
            optim = FusedAdam(model, lr=opt.lr, weight_decay=opt.weight_decay, param_groups=three_groups(model))
        return model, loss, optim

    def rewriting(fn, optim):
        base, k = [g['lr'] for g in optim.param_groups], [0]

        def step():
            k[0] += 1
            for g, b in zip(optim.param_groups, base):
                g['lr'] = b * (1.0 - 1e-3 * (k[0] % 7))
            fn()
        return step

    runs, info = {}, {}
    for arm in ARMS:
        model, loss, optim = make(arm)

        def eager(model=model, loss=loss, optim=optim):
            optim.zero_grad()
            loss(model(dict(batch)), batch).backward()
            optim.step()
        runs[('eager', arm)] = rewriting(eager, optim) if arm.endswith('every_step') else eager
        model, loss, optim = make(arm)
        g = RecordedTrainStep(model, loss, optim, batch, warmup=2)
        runs[('recorded', arm)] = rewriting(g.step, optim) if arm.endswith('every_step') else g.step
        info[arm] = {'groups': len(optim.param_groups), 'device_hyper': bool(optim.device_hyper), 'recorded_commands': g.cmds.size,
                     'recorded_form': {'overwrite': bool(g.overwrite), 'fused_first_layer_update': bool(g.fused), 'deferred_side_join': bool(g.defer)},
                     'tables': sorted(optim._tables)}
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
           'settle_steps': SETTLE, 'warmup_steps': WARMUP, 'device': torch.cuda.get_device_name(0), 'arms_info': info, 'arms': {}}
    for launch in ('eager', 'recorded'):
        base = ms[(launch, 'by_value')]
        res['arms'][launch] = {}
        for arm in ARMS:
            v = ms[(launch, arm)]
            res['arms'][launch][arm] = {'ms_per_step': round(statistics.median(v), 4), 'rounds': [round(x, 4) for x in v],
                                        'spread': round(max(v) - min(v), 4),
                                        'slower_than_by_value_by': round(statistics.median(v) - statistics.median(base), 4)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
