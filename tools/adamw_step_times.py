#!/usr/bin/env python
"""The bench-shape train step with decoupled weight decay (AdamW, ``FusedAdam(decoupled_weight_decay=...)``) and with the usual
AdamW grouping -- the weights decay, the biases do not --: what the flag costs, and whether the grouping keeps the folded
first-layer update.

Usage:  python tools/adamw_step_times.py [--batch 64 --tracks 16 --ctx-clips 18 --steps 100 --rounds 3 --out profiles/adamw_step.json]

Arms, on q32b feature storage, each in the eager loop and as a recorded step (lirec_amd.graph.RecordedTrainStep -- the headline's
form): (a) one group, coupled, by value (the code path without the feature); (b) one group, decoupled (the table route: the flag
needs it); (c) weights | biases as two groups, coupled, the biases without decay; (d) the same, the weights decoupled.  Every arm
has a model of its own; the arms run alternately in one process (``--rounds`` rounds of ``--steps`` steps each, behind bench.py's
settle and warm-up counts), so that drift of the box hits all of them.  Reported per arm: ms / step (median over the rounds), the
rounds, their spread (max - min), the difference to arm (a) of the same launch form and, for (b) and (d), to the coupled arm with
the same groups -- the yardstick is an arm of the same run, never an absolute time -- and whether the recorded step folded the
first-layer update in.  One JSON document, printed and written; figures only.
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
ARMS = ('a_one_group_coupled_by_value', 'b_one_group_decoupled', 'c_two_groups_coupled', 'd_two_groups_decoupled')
COUPLED_TWIN = {'b_one_group_decoupled': 'a_one_group_coupled_by_value', 'd_two_groups_decoupled': 'c_two_groups_coupled'}
WD = 1e-2


def two_groups(model, decoupled):
    names = [n for n, _ in model.named_parameters()]
    return [dict(params=[n for n in names if not n.endswith('.bias')], weight_decay=WD, decoupled_weight_decay=decoupled),
            dict(params=[n for n in names if n.endswith('.bias')], weight_decay=0.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adamw_step.json'))
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
        if arm.startswith(('a_', 'b_')):
            optim = FusedAdam(model, lr=opt.lr, weight_decay=WD, decoupled_weight_decay=arm.startswith('b_'))
        else:
            optim = FusedAdam(model, lr=opt.lr, param_groups=two_groups(model, arm.startswith('d_')))
        return model, loss, optim

    runs, info = {}, {}
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
        info[arm] = {'groups': len(optim.param_groups), 'device_hyper': bool(optim.device_hyper), 'decoupled': [bool(r[5]) for r in optim.hyper_rows()], 'recorded_commands': g.cmds.size,
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
        base = ms[(launch, ARMS[0])]
        res['arms'][launch] = {}
        for arm in ARMS:
            v = ms[(launch, arm)]
            res['arms'][launch][arm] = {'ms_per_step': round(statistics.median(v), 4), 'rounds': [round(x, 4) for x in v],
                                        'spread': round(max(v) - min(v), 4),
                                        'slower_than_by_value_by': round(statistics.median(v) - statistics.median(base), 4)}
            if arm in COUPLED_TWIN:
                res['arms'][launch][arm]['slower_than_coupled_twin_by'] = round(statistics.median(v) - statistics.median(ms[(launch, COUPLED_TWIN[arm])]), 4)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
