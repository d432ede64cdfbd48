#!/usr/bin/env python
"""The bench-shape recorded train step with gradient accumulation (``FusedAdam(accumulate_steps=k)``): that off costs nothing, what
on costs per micro-step, and what the new launches take on their own.

Usage:  python tools/accum_step_times.py [--parent DIR] [--steps 200 --pairs 3 --out profiles/accum_steps.json]

Every figure of a recorded step comes from a PROCESS OF ITS OWN (``--arm``: one model, one RecordedTrainStep, bench.py's settle
and warm-up counts, then ``--steps`` replays timed on the host's clock behind a synchronisation); the driver starts them in turn,
``--pairs`` rounds over all arms, so that drift of the box hits every arm.  Arms, all ``int_rel_ch`` at B = 64 on q32b storage:

  off      accumulate_steps unset: the headline form (gradient-overwrite mode, folded first-layer update, deferred side join)
  plain    the same step recorded with overwrite=False and the fold off: the launch form an accumulating step has (zeroing pass,
           weight gradients accumulate, unfolded update)
  k2 k4 k8 the accumulating step: ms per MICRO-step

``--parent DIR``: a built tree of the parent commit; its ``off`` and ``plain`` arms run from its own package (``parent_off``,
``parent_plain``), alternating with this tree's.  "Off costs nothing" holds if |off - parent_off| is inside the spread of
parent_off's own runs; an accumulating micro-step is set against parent_off (ratio as measured: it gives up the overwrite mode and
the fold) and against parent_plain (it skips the zeroing pass and the update on k - 1 of k micro-steps).

The launches alone (device events around ``--launch-reps`` back-to-back launches, model-sized buffers): lirec_accum_begin on
calls that zero and on calls that do not, a held lirec_adam_step, and the ungated lirec_adam_step for scale.
One JSON document, printed and written; figures only.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTLE, WARMUP = 40, 30                          # bench.py's --settle and --warmup defaults
B, T, R = 64, 16, 18


def one_arm(arm, steps, package_root):
    """this process: the arm's recorded step, timed; prints one JSON line"""
    sys.path.insert(0, package_root)
    import torch
    from lirec_amd import config
    from lirec_amd import model as M
    from lirec_amd.config import opt
    from lirec_amd.data import synthetic_batch, to_device_batch
    from lirec_amd.graph import RecordedTrainStep
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    kw = {}
    if arm == 'plain':
        opt.fuse_dw1_adam = False
        kw['overwrite'] = False
    batch = to_device_batch(synthetic_batch(1234, 'int_rel_ch', B, T=T, R=R), 'cuda', feature_dtype='q32')
    torch.manual_seed(1)
    model, loss, optim = M.create_model(101, n_rels=15)
    model.train()
    if arm.startswith('k'):
        optim.accumulate_steps = int(arm[1:])
    g = RecordedTrainStep(model, loss, optim, batch, warmup=2, **kw)
    for _ in range(SETTLE + WARMUP):
        g.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out = {'arm': arm, 'ms_per_step': ms, 'recorded_commands': g.cmds.size,
           'flags_overwrite_fused_defer': [bool(g.overwrite), bool(g.fused), bool(g.defer)], 'adam_step': int(optim._step),
           'device': torch.cuda.get_device_name(0)}
    g.release()
    print('ARM ' + json.dumps(out))


def launches_alone(reps):
    import torch
    sys.path.insert(0, ROOT)
    from lirec_amd import config, ops
    from lirec_amd import model as M
    from lirec_amd.config import opt
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    model, _, _ = M.create_model(101, n_rels=15)
    n = model.flat_params().numel()
    p, g, m, v = (torch.zeros(n, dtype=torch.float32, device='cuda') for _ in range(4))
    ctr = torch.zeros(3, dtype=torch.int64, device='cuda')
    hyper = (3e-5, .9, .999, 1e-8, 1e-5, 1.0)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) * 1e3 / reps, 3)
    # (k = 1: every call finds phase 0, zeroes and applies; phase 1 of a window nobody closes: no call zeroes)
    win = torch.zeros(4, dtype=torch.int64, device='cuda')
    zeroing = timed(lambda: ops.accum_begin(g, ctr, [1, 0, 0], [0, 1, 1], win, 1))
    win = torch.tensor([1, 0, 0, 0], dtype=torch.int64, device='cuda')
    holding = timed(lambda: ops.accum_begin(g, ctr, [1, 0, 0], [0, 1, 1], win, 1 << 30))
    zero_count = timed(lambda: ops.zero_count(g, ctr, [1, 1]))
    counter_add = timed(lambda: ops.counter_add(ctr, [1, 1]))
    flag = torch.tensor([0, 1, 0, 0], dtype=torch.int64, device='cuda')

    def held():
        with ops.adam_hold(flag[1:2], 2):
            ops.adam_step(p, g, m, v, 1, *hyper)
    return {'flat_elements': n, 'reps': reps,
            'us_accum_begin_zeroing': zeroing, 'us_accum_begin_not_zeroing': holding, 'us_zero_count': zero_count,
            'us_counter_add': counter_add, 'us_adam_step_held': timed(held),
            'us_adam_step': timed(lambda: ops.adam_step(p, g, m, v, 1, *hyper))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm')
    ap.add_argument('--package-root', default=ROOT)
    ap.add_argument('--parent')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--launch-reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'accum_steps.json'))
    a = ap.parse_args()
    if a.arm:
        return one_arm(a.arm, a.steps, os.path.abspath(a.package_root))
    arms = [('off', ROOT), ('plain', ROOT), ('k2', ROOT), ('k4', ROOT), ('k8', ROOT)]
    if a.parent:
        parent = os.path.abspath(a.parent)
        arms = [('parent_off', parent), ('off', ROOT), ('parent_plain', parent)] + arms[1:]
    runs = {name: [] for name, _ in arms}
    for _ in range(a.pairs):
        for name, root in arms:
            cmd = [sys.executable, os.path.abspath(__file__), '--arm', name.replace('parent_', ''), '--package-root', root,
                   '--steps', str(a.steps)]
            r = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            lines = [l for l in r.stdout.splitlines() if l.startswith('ARM ')]
            if r.returncode != 0 or not lines:
                raise SystemExit('arm %s failed (exit status %d):\n%s' % (name, r.returncode, r.stdout[-3000:]))
            runs[name].append(json.loads(lines[-1][4:]))
    res = {'shape': {'recipe': 'int_rel_ch', 'B': B, 'T': T, 'R': R, 'storage': 'q32b'}, 'steps': a.steps, 'pairs': a.pairs,
           'settle_steps': SETTLE, 'warmup_steps': WARMUP, 'device': runs[arms[0][0]][0]['device'], 'arms': {}}
    med = {}
    for name, _ in arms:
        v = [x['ms_per_step'] for x in runs[name]]
        med[name] = statistics.median(v)
        res['arms'][name] = {'ms_per_step': round(med[name], 4), 'runs': [round(x, 4) for x in v], 'spread': round(max(v) - min(v), 4),
                             'recorded_commands': runs[name][0]['recorded_commands'],
                             'flags_overwrite_fused_defer': runs[name][0]['flags_overwrite_fused_defer'],
                             'adam_steps_taken': runs[name][0]['adam_step']}
    base_off, base_plain = ('parent_off', 'parent_plain') if a.parent else ('off', 'plain')
    if a.parent:
        d = med['off'] - med['parent_off']
        res['off_against_parent'] = {'difference_ms': round(d, 4), 'parent_spread_ms': res['arms']['parent_off']['spread'],
                                     'inside_parent_spread': abs(d) <= res['arms']['parent_off']['spread']}
    res['micro_step_against'] = {}
    for k in ('k2', 'k4', 'k8'):
        pairs_plain = [x['ms_per_step'] <= y['ms_per_step'] for x, y in zip(runs[k], runs[base_plain])]
        res['micro_step_against'][k] = {'ratio_to_' + base_off: round(med[k] / med[base_off], 4),
                                        'ratio_to_' + base_plain: round(med[k] / med[base_plain], 4),
                                        'not_slower_than_' + base_plain + '_in_pairs': pairs_plain}
    res['launches_alone'] = launches_alone(a.launch_reps)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
