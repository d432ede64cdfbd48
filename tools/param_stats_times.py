#!/usr/bin/env python
"""What ``FusedAdam.param_stats()`` costs at the bench model, and that the train step does not notice the feature.

Usage:  python tools/param_stats_times.py [--parent DIR --pairs 3 --steps 200 --reps 100 --out profiles/param_stats.json]

1. The headline step of THIS tree against the parent commit's (``--parent``: a checkout of it with its library built), the feature
   adding nothing to a step: ``bench.py --gpus 1 --steps K --warmup W`` (its headline leg only) as a fresh child process per run,
   the two trees alternating, ``--pairs`` pairs.  Per tree: ms / step (median), the runs, their spread (max - min); and the
   difference of the medians beside the parent's own spread.  Run first, before this process opens the GPU.  Without ``--parent``
   the section says so.
2. One ``param_stats()`` at the bench model (38 parameters in one table: all three column groups, 16 bytes per element) and one
   ``lirec_grad_sq_partials`` over the same gradient buffer (4 bytes per element), each recorded into a command list and timed as
   device events around ``--reps`` back-to-back replays behind 10 warm-up ones, in the same process: microseconds per call, bytes over time, and that as a fraction of
   the 6.29 TB/s a float4 copy reaches on this chip.  The model's buffers fit the 256 MB last-level cache in part, so the same pair
   is also timed over buffers four times as long, which do not.
3. The table of that call against float64 torch arithmetic on the same buffers (largest relative difference of the three sums,
   maxima and counts compared exactly): the one place where the kernel runs at a real model's size.
One JSON document, printed and written; figures only.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12                              # bytes / s of a float4 copy on an MI355X (measured; 79 % of the HBM3E peak)
HEADLINE_ONLY = ['--no-cpu-baseline', '--no-parity-check', '--no-profile', '--no-dense', '--no-pcie', '--no-eval', '--no-strict',
                 '--no-configs']


def bench_once(tree, steps, warmup):
    """ms / step of the headline leg of ``tree``'s bench.py, in a process of its own"""
    r = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)] +
                       HEADLINE_ONLY, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit('bench.py failed in %s (exit %d): %s' % (tree, r.returncode, r.stderr[-2000:]))
    for line in reversed(r.stdout.splitlines()):
        if line.startswith('{') and '"ms_per_step"' in line:
            return float(json.loads(line)['ms_per_step'])
    raise SystemExit('bench.py in %s printed no result line' % tree)


def step_against_parent(parent, pairs, steps, warmup):
    if not parent:
        return {'measured': False, 'why': 'no --parent tree given'}
    trees = {'parent': os.path.abspath(parent), 'this_tree': ROOT}
    ms = {k: [] for k in trees}
    for _ in range(pairs):
        for k, tree in trees.items():
            ms[k].append(bench_once(tree, steps, warmup))
            print('%s: %.4f ms / step' % (k, ms[k][-1]), file=sys.stderr, flush=True)
    out = {'measured': True, 'command': 'bench.py --gpus 1 --steps %d --warmup %d %s' % (steps, warmup, ' '.join(HEADLINE_ONLY)),
           'pairs': pairs}
    for k, v in ms.items():
        out[k] = {'ms_per_step': round(statistics.median(v), 4), 'runs': [round(x, 4) for x in v], 'spread': round(max(v) - min(v), 4)}
    out['this_tree_minus_parent_ms'] = round(out['this_tree']['ms_per_step'] - out['parent']['ms_per_step'], 4)
    out['inside_parents_spread'] = abs(out['this_tree_minus_parent_ms']) <= out['parent']['spread']
    return out


def timed(fn, reps):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def recorded(fn):
    """``fn``'s launches as a command list: the replay is a C loop, so back-to-back replays time the device, not the Python host"""
    from lirec_amd import ops
    ops.CommandList.begin()
    try:
        fn()
    finally:
        cl = ops.CommandList.end()
    return cl.replay


def rate(bytes_, us):
    r = bytes_ / (us * 1e-6)
    return {'bytes': int(bytes_), 'us_per_call': round(us, 3), 'TB_per_s': round(r / 1e12, 4), 'fraction_of_float4_copy_rate': round(r / COPY_RATE, 4)}


def against_float64(optim, stats):
    """largest relative difference of the sums; maxima and counts exact"""
    import torch
    table = stats.table.cpu()
    worst, exact = 0.0, True
    for i, (name, p) in enumerate(optim.model.named_parameters()):
        st = optim.state[p]
        grp = optim.param_groups[optim._group_of[name]]
        t = int(optim._step)
        f1, f2 = optim.stat_factors(t, *grp['betas'])
        u = (st['exp_avg'].double() * f1) / (st['exp_avg_sq'].double().sqrt() * f2 + float(torch.tensor(grp['eps'], dtype=torch.float32)))
        for k, x in enumerate((p.grad.double(), p.detach().double(), u)):
            fin = torch.isfinite(x)
            want = (float((x[fin] ** 2).sum()), float(x[fin].abs().max()) if fin.any() else 0.0, float((~fin).sum()))
            got = [float(v) for v in table[i, 3 * k:3 * k + 3]]
            if want[0]:
                worst = max(worst, abs(got[0] - want[0]) / want[0])
            exact = exact and got[1] == want[1] and got[2] == want[2]
    return {'largest_relative_difference_of_a_sum': worst, 'maxima_and_counts_equal': bool(exact)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'param_stats.json'))
    a = ap.parse_args()
    res = {'headline_step': step_against_parent(a.parent, a.pairs, a.steps, a.warmup)}

    import torch
    from lirec_amd import _lib, config, ops
    from lirec_amd import model as M
    from lirec_amd.config import opt
    from lirec_amd.data import synthetic_batch, to_device_batch
    config.recipe('int_rel_ch', rels_n_clips=18)
    opt.device = 'cuda'
    batch = to_device_batch(synthetic_batch(1234, 'int_rel_ch', 64, T=16, R=18), 'cuda', feature_dtype='q32')
    torch.manual_seed(1)
    model, loss, optim = M.create_model(101, n_rels=15)
    model.train()
    for _ in range(3):
        optim.zero_grad()
        loss(model(dict(batch)), batch).backward()
        optim.step()
    torch.cuda.synchronize()
    n_params = sum(p.numel() for p in model.parameters())
    n_flat = model.flat_params().numel()
    stats = optim.param_stats()
    res.update(device=torch.cuda.get_device_name(0), parameters=n_params, parameter_tensors=len(stats.names), flat_elements=n_flat, reps=a.reps)
    res['against_float64'] = against_float64(optim, stats)

    g = model.flat_grads(attach=True)
    partials = torch.zeros(_lib.CLIP_PARTIALS, dtype=torch.float64, device='cuda')
    ent = [(off, k, 7) + optim.stat_factors(optim._step, *optim.param_groups[0]['betas']) + (optim.param_groups[0]['eps'],)
           for off, k in (model._offsets[n] for n in stats.names)]
    out = torch.empty((len(ent), 9), dtype=torch.float64, device='cuda')
    ws = torch.empty(ops.param_stats_ws_bytes(len(ent)) // 8, dtype=torch.float64, device='cuda')
    flat = model.flat_params()
    us_stats = timed(recorded(lambda: ops.param_stats(flat, g, optim._m, optim._v, ent, out, ws)), a.reps)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int64), stats.table.view(torch.int64)), 'the timed call is not the optimiser\'s'
    us_norm = timed(recorded(lambda: ops.grad_sq_partials(g, [(0, n_flat)], partials)), a.reps)
    res['python_call_us'] = round(timed(optim.param_stats, a.reps), 3)        # (host-bound: the table is built in Python)
    res['model_sized'] = {'param_stats': rate(16.0 * n_params, us_stats), 'grad_sq_partials': rate(4.0 * n_flat, us_norm),
                          'ratio': round(us_stats / us_norm, 3)}
    # four times as long: past the last-level cache.  The same table shape (38 ranges), every range four times its length.
    n4 = 4 * n_flat
    bufs = [torch.randn(n4, dtype=torch.float32, device='cuda') * 0.01 for _ in range(3)] + [torch.rand(n4, dtype=torch.float32, device='cuda') * 1e-4]
    ent = [(4 * off, 4 * k, 7) + optim.stat_factors(3, 0.9, 0.999) + (1e-8,) for off, k in model._offsets.values()]
    us_stats4 = timed(recorded(lambda: ops.param_stats(*bufs, ent, out, ws)), a.reps)
    us_norm4 = timed(recorded(lambda: ops.grad_sq_partials(bufs[1], [(0, n4)], partials)), a.reps)
    res['four_times_that'] = {'param_stats': rate(16.0 * 4 * n_params, us_stats4), 'grad_sq_partials': rate(4.0 * n4, us_norm4),
                              'ratio': round(us_stats4 / us_norm4, 3)}
    res['float4_copy_rate_TB_per_s'] = COPY_RATE / 1e12
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
