#!/usr/bin/env python
"""Per-clip weights in the fused loss at the bench shape: what the loss launch and the whole recorded step cost without weights,
with weights, and with weights + the per-clip loss values -- and the no-weights form of a PARENT checkout beside it.

Usage:  python tools/clip_weight_times.py [--parent DIR] [--batch 64 --tracks 16 --ctx-clips 18 --steps 100 --pairs 3
                                           --launch-reps 500 --out profiles/clip_weights.json]

Every measurement runs in a fresh child process (this file with ``--child``), so that a tree's library is loaded once and alone.
``--parent DIR``: a built checkout of the parent commit; its child imports ``lirec_amd`` from DIR and measures the one form that
tree has.  Parent and this tree alternate, ``--pairs`` times; with ``--parent`` left out, this tree is measured against itself
(two arms of the same code: the spread of the box).  Per child: the loss launch alone (``ops.margin_loss``, MarginTrackRelsLoss's
arguments at B x T x 101 / 15, in-launch finalize: device events around ``--launch-reps`` back-to-back launches -- which the host's
enqueue bounds -- and the GPU time of the launch by the library's per-site events) and the recorded
train step (lirec_amd.graph.RecordedTrainStep, q32b feature storage, ms / step over ``--steps`` steps behind bench.py's settle and
warm-up counts).  One JSON document, printed and written; figures only.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTLE, WARMUP = 40, 30                          # bench.py's --settle and --warmup defaults
FORMS = ('none', 'weights', 'weights+clip_loss')


def child(a):
    sys.path.insert(0, a.root)
    import torch
    from lirec_amd import config, ops
    from lirec_amd import model as M
    from lirec_amd.config import opt
    from lirec_amd.data import synthetic_batch, to_device_batch
    from lirec_amd.graph import RecordedTrainStep
    B, T, R, C, NR = a.batch, a.tracks, a.ctx_clips, 101, 15
    forms = a.forms.split(',')
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    hb = synthetic_batch(1234, 'int_rel_ch', B, T=T, R=R)
    g = torch.Generator().manual_seed(7)
    w = (10.0 ** (6 * torch.rand(B, generator=g, dtype=torch.float64) - 3)).cuda()
    out = {'root': os.path.abspath(a.root), 'device': torch.cuda.get_device_name(0), 'forms': {}}

    # ---- the loss launch alone
    ints = torch.randn(B * T, C, generator=g).cuda()
    rels = torch.randn(B * T, NR, generator=g).cuda()
    args = (hb['mem_mask'].cuda(), hb['multilab_weights'].cuda(), hb['labels'].reshape(-1).cuda(), hb['rels_label'].cuda(),
            hb['gt_tracks'].cuda(), None, B, T, C, NR, 0.1, 0.5, False, False, True, False)
    for form in forms:
        kw = {}
        if form != 'none':
            kw = dict(clip_weight=w, clip_weight_norm='sum',
                      clip_loss=torch.empty((B, 2), device='cuda') if form.endswith('clip_loss') else None)

        def launch():
            return ops.margin_loss(ints, rels, *args, loader_types=True, **kw)
        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launch_reps):
            launch()
        t1.record()
        torch.cuda.synchronize()
        out['forms'][form] = {'loss_launch_us': round(t0.elapsed_time(t1) * 1e3 / a.launch_reps, 3)}
        # ... and the GPU time of the launch by the library's own per-site events (back-to-back launches from Python are bound by
        # the host's enqueue, the site's events are not)
        ops.profile_enable(True)
        for _ in range(a.launch_reps):
            launch()
        torch.cuda.synchronize()
        site = [v for k, v in ops.profile_read().items() if 'loss' in k.lower()]
        ops.profile_enable(False)
        out['forms'][form]['loss_site_gpu_us'] = round(sum(v['ms'] for v in site) * 1e3 / max(sum(v['launches'] for v in site), 1), 3)

    # ---- the recorded step
    for form in forms:
        batch = to_device_batch(hb, 'cuda', feature_dtype='q32')
        if form != 'none':
            batch['clip_weight'] = w.clone()
        torch.manual_seed(1)
        model, loss, optim = M.create_model(C, n_rels=NR)
        model.train()
        if form.endswith('clip_loss'):
            loss.keep_clip_losses = True
        rec = RecordedTrainStep(model, loss, optim, batch, warmup=2)
        for _ in range(SETTLE + WARMUP):
            rec.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            rec.step()
        torch.cuda.synchronize()
        out['forms'][form]['recorded_step_ms'] = round((time.perf_counter() - t0) * 1e3 / a.steps, 4)
        out['forms'][form]['recorded_commands'] = rec.cmds.size
        rec.release()
    print('CHILD ' + json.dumps(out))


def run_child(a, root, forms):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--root', root, '--forms', ','.join(forms), '--batch', str(a.batch),
           '--tracks', str(a.tracks), '--ctx-clips', str(a.ctx_clips), '--steps', str(a.steps), '--launch-reps', str(a.launch_reps)]
    r = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith('CHILD ')]
    if r.returncode != 0 or not lines:
        raise RuntimeError('child in %s failed (%d):\n%s' % (root, r.returncode, r.stdout[-3000:]))
    return json.loads(lines[-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--forms', default=','.join(FORMS))
    ap.add_argument('--parent', default=None)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--launch-reps', type=int, default=500)
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'clip_weights.json'))
    a = ap.parse_args()
    if a.child:
        return child(a)
    parent = os.path.abspath(a.parent) if a.parent else HERE
    rows = {'parent': [], 'this': []}
    for _ in range(a.pairs):
        rows['parent'].append(run_child(a, parent, ('none',)))
        rows['this'].append(run_child(a, HERE, FORMS))
    res = {'shape': {'B': a.batch, 'T': a.tracks, 'R': a.ctx_clips, 'C': 101, 'NR': 15, 'storage': 'q32b'}, 'steps': a.steps,
           'pairs': a.pairs, 'launch_reps': a.launch_reps, 'settle_steps': SETTLE, 'warmup_steps': WARMUP,
           'device': rows['this'][0]['device'], 'parent_is_this_tree': a.parent is None, 'arms': {}}

    def summary(vals):
        return {'median': round(statistics.median(vals), 4), 'pairs': vals, 'spread': round(max(vals) - min(vals), 4)}
    for arm, forms in (('parent', ('none',)), ('this', FORMS)):
        res['arms'][arm] = {f: {k: summary([r['forms'][f][k] for r in rows[arm]]) for k in ('loss_launch_us', 'loss_site_gpu_us', 'recorded_step_ms')}
                            for f in forms}
        res['arms'][arm]['recorded_commands'] = {f: rows[arm][0]['forms'][f]['recorded_commands'] for f in forms}
    base, par = res['arms']['this']['none'], res['arms']['parent']['none']
    res['unweighted_minus_parent'] = {k: round(base[k]['median'] - par[k]['median'], 4) for k in base}
    res['extra_over_unweighted'] = {f: {k: round(res['arms']['this'][f][k]['median'] - base[k]['median'], 4) for k in base}
                                    for f in FORMS[1:]}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
