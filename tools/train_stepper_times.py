#!/usr/bin/env python
"""``lirec_amd.train.training()`` of this tree against a checkout of the parent commit: the loop is host-bound, so moving its
decision state into one object must not cost it clips/s.

Usage:  python tools/train_stepper_times.py --parent DIR [--pairs 3 --epochs 8 --out profiles/train_stepper_ab.json]

The world of ``tools/device_collate_times.py``: the 2 048-clip pieces world of ``bench.py`` (256 scenes of 8 clips, 101 classes, 15
relationships), resident, batch 64, shuffled, ``int_rel_ch``; clips/s as ``training()`` prints it, the median of the epochs from the
second on.  With ``opt.device_collate`` off and on: parent and this tree alternating, ``--pairs`` times each, every run a fresh
process under its own time limit that only calls ``training()``.  ``--parent DIR``: a checkout of the parent commit; its child imports
``lirec_amd`` from DIR (the native library is the same on both sides: a checkout without a built one loads this tree's).  This tree
passes an arm when its median over the runs is not below the parent's median by more than the parent's own spread (max - min of
its runs).  One JSON document, printed and written; figures only.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, B = 18, 64


def child(a):
    sys.path.insert(0, a.child)
    import torch
    from lirec_amd import config
    from lirec_amd import features as FA
    from lirec_amd import model as M
    from lirec_amd.config import opt
    from lirec_amd.train import training
    wd = FA.synthetic_world(4321, n_scenes=256, per_scene=8, n_rel_names=15, n_inter_names=101)
    ds = FA.PiecesDataset(wd, R, 101, resident=True)
    config.recipe('int_rel_ch', rels_n_clips=R, batch_size=B, num_workers=1)
    opt.device = 'cuda'
    opt.set(epochs=a.epochs, test_fr=1000, test=False, save_model=False, rels_dim=15, device_collate=bool(a.device_collate))
    torch.manual_seed(1)
    model, loss, optim = M.create_model(101, n_rels=15)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        training(ds, model=model, loss=loss, optimizer=optim)
    torch.cuda.synchronize()
    lines = buf.getvalue().splitlines()
    rates = [float(l.split(':')[1]) for l in lines if l.startswith('train clips/s')]
    last = training.last
    assert last['replays'] > 0 and (last['input_copies'] == 0) == bool(a.device_collate), last
    print(json.dumps({'clips_per_s': round(statistics.median(rates[1:]), 1), 'epochs': [round(r, 1) for r in rates],
                      'losses': [l.split(':')[1].strip() for l in lines if l.startswith('loss:')],
                      'replays': last['replays'], 'input_copies': last['input_copies'], 'device': torch.cuda.get_device_name(0)}))


def run_child(a, root, flag):
    env = dict(os.environ)
    if not os.path.exists(os.path.join(root, 'lirec_amd', 'liblirec_hip.so')):
        env['LIREC_LIB_PATH'] = os.path.join(HERE, 'lirec_amd', 'liblirec_hip.so')
    cmd = [sys.executable, os.path.abspath(__file__), '--child', root, '--device-collate', str(int(flag)), '--epochs', str(a.epochs)]
    r = subprocess.run(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit('child %s flag=%s ended with %d:\n%s' % (root, flag, r.returncode, (r.stdout + r.stderr)[-3000:]))
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print('%s device_collate=%d: %s' % ('parent' if root != HERE else 'this', flag, row['epochs']), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'train_stepper_ab.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--device-collate', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent:
        raise SystemExit('--parent DIR: a checkout of the parent commit')
    parent = os.path.abspath(a.parent)
    res = {'what': 'training(): clips/s as printed, median of the epochs from the second on; one fresh process per run, parent and '
                   'this tree alternating', 'clips_per_epoch': 2048, 'batch_size': B, 'epochs': a.epochs, 'pairs': a.pairs, 'arms': {}}
    for flag, name in ((False, 'device_collate_off'), (True, 'device_collate_on')):
        rows = {'parent': [], 'this': []}
        for _ in range(a.pairs):
            rows['parent'].append(run_child(a, parent, flag))
            rows['this'].append(run_child(a, HERE, flag))
        res['device'] = rows['this'][0]['device']
        v = {k: [r['clips_per_s'] for r in rows[k]] for k in rows}
        med = {k: statistics.median(v[k]) for k in v}
        spread = round(max(v['parent']) - min(v['parent']), 1)
        res['arms'][name] = {'parent': {'runs': v['parent'], 'median': med['parent'], 'spread': spread, 'epochs': [r['epochs'] for r in rows['parent']]},
                             'this': {'runs': v['this'], 'median': med['this'], 'epochs': [r['epochs'] for r in rows['this']]},
                             'this_over_parent': round(med['this'] / med['parent'], 4),
                             'same_printed_losses': all(r['losses'] == rows['parent'][0]['losses'] for r in rows['parent'] + rows['this']),
                             'same_counters': all((r['replays'], r['input_copies']) == (rows['parent'][0]['replays'], rows['parent'][0]['input_copies'])
                                                  for r in rows['parent'] + rows['this']),
                             'passes': bool(med['this'] >= med['parent'] - spread)}
    res['verdict'] = 'pass' if all(arm['passes'] for arm in res['arms'].values()) else 'fail'
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
