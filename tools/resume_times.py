#!/usr/bin/env python
"""What ``training(resume=)`` costs: one capture + write of the rolling checkpoint at the bench model, ``training()`` clips/s with both
flags off against a checkout of the parent commit, and the same run with ``opt.checkpoint_every`` on.

Usage:  python tools/resume_times.py --parent DIR [--pairs 3 --epochs 6 --every 8 --out profiles/resume.json]

The world of ``tools/train_stepper_times.py``: the 2 048-clip pieces world of ``bench.py`` (256 scenes of 8 clips, 101 classes, 15
relationships), resident, batch 64 (32 batches an epoch), shuffled, ``int_rel_ch``, the 18.43 M parameter model; clips/s as
``training()`` prints it, the median of the epochs from the second on.  Every run is a fresh process under its own time limit.
* ``off``: parent and this tree alternating, ``--pairs`` times each.  "Off costs nothing" means this tree's median is not below
  the parent's by more than the parent's own spread (max - min of its runs); otherwise the figures say what moved.
* ``checkpoint_every``: this tree with ``opt.checkpoint_every = --every`` (``32 / every`` rolling files an epoch and one at its
  end), ``--pairs`` runs, reported as measured: no bound.
* ``capture_write``: in one process, after a few steps, ``TrainState.capture`` and ``save_checkpoint(..., atomic=True)`` of the
  rolling file, each timed by the host clock around a device synchronisation, the median of five; the file's size.
``--parent DIR``: a checkout of the parent commit; its child imports ``lirec_amd`` from DIR (the native library is the same on both
sides: a checkout without a built one loads this tree's).  One JSON document, printed and written; figures only.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, B = 18, 64


def _setup(a, store, **flags):
    import torch
    from lirec_amd import config
    from lirec_amd import features as FA
    from lirec_amd import model as M
    from lirec_amd.config import opt
    wd = FA.synthetic_world(4321, n_scenes=256, per_scene=8, n_rel_names=15, n_inter_names=101)
    ds = FA.PiecesDataset(wd, R, 101, resident=True)
    config.recipe('int_rel_ch', rels_n_clips=R, batch_size=B, num_workers=1)
    opt.device = 'cuda'
    opt.set(epochs=a.epochs, test_fr=1000, test=False, save_model=False, rels_dim=15, store_root=store, **flags)
    torch.manual_seed(1)
    return (ds,) + tuple(M.create_model(101, n_rels=15))


def child(a):
    sys.path.insert(0, a.child)
    import torch
    from lirec_amd.train import training
    with tempfile.TemporaryDirectory() as store:
        ds, model, loss, optim = _setup(a, store, **({'checkpoint_every': a.every} if a.every else {}))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            training(ds, model=model, loss=loss, optimizer=optim)
        torch.cuda.synchronize()
        written = os.path.getsize(os.path.join(store, 'last.pth.tar')) if a.every else 0
    lines = buf.getvalue().splitlines()
    rates = [float(l.split(':')[1]) for l in lines if l.startswith('train clips/s')]
    print(json.dumps({'clips_per_s': round(statistics.median(rates[1:]), 1), 'epochs': [round(r, 1) for r in rates],
                      'losses': [l.split(':')[1].strip() for l in lines if l.startswith('loss:')], 'replays': training.last['replays'],
                      'file_bytes': written, 'device': torch.cuda.get_device_name(0)}))


def capture_child(a):
    sys.path.insert(0, a.child)
    import torch
    from lirec_amd.train import TrainState
    from lirec_amd.util import Averaging, ModelSaver, save_checkpoint
    with tempfile.TemporaryDirectory() as store:
        ds, model, loss, optim = _setup(a, store)
        model.train()
        loader = torch.utils.data.DataLoader(ds, batch_size=B, collate_fn=ds.collate_fn)
        for k, batch in enumerate(loader):                # (a few real steps: the moments exist, the counters have moved)
            batch = ds.to_device(batch)
            optim.zero_grad()
            loss(model(batch), batch).backward()
            optim.step()
            if k == 3:
                break
        path, losses, saver = os.path.join(store, 'last.pth.tar'), Averaging(), ModelSaver(path=store)
        cap, wr = [], []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ts = TrainState.capture(ds, model, loss, optim, None, saver, epoch=0, batches_done=4, steps_taken=4, seen=4 * B,
                                    losses=losses, epoch_rng=torch.get_rng_state(), start='x').as_dict()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            save_checkpoint(path, 0, model, optim, train_state=ts, atomic=True)
            t2 = time.perf_counter()
            cap.append((t1 - t0) * 1e3)
            wr.append((t2 - t1) * 1e3)
        print(json.dumps({'parameters': int(sum(p.numel() for p in model.parameters())), 'capture_ms': round(statistics.median(cap), 3),
                          'write_ms': round(statistics.median(wr), 1), 'write_ms_runs': [round(x, 1) for x in wr],
                          'file_bytes': os.path.getsize(path), 'device': torch.cuda.get_device_name(0)}))


def run_child(a, root, every=0, what='--child'):
    env = dict(os.environ)
    if not os.path.exists(os.path.join(root, 'lirec_amd', 'liblirec_hip.so')):
        env['LIREC_LIB_PATH'] = os.path.join(HERE, 'lirec_amd', 'liblirec_hip.so')
    cmd = [sys.executable, os.path.abspath(__file__), what, root, '--every', str(every), '--epochs', str(a.epochs)]
    r = subprocess.run(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit('child %s every=%s ended with %d:\n%s' % (root, every, r.returncode, (r.stdout + r.stderr)[-3000:]))
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print('%s every=%d: %s' % ('parent' if root != HERE else 'this', every, row.get('epochs', row)), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--every', type=int, default=8)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'resume.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--capture-child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.capture_child:
        a.child = a.capture_child
        return capture_child(a)
    if a.child:
        return child(a)
    if not a.parent:
        raise SystemExit('--parent DIR: a checkout of the parent commit')
    parent = os.path.abspath(a.parent)
    res = {'what': 'training(): clips/s as printed, median of the epochs from the second on; one fresh process per run',
           'clips_per_epoch': 2048, 'batch_size': B, 'epochs': a.epochs, 'pairs': a.pairs}
    every = a.every
    res['capture_write'] = run_child(a, HERE, 0, '--capture-child')
    rows = {'parent': [], 'this': []}
    for _ in range(a.pairs):
        rows['parent'].append(run_child(a, parent))
        rows['this'].append(run_child(a, HERE))
    res['device'] = rows['this'][0]['device']
    v = {k: [r['clips_per_s'] for r in rows[k]] for k in rows}
    med = {k: statistics.median(v[k]) for k in v}
    spread = round(max(v['parent']) - min(v['parent']), 1)
    res['off'] = {'parent': {'runs': v['parent'], 'median': med['parent'], 'spread': spread},
                  'this': {'runs': v['this'], 'median': med['this']}, 'this_over_parent': round(med['this'] / med['parent'], 4),
                  'same_printed_losses': all(r['losses'] == rows['parent'][0]['losses'] for r in rows['parent'] + rows['this']),
                  'same_replays': all(r['replays'] == rows['parent'][0]['replays'] for r in rows['parent'] + rows['this']),
                  'inside_parent_spread': bool(med['this'] >= med['parent'] - spread)}
    on = [run_child(a, HERE, every) for _ in range(a.pairs)]
    von = [r['clips_per_s'] for r in on]
    res['checkpoint_every'] = {'every': every, 'writes_per_epoch': 32 // every + 1, 'runs': von, 'median': statistics.median(von),
                               'over_off': round(statistics.median(von) / med['this'], 4), 'file_bytes': on[0]['file_bytes'],
                               'same_printed_losses': all(r['losses'] == rows['this'][0]['losses'] for r in on)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
