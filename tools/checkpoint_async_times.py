#!/usr/bin/env python
"""What ``opt.checkpoint_async`` costs and buys: ``training()`` clips/s with the rolling checkpoint written synchronously and behind
the steps, the host time of one ``AsyncCheckpointer.save()`` against one synchronous write, and the snapshot launch itself.

Usage:  python tools/checkpoint_async_times.py --parent DIR [--rounds 3 --epochs 6 --every 8 --out profiles/checkpoint_async.json]

The setting of ``tools/resume_times.py``: the 2 048-clip pieces world of ``bench.py``, resident, batch 64 (32 steps an epoch),
shuffled, ``int_rel_ch``, the 18.43 M parameter model; clips/s as ``training()`` prints it, the median of the epochs from the
second on; every run a fresh process under its own time limit; ``--rounds`` rounds with the arms in turn.
* ``off``: no rolling file -- the parent's build and this tree.  "Off costs nothing": this tree's median is not below the
  parent's by more than the parent's own spread (max - min of its runs).
* ``every``: ``checkpoint_every = --every`` -- the parent's build (synchronous), this tree with the flag off, this tree with it on.
* ``per_epoch``: ``checkpoint_every`` larger than an epoch, i.e. ONE WRITE PER 32 STEPS (the epoch's end always writes): the widest
  spacing this setting has -- NOT one write per thousand steps, which ``training()`` cannot be asked for while an epoch is 32
  steps.  The same three arms.
Every arm carries two figures: the printed clips/s (an epoch's steps and the writes inside it) and ``wall``: clips over the
host clock from the second epoch's first line to the drained end of ``training()``, which has the writes at the epochs' ends
too.  The comparisons (``*_over_*``, ``faster_in_every_pair``) are taken on ``wall``.
* ``save``: in one process after a few steps, the host time of ``save()`` (median of ``--saves``, the first -- which allocates arena
  and pinned memory -- apart), of the parent-style synchronous capture + write, the writer's time, and clips/s of eager steps
  with a write in flight against none (what the writer's share of the interpreter lock costs the loop).
* ``snapshot``: device events around ``--reps`` back-to-back ``lirec_snapshot`` launches over the model's three flat buffers, beside
  torch ``copy_`` of the same buffers in the same run: microseconds, GB/s read plus written.
``--parent DIR``: a checkout of the parent commit with its own build.  One JSON document, printed and written; figures only."""
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
    flags = {'checkpoint_every': a.every} if a.every else {}
    if a.async_on:
        flags['checkpoint_async'] = True
    with tempfile.TemporaryDirectory() as store:
        ds, model, loss, optim = _setup(a, store, **flags)
        buf = _Stamped()
        with contextlib.redirect_stdout(buf):
            training(ds, model=model, loss=loss, optimizer=optim)
        torch.cuda.synchronize()
        t_end = time.perf_counter()
        written = os.path.getsize(os.path.join(store, 'last.pth.tar')) if a.every else 0
    lines = buf.getvalue().splitlines()
    rates = [float(l.split(':')[1]) for l in lines if l.startswith('train clips/s')]
    last = training.last
    # (the printed figure times an epoch's steps and the writes INSIDE it; the write at an epoch's end falls between two printed
    #  figures -- the wall clock from the second epoch's first line to the drained end of training() has both)
    wall = (a.epochs - 1) * 2048 / (t_end - buf.at['Epoch # 1'])
    print(json.dumps({'clips_per_s': round(statistics.median(rates[1:]), 1), 'wall_clips_per_s': round(wall, 1),
                      'epochs': [round(r, 1) for r in rates],
                      'losses': [l.split(':')[1].strip() for l in lines if l.startswith('loss:')], 'replays': last['replays'],
                      'file_bytes': written, 'writes': last.get('checkpoint_writes'), 'waits': last.get('checkpoint_waits'),
                      'save_s': None if last.get('checkpoint_save_s') is None else round(last['checkpoint_save_s'], 5),
                      'device': torch.cuda.get_device_name(0)}))


class _Stamped(io.StringIO):
    """stdout kept, with the host clock at the first write of every 'Epoch # n' line"""
    def __init__(self):
        super().__init__()
        self.at = {}

    def write(self, text):
        if text.startswith('Epoch # '):
            self.at.setdefault(text.strip(), time.perf_counter())
        return super().write(text)


def _steps(ds, model, loss, optim, n):
    import torch
    loader = torch.utils.data.DataLoader(ds, batch_size=B, collate_fn=ds.collate_fn)
    batches = []
    for k, batch in enumerate(loader):
        batches.append(ds.to_device(batch))
        if k + 1 == n:
            break

    def step(batch):
        optim.zero_grad()
        loss(model(batch), batch).backward()
        optim.step()
    return batches, step


def save_child(a):
    sys.path.insert(0, a.child)
    import torch
    from lirec_amd.train import TrainState
    from lirec_amd.util import AsyncCheckpointer, Averaging, ModelSaver, save_checkpoint
    with tempfile.TemporaryDirectory() as store:
        ds, model, loss, optim = _setup(a, store)
        model.train()
        batches, step = _steps(ds, model, loss, optim, 4)
        for b in batches:
            step(b)
        path, losses, saver = os.path.join(store, 'last.pth.tar'), Averaging(), ModelSaver(path=store)

        def capture(device_reads):
            return TrainState.capture(ds, model, loss, optim, None, saver, epoch=0, batches_done=4, steps_taken=4, seen=4 * B,
                                      losses=losses, epoch_rng=torch.get_rng_state(), start='x', device_reads=device_reads).as_dict()
        sync = []
        for _ in range(a.saves):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            save_checkpoint(path, 0, model, optim, train_state=capture(True), atomic=True)
            sync.append((time.perf_counter() - t0) * 1e3)
        ck = AsyncCheckpointer(model, optim)
        host, writer = [], []
        for _ in range(a.saves + 1):
            torch.cuda.synchronize()
            w0 = ck.stats['writer_s']
            t0 = time.perf_counter()
            ck.save(path, 0, capture(False))
            host.append((time.perf_counter() - t0) * 1e3)
            ck.wait()
            writer.append((ck.stats['writer_s'] - w0) * 1e3)
        # eager steps with a write in flight against none: the same steps, timed by the host clock around a synchronisation
        def rate(in_flight, steps=8):
            n, t = 0, 0.0
            for _ in range(a.saves):
                torch.cuda.synchronize()
                if in_flight:
                    ck.save(path, 0, capture(False))
                t0 = time.perf_counter()
                k = 0
                while k < steps or (in_flight and ck._thread is not None and ck._thread.is_alive() and k < 1000):
                    step(batches[k % len(batches)])
                    k += 1
                torch.cuda.synchronize()
                t += time.perf_counter() - t0
                n += k
                ck.wait()
            return n * B / t, n
        busy, nb = rate(True)                             # (as many steps as the write lasts ...
        quiet, nq = rate(False, max(8, nb // a.saves))    #  ... and the same number with none in flight)
        arena = ck._arena.numel()
        pinned = sum(h.numel() * h.element_size() for h in ck._host.values())
        ck.close()
        print(json.dumps({'parameters': int(sum(p.numel() for p in model.parameters())),
                          'sync_capture_write_ms': round(statistics.median(sync), 1), 'sync_runs_ms': [round(x, 1) for x in sync],
                          'first_save_ms': round(host[0], 2), 'save_ms': round(statistics.median(host[1:]), 3),
                          'save_runs_ms': [round(x, 3) for x in host[1:]], 'writer_ms': round(statistics.median(writer[1:]), 1),
                          'writer_runs_ms': [round(x, 1) for x in writer[1:]],
                          'eager_clips_per_s_no_write': round(quiet, 1), 'eager_clips_per_s_write_in_flight': round(busy, 1),
                          'eager_steps_timed': [nq, nb], 'in_flight_over_none': round(busy / quiet, 4),
                          'arena_bytes': arena, 'pinned_bytes': pinned, 'file_bytes': os.path.getsize(path),
                          'device': torch.cuda.get_device_name(0)}))


def snapshot_child(a):
    sys.path.insert(0, a.child)
    import torch
    from lirec_amd import ops
    with tempfile.TemporaryDirectory() as store:
        ds, model, loss, optim = _setup(a, store)
        model.train()
        batches, step = _steps(ds, model, loss, optim, 2)
        for b in batches:
            step(b)
        src = [model.flat_params().detach(), optim._m, optim._v]
        dst = [torch.empty_like(s) for s in src]
        dig = torch.zeros(8, dtype=torch.int64, device='cuda')
        nbytes = sum(s.numel() * 4 for s in src)

        def timed(fn):
            for _ in range(10):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e3 / a.reps

        def copies():
            for s, d in zip(src, dst):
                d.copy_(s)
        rows = {}
        for round_ in range(3):
            rows.setdefault('snapshot_us', []).append(round(timed(lambda: ops.snapshot(list(zip(src, dst)), dig)), 2))
            rows.setdefault('torch_copy_us', []).append(round(timed(copies), 2))
        ok = all(torch.equal(s, d) for s, d in zip(src, dst))
        out = {'ranges': 3, 'bytes_copied': nbytes, 'reps': a.reps, 'copies_equal': ok}
        for k, v in rows.items():
            med = statistics.median(v)
            out[k] = med
            out[k + '_runs'] = v
            out[k.replace('_us', '_GBps_read_plus_written')] = round(2 * nbytes / med / 1e3, 1)
        out['device'] = torch.cuda.get_device_name(0)
        print(json.dumps(out))


def run_child(a, root, every=0, async_on=False, what='--child'):
    env = dict(os.environ)
    if not os.path.exists(os.path.join(root, 'lirec_amd', 'liblirec_hip.so')):
        raise SystemExit('%s holds no built library: build the parent checkout first (its own build is the yardstick)' % root)
    cmd = [sys.executable, os.path.abspath(__file__), what, root, '--every', str(every), '--epochs', str(a.epochs),
           '--saves', str(a.saves), '--reps', str(a.reps)] + (['--async-on'] if async_on else [])
    r = subprocess.run(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit('child %s %s every=%s async=%s ended with %d:\n%s' % (what, root, every, async_on, r.returncode, (r.stdout + r.stderr)[-3000:]))
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print('%s %s every=%d async=%s: %s' % (what, 'parent' if root != HERE else 'this', every, async_on, row.get('epochs', row)),
          file=sys.stderr, flush=True)
    return row


def _arm(rows):
    v, w = [r['clips_per_s'] for r in rows], [r['wall_clips_per_s'] for r in rows]
    out = {'runs': v, 'median': statistics.median(v), 'spread': round(max(v) - min(v), 1),
           'wall_runs': w, 'wall_median': statistics.median(w), 'wall_spread': round(max(w) - min(w), 1)}
    if rows[0].get('writes') is not None:
        out.update(writes=[r['writes'] for r in rows], waits=[r['waits'] for r in rows], save_s=[r['save_s'] for r in rows])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--every', type=int, default=8)
    ap.add_argument('--saves', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'checkpoint_async.json'))
    ap.add_argument('--async-on', action='store_true', help=argparse.SUPPRESS)
    for name in ('--child', '--save-child', '--snapshot-child'):
        ap.add_argument(name, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    for name, fn in (('save_child', save_child), ('snapshot_child', snapshot_child), ('child', child)):
        if getattr(a, name):
            a.child = getattr(a, name)
            return fn(a)
    if not a.parent:
        raise SystemExit('--parent DIR: a checkout of the parent commit, built')
    parent = os.path.abspath(a.parent)
    res = {'what': 'training(): clips/s as printed, median of the epochs from the second on; one fresh process per run; the arms in turn',
           'clips_per_epoch': 2048, 'batch_size': B, 'steps_per_epoch': 2048 // B, 'epochs': a.epochs, 'rounds': a.rounds}
    res['snapshot'] = run_child(a, HERE, what='--snapshot-child')
    res['save'] = run_child(a, HERE, what='--save-child')
    sparse = 1000
    arms = {'off/parent': (parent, 0, False), 'off/this': (HERE, 0, False),
            'every/parent': (parent, a.every, False), 'every/this_flag_off': (HERE, a.every, False), 'every/this_flag_on': (HERE, a.every, True),
            'per_epoch/parent': (parent, sparse, False), 'per_epoch/this_flag_off': (HERE, sparse, False), 'per_epoch/this_flag_on': (HERE, sparse, True)}
    rows = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (root, every, on) in arms.items():
            rows[k].append(run_child(a, root, every, on))
    res['device'] = rows['off/this'][0]['device']
    for group in ('off', 'every', 'per_epoch'):
        res[group] = {k.split('/')[1]: _arm(v) for k, v in rows.items() if k.startswith(group + '/')}
    off = res['off']
    off['this_over_parent'] = round(off['this']['median'] / off['parent']['median'], 4)
    off['inside_parent_spread'] = bool(off['this']['median'] >= off['parent']['median'] - off['parent']['spread'])
    off['wall_this_over_parent'] = round(off['this']['wall_median'] / off['parent']['wall_median'], 4)
    off['wall_inside_parent_spread'] = bool(off['this']['wall_median'] >= off['parent']['wall_median'] - off['parent']['wall_spread'])
    off['same_printed_losses'] = all(r['losses'] == rows['off/parent'][0]['losses'] for k in rows for r in rows[k])
    for group, every in (('every', a.every), ('per_epoch', sparse)):
        g = res[group]
        g['checkpoint_every'] = every
        g['writes_per_epoch'] = (2048 // B) // every + 1
        g['steps_per_write'] = round((2048 // B) / g['writes_per_epoch'], 1)
        g['flag_off_over_parent'] = round(g['this_flag_off']['wall_median'] / g['parent']['wall_median'], 4)
        g['flag_off_inside_parent_spread'] = bool(g['this_flag_off']['wall_median'] >= g['parent']['wall_median'] - g['parent']['wall_spread'])
        g['flag_on_over_parent'] = round(g['this_flag_on']['wall_median'] / g['parent']['wall_median'], 4)
        g['flag_on_over_no_checkpoint'] = round(g['this_flag_on']['wall_median'] / off['this']['wall_median'], 4)
        g['parent_over_no_checkpoint'] = round(g['parent']['wall_median'] / off['parent']['wall_median'], 4)
        g['flag_on_faster_in_every_pair'] = all(x > y for x, y in zip(g['this_flag_on']['wall_runs'], g['parent']['wall_runs']))
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
