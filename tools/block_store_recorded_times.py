#!/usr/bin/env python
"""``training()`` over a resident block store under the three values of ``opt.record_block_store`` -- '' (eager steps), 'bind' (the
recorded step, the batch written by the loader's collate call) and 'list' (the batch drawn inside the recorded list) -- and the GPU
time of one replayed step per recipe.

Usage:  python tools/block_store_recorded_times.py [--rounds 3 --epochs 3 --replays 200 --clips-modalties 16384 --clips-int-rels 1024
                                                     --clips-int-ch 1024 --unique 64 --limit 240 --out profiles/block_store_recorded.json]

``modalties``, ``int_rels`` and ``int_ch`` (T = 20) over the synthetic samples and pass lengths of tools/block_store_times.py (``--unique``
samples repeated, the real feature width, batch 64, ``opt.layer1_planes`` on).  Per recipe, in ONE process on one box: the store built
once, one warm-up ``training()`` call per arm, then ``--rounds`` rounds that alternate the three arms; an arm's figure in a round is the
median of its epochs from the second on, clips/s as ``training()`` prints it.  Then one recorded step ('bind' form, the batch bound
in place): ``--replays`` replays between two device events, microseconds per step -- the GPU time of the step when the host keeps ahead
(the figure says so: the host time of the same loop is recorded beside it).  Every recipe is measured by a child process of its own
under a time limit (``--limit`` seconds); the first one that fails or runs out ends the tool.  One JSON document, printed and
written; figures only -- what the documents recommend is decided by ``faster_than_eager_in_every_round`` / ``list_faster_than_bind_in_every_round``.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 64
ARMS = ('', 'bind', 'list')
NAMES = {'': 'eager', 'bind': 'bind', 'list': 'list'}


def measure(kind, n_clips, unique, rounds, epochs, replays):
    import torch
    from lirec_amd import config
    from lirec_amd import model as M
    from lirec_amd.blockstore import ResidentBlockDataset
    from lirec_amd.config import opt
    from lirec_amd.data import SyntheticMixedFeaturesDataset
    from lirec_amd.graph import RecordedTrainStep
    from lirec_amd.loader import BlockLoader
    from lirec_amd.train import training
    from block_store_times import Repeated

    kw = dict(T=20) if kind == 'int_ch' else {}
    config.recipe(kind, batch_size=B, num_workers=0)
    opt.device = 'cuda'
    opt.set(epochs=epochs, test_fr=1000, test=False, save_model=False, layer1_planes=True)
    base = SyntheticMixedFeaturesDataset(kind, unique, seed=7, soft_gt=opt.soft_gt, **kw)
    ds = ResidentBlockDataset(Repeated(base, unique, n_clips))
    torch.manual_seed(1)
    model, loss, optim = M.create_model(101, n_rels=15)
    rows = {'clips': n_clips, 'batch_size': B, 'steps_per_epoch': (n_clips + B - 1) // B}

    def train(arm):
        opt.record_block_store = arm
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            training(ds, model=model, loss=loss, optimizer=optim)
        torch.cuda.synchronize()
        rates = [float(l.split(':')[1]) for l in buf.getvalue().splitlines() if l.startswith('train clips/s')]
        last = training.last
        assert (last['replays'] > 0) == (arm != '') and last['input_copies'] == 0, (arm, last['replays'], last['input_copies'])
        assert (last['loader'].n_in_list > 0) == (arm == 'list'), arm
        print('%s training %r: %s' % (kind, arm, [round(r) for r in rates]), file=sys.stderr, flush=True)
        return statistics.median(rates[1:])
    for arm in ARMS:
        train(arm)                           # warm-up
    rate = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            rate[arm].append(train(arm))
    opt.record_block_store = ''
    t = {'what': 'clips/s as training() prints it, the median of the epochs from the second on; %d epochs a call; rounds alternate the arms' % epochs,
         'arms': {NAMES[a]: {'clips_per_s': round(statistics.median(v), 1), 'rounds': [round(x, 1) for x in v]} for a, v in rate.items()}}
    for a in ('bind', 'list'):
        t['%s_over_eager_rounds' % a] = [round(x / y, 3) for x, y in zip(rate[a], rate[''])]
        t['%s_faster_than_eager_in_every_round' % a] = all(x > y for x, y in zip(rate[a], rate['']))
    t['list_over_bind_rounds'] = [round(x / y, 3) for x, y in zip(rate['list'], rate['bind'])]
    t['list_faster_than_bind_in_every_round'] = all(x > y for x, y in zip(rate['list'], rate['bind']))
    rows['training'] = t
    # one replayed step: the batch stays what it is (no collate between the replays), ``replays`` of them between two device events
    model.train()
    loader = BlockLoader(ds, batch_size=B)
    layout, nbytes = loader.layout(B)
    loader.bind(layout, torch.empty(nbytes, dtype=torch.uint8, device='cuda'))
    ids = torch.randint(0, n_clips, (B,), generator=torch.Generator().manual_seed(5)).int().cuda()
    g = RecordedTrainStep(model, loss, optim, loader.collate_ids(ids, B), warmup=2)
    for _ in range(20):
        g.step()
    torch.cuda.synchronize()
    us, host_us = [], []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(replays):
            g.step()
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / replays)
        host_us.append((t1 - t0) * 1e6 / replays)
    g.release()
    rows['replayed_step'] = {'what': 'microseconds per step: %d replays of one recorded step between two device events (the GPU time of the '
                                     'step where it exceeds the host time of issuing it, recorded beside it)' % replays,
                             'overwrite': bool(g.overwrite), 'defer': bool(g.defer), 'fused': bool(g.fused),
                             'us_per_step': {'median': round(statistics.median(us), 1), 'rounds': [round(x, 1) for x in us]},
                             'host_us_per_step': {'median': round(statistics.median(host_us), 1), 'rounds': [round(x, 1) for x in host_us]}}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--clips-modalties', type=int, default=16384)
    ap.add_argument('--clips-int-rels', type=int, default=1024)
    ap.add_argument('--clips-int-ch', type=int, default=1024)
    ap.add_argument('--unique', type=int, default=64)
    ap.add_argument('--limit', type=int, default=240, help='seconds one recipe\'s child process may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'block_store_recorded.json'))
    ap.add_argument('--one', default=None, help=argparse.SUPPRESS)          # (the child: measure this recipe, print its JSON row)
    ap.add_argument('--clips', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        print('ROW ' + json.dumps(measure(a.one, a.clips, a.unique, a.rounds, a.epochs, a.replays)))
        return 0
    res = {'rounds': a.rounds, 'batch_size': B, 'rows': {}}
    for kind, n in (('modalties', a.clips_modalties), ('int_rels', a.clips_int_rels), ('int_ch', a.clips_int_ch)):
        cmd = [sys.executable, os.path.abspath(__file__), '--one', kind, '--clips', str(n), '--unique', str(a.unique), '--rounds', str(a.rounds),
               '--epochs', str(a.epochs), '--replays', str(a.replays)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print('%s: not finished inside %d s -- nothing more is started' % (kind, a.limit), file=sys.stderr)
            return 124
        row = [l for l in p.stdout.splitlines() if l.startswith('ROW ')]
        if p.returncode != 0 or not row:
            print('%s: the child ended with status %d -- nothing more is started' % (kind, p.returncode), file=sys.stderr)
            return p.returncode or 1
        res['rows'][kind] = json.loads(row[-1][4:])
    import torch
    res['device'] = torch.cuda.get_device_name(0)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
