#!/usr/bin/env python
"""Train-mode context sampling (``PiecesDataset(context_draw='random')``, ``lirec_draw_context``): what the per-epoch draw costs.

Usage:  python tools/context_draw_times.py [--pairs 3 --epochs 8 --launches 20 --samples 16384 --slots-per-sample 2 --max-len 512
                                            --strided-only --parent FILE --out profiles/context_draw.json]

1. The launch: synthetic tables of ``--samples`` samples, T = 20, R = 18, ``--slots-per-sample`` slots a sample at random
   candidates, list lengths uniform in [19, ``--max-len``]; ``--launches`` back-to-back ``ops.draw_context`` calls between two device
   events, the median of ``--pairs`` rounds, microseconds per call (launch overhead included).  Beside it, measured the same way
   in the same process, one ``ops.collate_resident`` call at batch 64 over the training world below.
2. ``training()``: ``int_rel_ch`` over a resident store with ``opt.device_collate`` on, the 2 048-clip pieces world of ``bench.py``
   (256 scenes of 8 clips, 101 classes, 15 relationships: 4 836 over-long lists at R = 18, the longest of 111 clips), batch 64,
   shuffled; ``'strided'`` against ``'random'``, one warm-up per arm, then ``--pairs`` alternating pairs in one process; clips/s as
   ``training()`` prints it, the median of the epochs from the second on.
3. ``'strided'`` against the parent commit: ``--strided-only`` runs arm ``'strided'`` alone and constructs the dataset without the
   new arguments, so the same file runs in a checkout of the parent; ``--parent FILE`` reads such a run's output and puts its
   figures beside this run's.  (Two processes, one after the other on one box: their difference includes what two runs of the
   same code differ by.)
One JSON document, printed and written; figures only.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lirec_amd import config, ops            # noqa: E402
from lirec_amd import features as FA         # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.train import training         # noqa: E402

R, B, T = 18, 64, 20


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches              # microseconds per call


def rounds(fn, launches, pairs):
    timed(fn, launches)
    us = [timed(fn, launches) for _ in range(pairs)]
    return {'median': round(statistics.median(us), 2), 'rounds': [round(x, 2) for x in us]}


def launch_row(a):
    rng = np.random.Generator(np.random.PCG64(7))
    N, S = a.samples, a.samples * a.slots_per_sample
    cand = np.stack([rng.permutation(T)[:a.slots_per_sample] for _ in range(N)])
    slots = (np.arange(N)[:, None] * T + cand).reshape(-1)
    lens = rng.integers(R + 1, a.max_len + 1, size=S)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pool = rng.integers(-1, 100000, size=(int(off[-1]), 3), dtype=np.int32)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dst, offd, poold = up(slots.astype(np.int32)), up(off), up(pool)
    table = torch.full((N, T, R + 1, 3), -1, dtype=torch.int32, device='cuda')
    epoch = [0]

    def call():
        epoch[0] += 1
        ops.draw_context(dst, offd, poold, table, R, 0x5eed00000007, epoch[0])
    row = {'samples': N, 'T': T, 'R': R, 'slots': S, 'pool_entries': int(off[-1]), 'longest_list': int(lens.max()), 'launches': a.launches,
           'what': 'microseconds per call, back-to-back calls between two device events (launch overhead included; one launch a call)',
           'us_per_call': rounds(call, a.launches, a.pairs)}
    # (against the CPU statement, once: the figure is of a launch that computes the rule)
    want = FA.draw_context(slots.astype(np.int32), off, pool, np.full((N, T, R + 1, 3), -1, dtype=np.int32), R, 0x5eed00000007, epoch[0])
    row['equals_the_cpu_statement'] = bool(np.array_equal(table.cpu().numpy(), want))
    return row


def collate_row(ds, a):
    from lirec_amd.loader import ResidentLoader
    tabs = ds.device_tables('cuda')
    layout, nbytes = ResidentLoader(ds, batch_size=B).layout(B)
    ids = torch.randint(0, len(ds), (B,), generator=torch.Generator().manual_seed(5)).int().cuda()
    view = FA.layout_views(torch.empty(nbytes, dtype=torch.uint8, device='cuda'), layout)
    ws = ops.collate_workspace(*tabs['n_all'], 'cuda')
    counts = torch.empty(2, dtype=torch.int32, device='cuda')
    fields = [(tabs[k], view[k]) for k in FA._FIELDS]
    call = lambda: ops.collate_resident(ids, tabs['index_rows'], tabs['n_all'][0], tabs['n_all'][1], view['feature_index'],
                                        view['clip_rows'], view['track_rows'], counts, fields, ws)
    return {'batch_size': B, 'launches': 200, 'what': 'one ops.collate_resident call over the training world, measured the same way (four commands)',
            'us_per_call': rounds(call, 200, a.pairs)}


def train_rows(world, arms, a):
    config.recipe('int_rel_ch', rels_n_clips=R, batch_size=B, num_workers=1)
    opt.device = 'cuda'
    opt.set(epochs=a.epochs, test_fr=1000, test=False, save_model=False, rels_dim=len(world.rel_names), device_collate=True)
    torch.manual_seed(1)
    model, loss, optim = M.create_model(101, n_rels=len(world.rel_names))
    # ('strided' without the new arguments: the same call in a checkout of the parent)
    ds = {arm: FA.PiecesDataset(world, R, 101, resident=True, **({} if arm == 'strided' else dict(context_draw=arm, context_seed=11)))
          for arm in arms}

    def run(arm):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            training(ds[arm], model=model, loss=loss, optimizer=optim)
        torch.cuda.synchronize()
        rates = [float(l.split(':')[1]) for l in buf.getvalue().splitlines() if l.startswith('train clips/s')]
        last = training.last
        assert last['replays'] > 0 and last['input_copies'] == 0, last
        assert getattr(last['loader'], 'n_draw', 0) == (a.epochs if arm == 'random' else 0), arm
        print('training %s: %s' % (arm, [round(r) for r in rates]), file=sys.stderr, flush=True)
        return statistics.median(rates[1:])
    for arm in arms:
        run(arm)                             # warm-up
    rate = {arm: [] for arm in arms}
    for _ in range(a.pairs):
        for arm in arms:
            rate[arm].append(run(arm))
    row = {'clips_per_epoch': len(ds[arms[0]]), 'epochs': a.epochs, 'batch_size': B,
           'what': 'training(), opt.device_collate on: median of the epochs from the second on, clips/s as training() prints it',
           'arms': {arm: {'clips_per_s': round(statistics.median(v), 1), 'pairs': [round(x, 1) for x in v], 'spread': round(max(v) - min(v), 1)}
                    for arm, v in rate.items()}}
    if 'random' in rate:
        rd = ds['random']
        row['slots'], row['longest_list'], row['pool_entries'] = int(rd.slot_dst.size), int(np.diff(rd.slot_off).max()), int(rd.pool_rows.shape[0])
        row['random_over_strided'] = round(statistics.median(rate['random']) / statistics.median(rate['strided']), 4)
        row['random_over_strided_pairs'] = [round(x / y, 4) for x, y in zip(rate['random'], rate['strided'])]
    return row, ds[arms[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--samples', type=int, default=16384)
    ap.add_argument('--slots-per-sample', type=int, default=2)
    ap.add_argument('--max-len', type=int, default=512)
    ap.add_argument('--strided-only', action='store_true')
    ap.add_argument('--parent', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'context_draw.json'))
    a = ap.parse_args()
    world = FA.synthetic_world(4321, n_scenes=256, per_scene=8, n_rel_names=15, n_inter_names=101)
    res = {'device': torch.cuda.get_device_name(0), 'pairs': a.pairs}
    res['training'], ds = train_rows(world, ('strided',) if a.strided_only else ('strided', 'random'), a)
    if not a.strided_only:
        res['collate_call'] = collate_row(ds, a)
        res['draw_launch'] = launch_row(a)
        res['draw_over_collate'] = round(res['draw_launch']['us_per_call']['median'] / res['collate_call']['us_per_call']['median'], 2)
    if a.parent:
        with open(a.parent) as f:
            parent = json.load(f)['training']['arms']['strided']
        mine = res['training']['arms']['strided']
        res['strided_against_parent'] = {'parent': parent, 'this': mine, 'this_over_parent': round(mine['clips_per_s'] / parent['clips_per_s'], 4),
                                         'what': 'the strided arm of this run beside the same arm run by a checkout of the parent commit '
                                                 '(--strided-only), one process after the other'}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
