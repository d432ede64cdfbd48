#!/usr/bin/env python
"""``testing()`` and ``predict()`` over a resident block store with ``opt.record_eval`` on against off (the eager loop), the GPU time
of one replayed evaluation step, and -- the claim that the default did not move -- the off arm against another build of the package.

Usage:  python tools/recorded_eval_times.py [--pairs 3 --replays 10 --repeats 7 --clips-modalties 16384 --clips-int-rels 1024 --clips-int-ch 1024
                                              --unique 64 --other-root DIR --out profiles/recorded_eval.json]

``modalties``, ``int_rels`` and ``int_ch`` (T = 20) over the synthetic tiled dataset at the real feature width (``--unique`` samples
repeated), batch 64, ``opt.layer1_planes`` on.  Host clock around a call that ends in a device synchronise, clips/s.  One warm-up
per arm, then ``--pairs`` alternating off / on pairs in one process.  The store is built once per recipe, outside the timed region.
The step: a ``RecordedEvalStep`` of draw + forward + loss + the loss's accumulation (the counters' one launch is not in it),
``--replays`` back-to-back replays between two device events, the cursor set back outside them; the median of ``--pairs`` rounds.
``--other-root DIR``: a checkout of another commit (the parent), built, running FROM ITS OWN PACKAGE in a process of its own: this
tree's off arm and that tree's loop alternate, ``--pairs`` processes each, every process one warm-up and the median of
``--repeats`` timed calls per entry point and recipe (a pass over 1 024 clips is 3 ms long: single calls scatter by several per cent).
``off_inside_other_spread``: this tree's median lies inside [min, max] of the other tree's runs.
One JSON document, printed and written; figures only.  (``--one-arm``: what such a process runs; it prints its rates.)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64
ARMS = ('off', 'on')
KINDS = ('modalties', 'int_rels', 'int_ch')


class Repeated:
    """``n_clips`` clips that repeat the first ``unique`` samples of a synthetic dataset, drawn once"""

    def __init__(self, base, unique, n_clips):
        self.samples = [base[i] for i in range(unique)]
        self.n_clips, self.epoch = n_clips, 0
        self.n_classes, self.n_rels, self.rels_list, self.interidx2mgdidx = base.n_classes, base.n_rels, base.rels_list, base.interidx2mgdidx

    def __len__(self):
        return self.n_clips

    def __getitem__(self, idx):
        return self.samples[idx % len(self.samples)]


def setup(kind, n_clips, unique):
    """(store, model, loss) of one recipe -- from whichever package is first on sys.path"""
    import torch
    from lirec_amd import config, model as M
    from lirec_amd.blockstore import ResidentBlockDataset
    from lirec_amd.config import opt
    from lirec_amd.data import SyntheticMixedFeaturesDataset
    kw = dict(T=20) if kind == 'int_ch' else {}
    config.recipe(kind, batch_size=B, num_workers=0)
    opt.device = 'cuda'
    opt.set(layer1_planes=True)
    base = SyntheticMixedFeaturesDataset(kind, unique, seed=7, soft_gt=opt.soft_gt, **kw)
    store = ResidentBlockDataset(Repeated(base, unique, n_clips))
    torch.manual_seed(1)
    model, loss, _ = M.create_model(101, n_rels=15)
    return store, model, loss


def calls(store, model, loss):
    from lirec_amd.predict import predict
    from lirec_amd.test import testing
    return (('testing', lambda: testing(store, model, loss, mode='test', verbose=False), testing),
            ('predict', lambda: predict(store, model), predict))


def timed_call(call, n_clips):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return n_clips / (time.perf_counter() - t0)


def summary(rate):
    row = {'arms': {k: {'clips_per_s': round(statistics.median(v), 1), 'pairs': [round(x, 1) for x in v]} for k, v in rate.items()}}
    row['on_over_off'] = round(statistics.median(rate['on']) / statistics.median(rate['off']), 3)
    row['on_over_off_pairs'] = [round(a / b, 3) for a, b in zip(rate['on'], rate['off'])]
    row['on_faster_in_every_pair'] = all(a > b for a, b in zip(rate['on'], rate['off']))
    return row


def step_time(store, model, loss, replays, rounds):
    """GPU milliseconds of one replayed step: draw + forward + loss + accumulate, back-to-back replays between two device events"""
    import torch
    from lirec_amd import ops
    from lirec_amd.graph import RecordedEvalStep
    from lirec_amd.loader import BlockLoader
    loader = BlockLoader(store, batch_size=B)
    loader.stable_ids = True
    it = iter(loader)
    model.eval()
    acc = torch.zeros(1, dtype=torch.float64, device='cuda')
    with torch.no_grad():
        first = next(it)
        loss(model(dict(first)), first)                     # lazy allocations happen on an eager batch
        batch = next(it)
        loader.cursor_to_last()
        lay, blob = tuple(batch['_layout']), batch['_dev_blob']
        step = RecordedEvalStep(model, batch, lambda: loader.collate_at(lay, blob),
                                lambda out, b: ops.scalar_accumulate(acc, loss(out, b).detach().reshape(-1)[:1]), loss=loss)
    assert (replays + 2) * B <= len(store), 'not enough clips for that many replays'
    ms = []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds + 1):                             # (the first round is the warm-up)
        loader.cursor.fill_(0)
        a.record()
        for _ in range(replays):
            step.step()
        b.record()
        b.synchronize()
        if r:
            ms.append(a.elapsed_time(b) / replays)
    n = step.cmds.size
    step.release()
    return {'ms_per_step': round(statistics.median(ms), 4), 'rounds': [round(x, 4) for x in ms], 'commands': n, 'replays_per_round': replays}


def recipe_rows(kind, n_clips, unique, pairs, replays):
    import torch
    from lirec_amd.config import opt
    store, model, loss = setup(kind, n_clips, unique)
    rows = {'clips': n_clips, 'batch_size': B}
    for what, call, fn in calls(store, model, loss):
        def run(arm):
            opt.record_eval = arm == 'on'
            try:
                rate = timed_call(call, n_clips)
            finally:
                opt.record_eval = False
            want = (n_clips // B - 2) if arm == 'on' else 0
            assert fn.last['recorded_steps'] == want, (kind, what, arm, fn.last['recorded_steps'], want)
            print('%s %s %s: %.1f clips/s' % (kind, what, arm, rate), file=sys.stderr, flush=True)
            return rate
        for arm in ARMS:
            run(arm)                                        # warm-up
        rate = {arm: [] for arm in ARMS}
        for _ in range(pairs):
            for arm in ARMS:
                rate[arm].append(run(arm))
        rows[what] = summary(rate)
    rows['replayed_step'] = step_time(store, model, loss, replays, pairs)
    del store, model, loss
    torch.cuda.empty_cache()
    return rows


def one_arm(sizes, unique, repeats):
    """this process's package, the default flags: one warm-up and the median of ``repeats`` timed calls per entry point and recipe"""
    import torch
    out = {}
    for kind in KINDS:
        store, model, loss = setup(kind, sizes[kind], unique)
        out[kind] = {}
        for what, call, _ in calls(store, model, loss):
            call()
            out[kind][what] = statistics.median(timed_call(call, sizes[kind]) for _ in range(repeats))
        del store, model, loss
        torch.cuda.empty_cache()
    return out


def against_other(other_root, sizes, unique, pairs, repeats):
    """this tree's default loop against ``other_root``'s, each process running its own package, alternating"""
    me = os.path.abspath(__file__)
    runs = {'this': [], 'other': []}
    for _ in range(pairs):
        for who, root in (('other', os.path.abspath(other_root)), ('this', HERE)):
            cmd = [sys.executable, me, '--one-arm', '--package-root', root, '--unique', str(unique), '--repeats', str(repeats)] + \
                  [x for k in KINDS for x in ('--clips-' + k.replace('_', '-'), str(sizes[k]))]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600)
            runs[who].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
            print('%s: %s' % (who, runs[who][-1]), file=sys.stderr, flush=True)
    res = {}
    for kind in KINDS:
        res[kind] = {}
        for what in ('testing', 'predict'):
            t, o = [r[kind][what] for r in runs['this']], [r[kind][what] for r in runs['other']]
            res[kind][what] = {'this_off': [round(x, 1) for x in t], 'other': [round(x, 1) for x in o],
                               'this_over_other': round(statistics.median(t) / statistics.median(o), 3),
                               'off_inside_other_spread': min(o) <= statistics.median(t) <= max(o)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--replays', type=int, default=10)
    ap.add_argument('--clips-modalties', type=int, default=16384)
    ap.add_argument('--clips-int-rels', type=int, default=1024)
    ap.add_argument('--clips-int-ch', type=int, default=1024)
    ap.add_argument('--unique', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--other-root', default='')
    ap.add_argument('--one-arm', action='store_true')
    ap.add_argument('--package-root', default=HERE)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'recorded_eval.json'))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    sizes = {'modalties': a.clips_modalties, 'int_rels': a.clips_int_rels, 'int_ch': a.clips_int_ch}
    if a.one_arm:
        print(json.dumps(one_arm(sizes, a.unique, a.repeats)))
        return
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'pairs': a.pairs, 'rows': {}}
    for kind in KINDS:
        res['rows'][kind] = recipe_rows(kind, sizes[kind], a.unique, a.pairs, a.replays)
    if a.other_root:
        res['default_against_other_build'] = against_other(a.other_root, sizes, a.unique, a.pairs, a.repeats)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
