#!/usr/bin/env python
"""``lirec_amd.predict`` (every clip decided on the device, one copy per field at the end) against the host route on the same
commit -- the logits copied back once per batch and decided by ``lirec_amd.metrics.joint_predictions`` / ``top_lists`` -- for
``int_rel_ch`` (a maximum over tracks, with relationships) and ``modalties`` (the clip-level form); and the kernel alone against
``lirec_eval_max_tracks`` on the same logits at B = 64, T = 16, C = 101, NR = 15.

Usage:  python tools/predict_times.py [--clips-int-rel-ch 1024 --clips-modalties 32768 --unique 64 --pairs 3 --launches 500
                                       --out profiles/predict_clips.json]

Per recipe: the synthetic dataset at full dimensions, ``--unique`` samples drawn once and repeated up to the dataset's length
(the loop is not timed on the random generator); the loader runs in the predicting process (``num_workers=0``) and is part of
both arms.  One warm-up run per arm, then ``--pairs`` alternating device / host pairs in one process, so that drift of the box
hits both arms; clips / s from a host clock around work that ends in a device synchronise.  The kernels: ``--launches`` launches
of each between two device events, ``--pairs`` alternating pairs, the median per launch.  One JSON document, printed and
written; figures only.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lirec_amd import config, ops            # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.data import SyntheticMixedFeaturesDataset   # noqa: E402
from lirec_amd.metrics import joint_predictions, top_lists  # noqa: E402
from lirec_amd.predict import predict        # noqa: E402

LABEL_KEYS = ('labels', 'rels_label', 'gt_tracks', 'just_zeros', 'soft_labels', 'multilab_weights', 'multilab_weights_axl')


class Repeated(torch.utils.data.Dataset):
    """``n_clips`` unlabelled clips that repeat the first ``unique`` samples of a synthetic dataset, drawn once"""

    def __init__(self, base, unique, n_clips):
        self.samples = [{k: v for k, v in base[i].items() if k not in LABEL_KEYS} for i in range(unique)]
        self.n_clips = n_clips

    def __len__(self):
        return self.n_clips

    def __getitem__(self, idx):
        return self.samples[idx % len(self.samples)]


def host_route(ds, model, batch_size, top_k):
    """what a user had to write before: every batch's logits to the host, the rules of the evaluation re-derived in numpy"""
    out_trk, out_cls, out_top = [], [], []
    model.eval()
    with torch.no_grad():
        for batch in torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=0):
            out = model(batch)
            ints = out['inters'].cpu().numpy()
            C = ints.shape[-1]
            rels = out['rels'].cpu().numpy() if opt.ctx == 1 else None
            if opt.tr_maximize:
                bs = ints.shape[0]
                ints = ints.reshape(bs, -1, C)
                rels = rels.reshape(bs, ints.shape[1], -1) if rels is not None else None
                mem = batch['mem_mask'].numpy()
            else:
                bs = batch['features'].shape[0]
                ints, mem = ints.reshape(bs, -1, C)[:, :1].copy(), None
                rels = rels.reshape(bs, 1, -1) if rels is not None else None
            trk, cls, rel, score, trk_score = joint_predictions(ints, rels, mem)
            rows = np.arange(bs)
            out_top.append(top_lists(ints[rows, trk], top_k))
            if rels is not None:
                out_top.append(top_lists(rels[rows, trk], top_k))
            out_trk.append(trk)
            out_cls.append(cls)
    return np.concatenate(out_trk), np.concatenate(out_cls)


def one_recipe(kind, batch_size, n_clips, unique, pairs, top_k=5):
    config.recipe(kind, batch_size=batch_size, num_workers=0)
    opt.device = 'cuda'
    torch.manual_seed(1)
    model, _, _ = M.create_model(101, n_rels=15)
    ds = Repeated(SyntheticMixedFeaturesDataset(kind, unique, seed=7, soft_gt=opt.soft_gt), unique, n_clips)

    def run(device):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if device:
            p = predict(ds, model, top_k=top_k)
            res = (p.trk, p.cls)
        else:
            res = host_route(ds, model, batch_size, top_k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print('%s %s: %.1f clips/s' % (kind, 'device' if device else 'host', n_clips / dt), file=sys.stderr, flush=True)
        return n_clips / dt, res

    results = {device: run(device)[1] for device in (True, False)}   # warm-up, and the two arms' predictions
    rate = {True: [], False: []}
    for _ in range(pairs):
        for device in (True, False):
            rate[device].append(run(device)[0])
    same = all(np.array_equal(a, b) for a, b in zip(results[True], results[False]))
    row = {'batch_size': batch_size, 'clips': n_clips, 'unique_samples': unique, 'batches': -(-n_clips // batch_size),
           'same_predictions': bool(same), 'arms': {}}
    for device, name in ((True, 'device'), (False, 'host')):
        v = rate[device]
        row['arms'][name] = {'clips_per_s': round(statistics.median(v), 1), 'pairs': [round(x, 1) for x in v],
                             'spread': round(max(v) - min(v), 1)}
    row['device_over_host'] = round(statistics.median(rate[True]) / statistics.median(rate[False]), 4)
    row['device_over_host_pairs'] = [round(a / b, 4) for a, b in zip(rate[True], rate[False])]
    return row


def kernels(pairs, launches, B=64, T=16, Cn=101, NR=15, top_k=5):
    g = torch.Generator().manual_seed(3)
    ints = (torch.randn(B * T, Cn, generator=g) * 3).cuda()
    rels = (torch.randn(B * T, NR, generator=g) * 3).cuda()
    nb = torch.randint(T // 2, T + 1, (B,), generator=g)
    mem = (torch.arange(T)[None, :] < nb[:, None]).double().cuda()
    y = torch.randint(0, Cn, (B,), generator=g).cuda()
    r = torch.randint(0, NR + 1, (B, T), generator=g).cuda()
    gt = torch.stack([torch.zeros(B, dtype=torch.int64), (torch.rand(B, generator=g) * nb).long()], 1).cuda()
    jz = torch.zeros(B, dtype=torch.bool).cuda()
    counters = torch.zeros(8, dtype=torch.int64, device='cuda')
    out = ops.predict_buffers(B, T, top_k, 'cuda')
    joint_only = {k: out[k] for k in ('trk', 'cls', 'rel', 'score')}
    arms = {
        'eval_max_tracks': lambda: ops.eval_max_tracks(ints, rels, mem, y, r, gt, jz, counters, B, T, Cn, NR, loader_types=True),
        'predict_clips': lambda: ops.predict_clips(ints, rels, mem, B=B, T=T, K=top_k, loader_types=True, out=out),
        'predict_clips_joint_only': lambda: ops.predict_clips(ints, rels, mem, B=B, T=T, K=top_k, loader_types=True, out=joint_only),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / launches          # microseconds per launch

    us = {k: [] for k in arms}
    for fn in arms.values():
        timed(fn)                                            # warm-up
    for _ in range(pairs):
        for k, fn in arms.items():
            us[k].append(timed(fn))
    row = {'B': B, 'T': T, 'C': Cn, 'NR': NR, 'K': top_k, 'launches': launches,
           'what': 'microseconds per launch, back-to-back launches between two device events (launch overhead included)',
           'us_per_launch': {k: {'median': round(statistics.median(v), 2), 'pairs': [round(x, 2) for x in v]} for k, v in us.items()}}
    base = statistics.median(us['eval_max_tracks'])
    row['predict_over_eval'] = round(statistics.median(us['predict_clips']) / base, 4)
    row['predict_joint_only_over_eval'] = round(statistics.median(us['predict_clips_joint_only']) / base, 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips-int-rel-ch', type=int, default=1024)
    ap.add_argument('--clips-modalties', type=int, default=32768)
    ap.add_argument('--unique', type=int, default=64)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--launches', type=int, default=500)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'predict_clips.json'))
    a = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'pairs': a.pairs, 'num_workers': 0,
           'kernels': kernels(a.pairs, a.launches),
           'recipes': {'int_rel_ch': one_recipe('int_rel_ch', 64, a.clips_int_rel_ch, a.unique, a.pairs),
                       'modalties': one_recipe('modalties', 64, a.clips_modalties, a.unique, a.pairs)}}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
