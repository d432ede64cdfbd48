#!/usr/bin/env python
"""The eager train step on a batch of de-duplicated piece tables with and without ``requires_grad`` tables (lirec_embed_dx_indexed),
against the same batch as a gathered block that requires grad (lirec_embed_dx, the route a user has without the tables' gradient).

Usage:  python tools/pieces_input_grad_step.py [--batch 64 --ctx-clips 18 --steps 30 --rounds 4]

The batch: ``--batch`` shuffled clips of bench.py's pieces world (synthetic_world(4321, n_scenes=256, per_scene=8), T = 20), GEMM
mode 2.  Three arms, run alternately in the same process (``--rounds`` rounds of ``--steps`` steps each) so that drift of the box
hits all of them: (a) tables without grad on the once-per-piece path (opt.pieces_q32b = False), (b) tables that require grad (the
same path), (c) the gathered (B T, R+1, D) block requiring grad.  The report gives ms / step per arm (median over rounds and the
spread), the new launch alone by HIP events around the library call (on the S a real backward left), and its algorithmic FLOPs and
bytes against the MFMA bound (three bf16 passes) and the HBM bound.  One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lirec_amd import config, ops            # noqa: E402
from lirec_amd import features as F          # noqa: E402
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402

BF16_PEAK, HBM_BW = 2.5e15, 5e12             # dense bf16 MFMA spec; the HBM rate the other tools take as reachable


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    B, R = a.batch, a.ctx_clips
    wd = F.synthetic_world(4321, n_scenes=256, per_scene=8, n_rel_names=15, n_inter_names=101)
    ds = F.PiecesDataset(wd, R, 101, pin_memory=False)
    pick = torch.randperm(len(ds), generator=torch.Generator().manual_seed(7))[:B].tolist()
    hb = ds.collate_fn([ds[i] for i in pick])
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    ops.set_gemm_mode(2)
    model, loss, optim = M.create_model(101, n_rels=15)
    model.train()
    pieces = F.indexed_batch(hb, 'cuda')
    block = F.gather_features(hb, 'cuda')
    clip0, track0 = pieces['feature_pieces']['clip'], pieces['feature_pieces']['track']
    clip_g, track_g = clip0.detach().clone().requires_grad_(True), track0.detach().clone().requires_grad_(True)
    feat_g = block['features'].detach().clone().requires_grad_(True)
    T = hb['feature_index'].shape[1]

    def step(arm):
        if arm == 'block_requires_grad':
            b = dict(block, features=feat_g)
        else:
            tabs = (clip_g, track_g) if arm == 'tables_requires_grad' else (clip0, track0)
            b = dict(pieces, feature_pieces=dict(pieces['feature_pieces'], clip=tabs[0], track=tabs[1]))
        optim.zero_grad()
        loss(model(b), b).backward()
        optim.step()
        for t in (clip_g, track_g, feat_g):
            t.grad = None

    opt.pieces_q32b = False                  # arm (a): the once-per-piece path (where (b) is routed whatever the flag says)
    arms = ('tables_no_grad', 'tables_requires_grad', 'block_requires_grad')
    for arm in arms:
        for _ in range(a.warmup):
            step(arm)
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for arm in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(arm)
            torch.cuda.synchronize()
            ms[arm].append((time.perf_counter() - t0) * 1e3 / a.steps)

    # the new launch alone: five more steps of arm (b) with the library call timed by HIP events around it
    ev = []
    real = ops.embed_dx_indexed

    def timed(*args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(*args)
        e1.record()
        ev.append((e0, e1))
    ops.embed_dx_indexed = timed
    try:
        for _ in range(5):
            step('tables_requires_grad')
    finally:
        ops.embed_dx_indexed = real
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)

    J, nh = opt.joint_dim, 2
    nc1, nt1 = clip0.shape[0], track0.shape[0]
    cd, kd = clip0.shape[1], track0.shape[1]
    flops = 2.0 * (nc1 * cd * nh * J + nt1 * kd * 2 * nh * J)
    written = 4.0 * (nc1 * cd + nt1 * kd)
    read = 4.0 * nh * ((nc1 + nt1) * 2 * J + J * (cd + 2 * kd))        # S of both heads + both heads' W1
    mfma_us = 3 * flops / BF16_PEAK * 1e6                              # bf16x3: three bf16 passes
    hbm_us = (written + read) / HBM_BW * 1e6
    med = statistics.median(us)
    res = {'shape': {'B': B, 'T': T, 'R': R, 'n_clip': nc1 - 1, 'n_track': nt1 - 1, 'clip_dim': cd, 'track_dim': kd, 'J': J,
                     'block_MB': round(feat_g.numel() * 4 / 1e6, 1), 'tables_MB': round(4.0 * (nc1 * cd + nt1 * kd) / 1e6, 1)},
           'gemm_mode': ops.get_gemm_mode(),
           'ms_per_step': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'rounds': v} for k, v in ms.items()},
           'dx_indexed_us': {'median': med, 'min': us[0], 'all': us},
           'dx_indexed_flops': flops, 'dx_indexed_bytes_written': written, 'dx_indexed_bytes_read': read,
           'mfma_bound_us_bf16x3': mfma_us, 'hbm_bound_us_at_5TBps': hbm_us,
           'dx_indexed_over_larger_bound': med / max(mfma_us, hbm_us),
           'dx_indexed_tflops': flops / (med * 1e-6) / 1e12}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
