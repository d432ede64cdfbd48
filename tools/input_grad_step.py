#!/usr/bin/env python
"""The bench-shape eager train step with and without ``requires_grad`` features (lirec_embed_dx), on an fp32 resident block.

Usage:  python tools/input_grad_step.py [--batch 64 --tracks 16 --ctx-clips 18 --fill survey --steps 30 --rounds 4]

Both arms run alternately in the same process (``--rounds`` rounds of ``--steps`` steps each), so that drift of the box hits both;
the report gives ms / step per arm (median over rounds and the spread), the dX launches alone by HIP events around one call of
the library (the zero pass + the grouped GEMM, on the dZ1 a real backward left), and their algorithmic FLOPs and bytes against
the write bound.  One JSON line on stdout.
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
from lirec_amd import model as M             # noqa: E402
from lirec_amd.config import opt             # noqa: E402
from lirec_amd.data import synthetic_batch, to_device_batch   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=16)
    ap.add_argument('--ctx-clips', type=int, default=18)
    ap.add_argument('--fill', choices=['survey', 'dense'], default='survey')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    B, T, R = a.batch, a.tracks, a.ctx_clips
    config.recipe('int_rel_ch', rels_n_clips=R)
    opt.device = 'cuda'
    model, loss, optim = M.create_model(101, n_rels=15)
    model.train()
    hb = synthetic_batch(1234, 'int_rel_ch', B, T=T, R=R)
    if a.fill == 'dense':
        hb['rels_mask'].fill_(1)
    batch = to_device_batch(hb, 'cuda')
    f = batch['features']
    fg = f.detach().clone().requires_grad_(True)
    valid = int((hb['rels_mask'] != 0).sum())

    def step(feat):
        b = dict(batch, features=feat)
        optim.zero_grad()
        loss(model(b), b).backward()
        optim.step()
        if feat.requires_grad:
            feat.grad = None

    arms = {'plain': f, 'requires_grad': fg}
    for feat in arms.values():
        for _ in range(a.warmup):
            step(feat)
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, feat in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(feat)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)

    # the dX launches alone: one more forward + backward with the library call timed by HIP events around it
    ev = []
    real = ops.embed_dx

    def timed(heads, W1, dX):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(heads, W1, dX)
        e1.record()
        ev.append((e0, e1))
    ops.embed_dx = timed
    try:
        for _ in range(5):
            step(fg)
    finally:
        ops.embed_dx = real
    torch.cuda.synchronize()
    dx_us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)

    n, D, J = B * T, f.shape[-1], opt.joint_dim
    rows = n + valid
    flops = 2.0 * rows * J * D
    out_bytes = 4.0 * n * (R + 1) * D                      # the whole block is written (fp32)
    nz_bytes = 4.0 * rows * D
    read_bytes = 4.0 * rows * 4 * J + 2 * 4.0 * J * D       # dZ1 (fp32 or hi + lo planes) + both heads' W1
    write_bound_us = out_bytes / 5e12 * 1e6
    res = {'shape': {'B': B, 'T': T, 'R': R, 'fill': a.fill, 'valid_ctx_rows': valid, 'rows': rows, 'D': D, 'J': J},
           'gemm_mode': ops.get_gemm_mode(),
           'ms_per_step': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'rounds': v} for k, v in ms.items()},
           'dx_us': {'median': statistics.median(dx_us), 'min': dx_us[0], 'all': dx_us},
           'dx_flops': flops, 'dx_bytes_written': out_bytes, 'dx_bytes_nonzero': nz_bytes, 'dx_bytes_read': read_bytes,
           'write_bound_us_at_5TBps': write_bound_us,
           'dx_over_write_bound': statistics.median(dx_us) / write_bound_us,
           'dx_tflops': flops / (statistics.median(dx_us) * 1e-6) / 1e12}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
