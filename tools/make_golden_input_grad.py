#!/usr/bin/env python
"""Golden input-feature gradients from the REFERENCE itself (CPU; build container only -- the GPU box has no reference).

Usage:  python tools/make_golden_input_grad.py        (writes tests/golden/input_grad/cells.npz)

Re-runs a representative set of the golden cells of ``oracle/make_golden.py`` -- same flags, seeds, parameters, dropout script and
recorded track draws -- with ``batch['features'].requires_grad_(True)`` and stores the reference's ``features.grad`` (float64, the
loader's dtype: the reference's ``.float()`` is differentiable, mlp/model.py:279), keyed by cell name.  Data only.  The file lives in
a subdirectory so that the cell lists of the existing golden tests (tests/golden_util.cell_names: ``tests/golden/*.npz``) stay as
they are; the existing fixtures are neither read nor written.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as G          # noqa: E402
from oracle import lirec_oracle as O         # noqa: E402
from lirec_amd.data import synthetic_batch   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'input_grad', 'cells.npz')
CELLS = ('modalties_m', 'modalties_t', 'int_rels_train', 'int_rels_nogate', 'int_ch_train', 'int_rel_ch_train',
         'int_rel_ch_cat_train', 'full_int_rel_ch')


def input_grad(opt, M, name, kind, flags, dims, bkw, train, seed):
    """make_golden.run_cell's model + loss on the same inputs, returning d loss / d features (and the loss, as a cross-check)."""
    cfg = dict(G.BASE, **dims)
    cfg.update({k: v for k, v in flags.items() if k not in ('use_ce', 'force_none_gt')})
    for k, v in cfg.items():
        setattr(opt, k, v)
    opt.device = 'cpu'
    opt.mlp_dim = cfg['text_dim'] + cfg['visual_dim'] + (2 * cfg['track_dim'] if cfg['tracks'] else 0)
    n_classes, n_rels = bkw['n_classes'], bkw['n_rels']
    with contextlib.redirect_stdout(io.StringIO()):
        model, loss, _ = M.create_model(n_classes, n_rels=n_rels)
    ocfg = O.OracleCfg(**{k: v for k, v in cfg.items() if k in O.OracleCfg.__dataclass_fields__})
    model.load_state_dict(O.fill_params(O.param_shapes(ocfg, n_classes, n_rels), seed + 1000), strict=True)
    gen_kw = dict(text_dim=cfg['text_dim'], visual_dim=cfg['visual_dim'], track_dim=cfg['track_dim'],
                  tracks=cfg['tracks'], **{k: v for k, v in bkw.items() if k != 'B'})
    batch = synthetic_batch(seed, kind, bkw['B'], **gen_kw)
    feats = batch['features'].requires_grad_(True)      # the leaf (the model re-binds x['features'] to a view of it)
    dseed = seed + 77
    if train:
        s_main, s_gate = G.dropout_script(cfg)
        model.dropout = G.ScriptedDropout(dseed, cfg['dropout'], s_main)
        if hasattr(model, 'gates_ints'):
            model.gates_ints.dropout = G.ScriptedDropout(dseed, cfg['dropout'], s_gate)
        model.train()
    else:
        model.eval()
    torch.manual_seed(seed)            # (the same draws as make_golden: torch.multinomial is seeded identically)
    out = model(batch)
    lv = loss(out, batch)
    lv.sum().backward()
    return feats.grad.detach().numpy().copy(), lv.detach().numpy().copy()


def main():
    opt, M = G.load_reference()
    fx = {}
    for i, (name, kind, flags, dims, bkw, train) in enumerate(G.cells()):
        if name not in CELLS:
            continue
        g, lv = input_grad(opt, M, name, kind, flags, dims, bkw, train, seed=100 + i)
        ref = np.load(os.path.join(G.OUT, name + '.npz'))
        assert np.allclose(lv, ref['loss'], rtol=1e-6, atol=1e-7), (name, lv, ref['loss'])    # same run as the fixture's
        if dims is G.FULL:
            # full-dimension cell: the gradient's norm and its first rows only (fixture size); the GPU test holds every element
            # to the oracle, which the norm and rows here pin to the reference
            fx[name + '/norm'] = np.array(np.linalg.norm(g.astype(np.float64)))
            fx[name + '/head'] = g.reshape(-1, g.shape[-1])[:4].astype(np.float32)
            fx[name + '/shape'] = np.array(g.shape, dtype=np.int64)
        else:
            fx[name] = g
        print('%-24s dX %s |dX| = %.6e' % (name, g.shape, float(np.abs(g).sum())))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **fx)


if __name__ == '__main__':
    main()
