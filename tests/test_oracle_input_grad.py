"""Pin the CPU oracle's input-feature gradient (autograd through oracle.lirec_oracle) to the reference's own
(tests/golden/input_grad/cells.npz, written by tools/make_golden_input_grad.py): the tolerance of tests/test_oracle_golden.py --
both are torch-CPU fp32 graphs of the same ops."""
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, Cell, assert_close
from oracle import lirec_oracle as O

REF = dict(np.load(os.path.join(GOLDEN, 'input_grad', 'cells.npz')))
NAMES = sorted({k.split('/')[0] for k in REF})


def oracle_dx(cell):
    P = {k: v.clone().requires_grad_(True) for k, v in cell.params().items()}
    batch = cell.batch()
    f = batch['features'].requires_grad_(True)
    out = O.model_forward(P, cell.ocfg, batch, cell.dropout())
    O.loss_forward(cell.ocfg, out, batch, cell.n_rels, cell.sampler(), use_ce=cell.use_ce).sum().backward()
    return f.grad


def test_fixture_covers_the_representative_cells():
    assert set(NAMES) >= {'modalties_m', 'modalties_t', 'int_rels_train', 'int_rels_nogate', 'int_ch_train', 'int_rel_ch_train',
                          'int_rel_ch_cat_train', 'full_int_rel_ch'}


@pytest.mark.parametrize('name', NAMES)
def test_oracle_input_grad_matches_reference(name):
    g = oracle_dx(Cell(name))
    assert g.dtype == torch.float64
    if name + '/norm' in REF:
        n = float(REF[name + '/norm'])
        assert tuple(g.shape) == tuple(REF[name + '/shape'])
        assert abs(g.norm().item() - n) <= 1e-5 * n
        assert_close(g.reshape(-1, g.shape[-1])[:4], REF[name + '/head'], 1e-5, 1e-6, 'dX head')
    else:
        assert tuple(g.shape) == REF[name].shape
        assert_close(g, REF[name], 1e-5, 1e-6, 'dX')
