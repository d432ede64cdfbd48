"""Per-clip weights and per-clip loss values without a GPU: the three exports and the struct, every LIREC_EINVAL of the contract
before any device call (with and without the library's host-side dry run), the float64 composition of tests/weight_cases.py against
the oracle of the whole batch, the caps of the decisions float32 may take the other way for every case the GPU file uses, and the
host side of the feature: class-balanced weights, the datasets that carry weights, the batch buffer's optional tenth field, the
device-collate fall-back and the validation of host weights."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import loss_cases as LC
import weight_cases as WC
from lirec_amd import _lib, config, data
from lirec_amd import features as F
from lirec_amd.config import opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
NEW = ('lirec_margin_loss_weighted', 'lirec_heads_loss_fwd_bwd_weighted', 'lirec_ce_loss_weighted')
# fake, aligned, never dereferenced
P = [0x10000000 * k for k in range(1, 16)]


def test_exports_struct_and_version():
    hdr = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert 'lirec_clip_weights' in hdr
    assert L.lirec_abi_sizeof(19) == C.sizeof(_lib.ClipWeights) == 24
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    for which in (14, 16, 18, 99):
        assert L.lirec_abi_sizeof(which) == -1
    assert L.lirec_abi_sizeof(2) == C.sizeof(_lib.MarginLossArgs)                  # (the loss's own struct keeps its layout)


def _margin_args(**kw):
    a = _lib.MarginLossArgs()
    a.ints, a.ld_ints, a.rels, a.ld_rels, a.y, a.r = P[0], 101, P[1], 15, P[2], P[3]
    a.d_ints, a.ld_dints, a.d_rels, a.ld_drels, a.loss, a.partial = P[4], 101, P[5], 15, P[6], P[7]
    a.B, a.T, a.C, a.NR, a.margin, a.lymbda = 4, 3, 101, 15, 0.1, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _cw(w=P[8], w_f64=0, norm=0, clip_loss=P[9]):
    s = _lib.ClipWeights()
    s.w, s.w_f64, s.norm, s.clip_loss = w, w_f64, norm, clip_loss
    return s


BAD = {
    'w and clip_loss both NULL': dict(w=None, clip_loss=None),
    'norm 2': dict(norm=2),
    'norm -1': dict(norm=-1),
    'float32 w misaligned': dict(w=P[8] + 2),
    'float64 w misaligned': dict(w=P[8] + 4, w_f64=1),
    'clip_loss misaligned': dict(clip_loss=P[9] + 1),
}


def _calls(L, cw, sample=0):
    """the three weighted calls with otherwise valid arguments"""
    a = _margin_args(sample=sample, probs_out=P[10], sel_out=P[11])
    heads = (_lib.LinearFwdArgs * 1)()
    heads[0].A, heads[0].lda, heads[0].W, heads[0].b, heads[0].Y, heads[0].ldy = P[12], 64, P[13], P[14], P[0], 101
    heads[0].n, heads[0].K, heads[0].N = 12, 64, 101
    back = (_lib.LinearBwdArgs * 1)()
    ref = C.byref(cw) if cw is not None else None
    yield 'margin', L.lirec_margin_loss_weighted(C.byref(a), ref, None)
    yield 'heads', L.lirec_heads_loss_fwd_bwd_weighted(heads, back, 1, C.byref(a), ref, None)
    if not sample:
        yield 'ce', L.lirec_ce_loss_weighted(P[0], 101, P[1], 15, P[2], P[3], None, 4, 101, 15, P[4], 101, P[5], 15, P[6], P[7],
                                             0.0, 0.0, None, ref, None)


@pytest.mark.parametrize('dry', [False, True], ids=['plain', 'dry-run'])
@pytest.mark.parametrize('what', sorted(BAD))
def test_invalid_structs_are_refused_before_any_device_call(what, dry):
    """without the dry run a call that got past the checks would reach the HIP runtime, which has no device here"""
    L = _lib.lib()
    if dry:
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        for name, rc in _calls(L, _cw(**BAD[what])):
            assert rc == EINVAL, (what, name)
    finally:
        assert L.lirec_debug_set(0, -1) == 0


@pytest.mark.parametrize('dry', [False, True], ids=['plain', 'dry-run'])
def test_probabilities_only_refuses_a_struct(dry):
    L = _lib.lib()
    if dry:
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        for name, rc in _calls(L, _cw(), sample=2):
            assert rc == EINVAL, name
        assert L.lirec_heads_loss_fwd_bwd_weighted((_lib.LinearFwdArgs * 1)(), None, 1, None, C.byref(_cw()), None) == EINVAL
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def test_valid_structs_pass_the_checks_in_the_dry_run():
    """weights only, per-clip values only, both, float64 weights, both norms: the dry run hands the launches to nobody"""
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        for cw in (_cw(clip_loss=None), _cw(w=None), _cw(), _cw(w_f64=1, norm=1), None):
            for name, rc in _calls(L, cw):
                if name != 'heads':                                   # (the heads' GEMMs want real shapes; the checks are shared)
                    assert rc == 0, name
    finally:
        assert L.lirec_debug_set(0, -1) == 0


# ---- the float64 composition ------------------------------------------------------------------------------------------------
CASES = WC.all_cases()


@pytest.mark.parametrize('case,how', CASES, ids=['%s-%s' % (LC.case_id(c), h) for c, h in CASES])
def test_composition_equals_the_oracle_at_unit_weights_and_caps_hold(case, how):
    """one-clip slices, recombined with weights 1 under either norm, are the oracle of the whole batch (1e-12); the seeds of the GPU
    file keep the float64 decisions clear of rounding (loss_cases.caps_hold, unchanged)"""
    case = LC.seeded(case, how)
    inp = LC.make_inputs(case)
    k = LC.positive(case, inp, how)
    assert LC.caps_hold(case, LC.restate(case, inp, k), forced=how in ('sel', 'sample'))
    loss, d_i, d_r, xm = LC.oracle64(case, inp, k)
    terms = WC.clip_terms64(case, inp, k)
    for norm in WC.NORMS:
        for w in (None, torch.ones(case.B, dtype=torch.float64)):
            l2, g_i, g_r, clip, xm2 = WC.weighted64(case, inp, w, norm, k, terms=terms)
            assert abs(float(l2 - loss)) <= 1e-12
            assert float((g_i - d_i).abs().max()) <= 1e-12
            if case.rels:
                assert float((g_r - d_r).abs().max()) <= 1e-12
            assert torch.equal(xm2, xm)
            den_i, den_r = WC.denominators(case, inp, w, norm)[0]
            total = clip[:, 0].sum() / den_i + (clip[:, 1].sum() / den_r if den_r > 0 else 0.0)
            assert abs(float(total - loss)) <= 1e-12


def test_composition_weights_and_zero_denominators():
    """doubling every weight changes nothing under 'sum' and doubles everything under 'count'; all weights 0 is loss 0, no NaN"""
    case = LC.seeded(WC.FORMS[1])
    assert case.form == 'mtmm'
    inp = LC.make_inputs(case)
    terms = WC.clip_terms64(case, inp)
    w = WC.draw_weights(case.B, 5)
    assert int((w == 0).sum()) == 2 and float(w[w > 0].min()) >= 1e-3 and float(w.max()) <= 1e3
    for norm, factor in (('sum', 1.0), ('count', 2.0)):
        a, b = WC.weighted64(case, inp, w, norm, terms=terms), WC.weighted64(case, inp, 2 * w, norm, terms=terms)
        assert abs(float(b[0] - factor * a[0])) <= 1e-12 * max(1.0, abs(float(a[0])))
        assert torch.allclose(b[1], factor * a[1], rtol=1e-12, atol=0) and torch.allclose(b[2], factor * a[2], rtol=1e-12, atol=0)
        z = WC.weighted64(case, inp, torch.zeros(case.B, dtype=torch.float64), norm, terms=terms)
        assert float(z[0]) == 0.0 and not z[1].any() and not z[2].any() and bool(torch.isfinite(z[3]).all())
    # every labelled clip at weight 0: the relationship half alone is 0
    w2 = torch.where(WC.labelled(case, inp), torch.zeros_like(w), w + 1.0)
    l, g_i, g_r, _, _ = WC.weighted64(case, inp, w2, 'sum', terms=terms)
    assert not g_r.any() and g_i.any() and float(l) > 0


# ---- weights from data ------------------------------------------------------------------------------------------------------
def test_class_balanced_weights_by_hand():
    y = [0, 0, 0, 2, 2, 3]                                    # class 1 has no sample
    w = data.class_balanced_weights(y, 4, 'inverse')
    raw = np.array([1 / 3, 1 / 3, 1 / 3, 1 / 2, 1 / 2, 1.0])
    assert w.dtype == np.float64 and np.allclose(w, raw / raw.mean(), rtol=1e-15) and abs(w.mean() - 1) < 1e-15
    beta = 0.9
    e = data.class_balanced_weights(y, 4, 'effective', beta=beta)
    raw = np.array([(1 - beta) / (1 - beta ** n) for n in (3, 3, 3, 2, 2, 1)])
    assert np.allclose(e, raw / raw.mean(), rtol=1e-15) and bool(np.isfinite(e).all())
    assert np.allclose(data.class_balanced_weights([1, 1, 1], 3), 1.0)
    assert data.class_balanced_weights([], 3).shape == (0,)
    with pytest.raises(ValueError):
        data.class_balanced_weights(y, 4, 'other')
    with pytest.raises(ValueError):
        data.class_balanced_weights([0, 4], 4)


def test_weighted_dataset_adds_the_key_per_sample():
    base = data.SyntheticMixedFeaturesDataset('int_ch', 6, seed=3, T=4, R=2, text_dim=8, visual_dim=8, track_dim=8)
    w = np.arange(6) / 2.0
    ds = data.WeightedDataset(base, w)
    assert len(ds) == 6 and ds.n_classes == base.n_classes and ds.carries_clip_weights
    s = ds[3]
    assert s['clip_weight'] == 1.5 and s['clip_weight'].dtype == np.float64 and 'clip_weight' not in base[3]
    batch = torch.utils.data.default_collate([ds[i] for i in range(4)])
    assert batch['clip_weight'].dtype == torch.float64 and batch['clip_weight'].tolist() == [0.0, 0.5, 1.0, 1.5]
    ds.epoch = 4
    assert base.epoch == 4
    for bad in ([-1.0] + [1.0] * 5, [float('nan')] + [1.0] * 5, [float('inf')] + [1.0] * 5, [1.0] * 5):
        with pytest.raises(_lib.LirecError):
            data.WeightedDataset(base, bad)
    assert np.array_equal(data.interaction_labels(base), [int(np.asarray(base[i]['labels']).reshape(-1)[0]) for i in range(6)])


def test_pieces_dataset_and_layout_carry_the_field_only_with_weights():
    world = F.synthetic_world(9, n_scenes=3, per_scene=3, text_dim=16, visual_dim=16, track_dim=16)
    plain = F.PiecesDataset(world, 4, pin_memory=False)
    n = len(plain)
    w = np.linspace(0.0, 2.0, n)
    ds = F.PiecesDataset(world, 4, pin_memory=False, clip_weight=w)
    assert F._FIELDS == ('labels', 'just_zeros', 'hash_rel', 'gt_tracks', 'n_names', 'mem_mask', 'rels_label', 'rels_mask',
                         'multilab_weights')
    assert F.batch_fields(plain._stacked) == F._FIELDS and F.batch_fields(ds._stacked) == F._FIELDS + ('clip_weight',)
    ids = [4, 1, 6]
    a, b = plain.collate_fn([plain[i] for i in ids]), ds.collate_fn([ds[i] for i in ids])
    assert 'clip_weight' not in a and b['clip_weight'].dtype == torch.float64 and np.array_equal(b['clip_weight'].numpy(), w[ids])
    # without weights the layout is what the nine fields alone give; with weights the tenth entry lies behind them
    fields = [(k, plain._stacked[k].dtype, (3,) + plain._stacked[k].shape[1:]) for k in F._FIELDS]
    lay9, n9 = F.batch_layout(a['feature_index'].shape, fields)
    assert list(a['_layout']) == lay9 and a['_blob'].numel() == n9
    assert list(b['_layout'])[:len(lay9)] == lay9 and b['_layout'][-1][0] == 'clip_weight' and b['_layout'][-1][1] >= n9 - 256
    assert b['_layout'][-1][2:] == (24, np.dtype(np.float64), (3,))
    assert all(torch.equal(a[k], b[k]) for k in F._FIELDS + ('feature_index',))
    # taken away again / given later: the same dataset
    ds.set_clip_weights(None)
    assert list(ds.collate_fn([ds[i] for i in ids])['_layout']) == lay9 and 'clip_weight' not in ds[0]
    plain.set_clip_weights(w)
    assert np.array_equal(plain.collate_fn([plain[i] for i in ids])['clip_weight'].numpy(), w[ids])
    for bad in (-w - 1, np.full(n, np.nan), w[:-1]):
        with pytest.raises(_lib.LirecError):
            F.PiecesDataset(world, 4, pin_memory=False, clip_weight=bad)
    # the tiled form carries the weight in its samples too
    tiled = F.PiecesDataset(world, 4, emit='tiled', clip_weight=w)
    assert tiled[2]['clip_weight'] == w[2]


def test_device_collate_falls_back_with_weights():
    from lirec_amd.loader import device_collate_in_force
    world = F.synthetic_world(9, n_scenes=3, per_scene=3, text_dim=16, visual_dim=16, track_dim=16)
    ds = F.PiecesDataset(world, 4, pin_memory=False, resident=True)
    config.reset()
    try:
        opt.set(device_collate=True, pieces_gather=True, pieces_q32b=True, layer1_planes=True)
        assert device_collate_in_force(ds, 'cuda')
        ds.set_clip_weights(np.ones(len(ds)))
        assert not device_collate_in_force(ds, 'cuda')
        ds.set_clip_weights(None)
        assert device_collate_in_force(ds, 'cuda')
    finally:
        config.reset()


def test_class_balance_and_norm_flags_default_off():
    config.reset()
    assert opt.class_balance == '' and opt.clip_weight_norm == 'sum'


def test_losses_reject_bad_host_weights():
    """a host tensor is checked (finite, non-negative, one per clip) before anything reaches the device"""
    from lirec_amd import model as M
    config.reset()
    for cls in (M.MaxMarginCrossEntropyLoss, M.MultiTaskMaxMargin, M.MarginLoss, M.MarginTrackRelsLoss,
                lambda: M.MultiTaskCrossEntropyLoss(5, n_rels=3)):
        loss = cls()
        assert loss.keep_clip_losses is False and loss.last_clip_losses is None
        for bad in ([1.0, -0.5, 1.0], [1.0, float('nan'), 1.0], [float('inf'), 1.0, 1.0], [1.0, 1.0]):
            with pytest.raises(_lib.LirecError):
                loss._clip_weight({'clip_weight': torch.tensor(bad, dtype=torch.float64)}, 3, torch.device('cpu'))
        assert loss._clip_weight({}, 3, torch.device('cpu')) is None
    opt.clip_weight_norm = 'mean'
    try:
        with pytest.raises(_lib.LirecError):
            M.MarginLoss()._clip_norm()
    finally:
        config.reset()
