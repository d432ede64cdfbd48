"""lirec_amd.test.testing with the evaluation counters on the device (opt.device_metrics) against the per-batch host counters,
for all four recipes: the returned dict, the confusion matrix, every Precision counter and the per-pair relationship scores are
EQUAL; the loss of the two recipes without a maximum over tracks agrees to 1e-12 relative (the same float32 per-batch values
summed in double on both sides: only the rounding of the host's ``val * n`` differs), that of the max-over-tracks recipes, whose
device sum is a float32 one, to the rounding of that sum."""
import numpy as np
import pytest

from lirec_amd.config import opt
from test_gpu_loops import _setup

pytestmark = pytest.mark.gpu


def _run(ds, model, loss, on):
    from lirec_amd.test import testing
    opt.device_metrics = on
    try:
        res = testing(ds, model, loss, mode='test', verbose=False)
    finally:
        opt.device_metrics = True
    return res, dict(testing.last)


@pytest.mark.parametrize('kind', ['modalties', 'int_rels', 'int_ch', 'int_rel_ch'])
def test_device_metrics_equal_host_metrics_for_every_recipe(kind, tmp_path):
    mk, model, loss, optim = _setup(kind, tmp_path)
    ds = mk(23, 4)                                        # 23 clips in batches of 4: a last batch of three
    dev, ld = _run(ds, model, loss, True)
    host, lh = _run(ds, model, loss, False)
    assert ld['metrics_on_device'] is True and lh['metrics_on_device'] is False
    assert dev == host
    assert ld['n_clips'] == lh['n_clips'] == 23
    assert np.array_equal(ld['conf_mat'], lh['conf_mat']) and ld['conf_mat'].dtype == lh['conf_mat'].dtype
    cd, ch = ld['precision'].counters(), lh['precision'].counters()
    assert cd == ch and cd['total'] > 0
    if not opt.tr_maximize:
        assert lh['conf_mat'].sum() == 23 and ch['total'] == 23
    if opt.soft_gt:
        assert ch['_top5_sf'] >= ch['_top1_sf'] and ld['precision'].top5_sf() == lh['precision'].top5_sf()
    rd, rh = ld['relationships'], lh['relationships']
    assert (rd is None) == (rh is None)
    if rd is not None and not opt.tr_maximize:
        assert len(rh._gt) > 0                            # (the synthetic clips do carry labelled pairs)
        assert list(rd._gt) == list(rh._gt) and all(rd._gt[h] == rh._gt[h] for h in rh._gt)
        assert all(np.array_equal(rd._scores[h], rh._scores[h]) and rd._scores[h].dtype == rh._scores[h].dtype for h in rh._scores)
        assert rd.preds == rh.preds and np.array_equal(rd.conf_mat, rh.conf_mat)
        assert (rd.total, rd._top1, rd._top3) == (rh.total, rh._top1, rh._top3)
    if not opt.tr_maximize:
        assert abs(ld['loss'] - lh['loss']) <= 1e-12 * abs(lh['loss']), (ld['loss'], lh['loss'])
    else:
        # the max-over-tracks loop keeps its float32 accumulator on the device (left as it was): six non-negative per-batch
        # values added one after the other in float32 carry at most gamma_5 = 5u / (1 - 5u) relative, u = 2^-24 -- below 6u with the
        # few double roundings of the averages on top; the host sums in double
        assert abs(ld['loss'] - lh['loss']) <= 6 * 2.0 ** -24 * abs(lh['loss']), (ld['loss'], lh['loss'])
    assert np.isfinite(lh['loss']) and lh['loss'] != 0.0
