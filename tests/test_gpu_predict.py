"""lirec_predict_clips and lirec_amd.predict on the GPU.  The expected side is never a run of the kernel: the integer outputs
are those of lirec_amd.metrics.joint_predictions / top_lists (pinned to the reference through Precision, tests/test_metrics.py
and tests/test_host_predict.py) and must be EQUAL; the real-valued ones are formed from fp64 sigmoids and must agree within the
project's logit tolerance, 1e-5 + 1e-4 |ref|.  Inputs: tests/predict_cases.py (exact ties, margin-safe random logits, every
layout option), the reference's tie fixtures, and logits of the four recipes' models."""
import numpy as np
import pytest
import torch

import predict_cases as PC
from lirec_amd import ops
from lirec_amd.config import opt
from lirec_amd.metrics import joint_predictions
from test_metrics import TIE_CASES, tie_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = PC.named_cases()
INT_FIELDS = ('trk', 'cls', 'rel')
LABEL_KEYS = ('labels', 'rels_label', 'gt_tracks', 'just_zeros', 'soft_labels', 'multilab_weights', 'multilab_weights_axl')


def _rows(x, ld):
    """[B, T, n] host array -> [B*T, n] device view of a NaN-filled block with row stride ``ld``"""
    n = x.shape[-1]
    block = torch.full((x.shape[0] * x.shape[1], ld or n), float('nan'), dtype=torch.float32)
    block[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1, n)
    return block.to(DEV)[:, :n]


def device_inputs(case):
    ints = _rows(case['ints'], case.get('ld_ints'))
    rels = _rows(case['rels'], case.get('ld_rels')) if case['rels'] is not None else None
    mem = None
    if case['mem'] is not None:
        mem = torch.from_numpy(np.asarray(case['mem'])).to(torch.float64 if case.get('mem_f64') else torch.float32).to(DEV)
    return ints, rels, mem


def fresh_outputs(case, byte):
    """the output arrays, every byte set to ``byte``: an element the kernel does not write shows"""
    B, T = case['ints'].shape[:2]
    out = ops.predict_buffers(B, T, case['K'], DEV, with_rels=case['rels'] is not None)
    for v in out.values():
        v.view(torch.uint8).fill_(byte)
    return out


def run_device(case, byte=0x7b, inputs=None):
    ints, rels, mem = inputs or device_inputs(case)
    B, T = case['ints'].shape[:2]
    out = ops.predict_clips(ints, rels, mem, B=B, T=T, K=case['K'], loader_types=bool(case.get('mem_f64')),
                            out=fresh_outputs(case, byte))
    return {k: v.cpu().numpy() for k, v in out.items()}


def close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(ref)
    with np.errstate(invalid='ignore'):
        return bool((both_nan | (np.abs(got - ref) <= 1e-5 + 1e-4 * np.abs(ref))).all())


def check(case, got, what=''):
    exp = PC.expected(case, trk=got['trk'].astype(np.int64))
    assert set(got) == set(exp), (what, sorted(got), sorted(exp))
    assert np.array_equal(got['flags'], exp['flags']), (what, got['flags'], exp['flags'])
    ok = (exp['flags'] & 1) == 0                    # a NaN-flagged clip: only its flags and its top lists are pinned
    for k in INT_FIELDS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k][ok], exp[k][ok]), (what, k, got[k], exp[k])
    B, T, Cn = case['ints'].shape
    NR = case['rels'].shape[2] if case['rels'] is not None else 0
    assert ((got['trk'] >= 0) & (got['trk'] < T) & (got['cls'] >= 0) & (got['cls'] < Cn)).all(), what
    assert ((got['rel'] >= 0) & (got['rel'] <= NR)).all() if NR else (got['rel'] == -1).all(), what
    for k in ('score', 'trk_score'):
        assert got[k].dtype == np.float64 and close(got[k][ok], exp[k][ok]), (what, k, got[k], exp[k])
    for k in ('top_cls', 'top_rel'):
        if k in exp:
            assert np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
            assert got[k + '_p'].dtype == np.float32 and close(got[k + '_p'], exp[k + '_p']), (what, k + '_p')
    n = min(case['K'], Cn)
    assert (got['top_cls'][:, n:] == -1).all() and (got['top_cls_p'][:, n:] == 0).all(), what
    return exp


# ---- named and generated cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_named_cases_equal_the_host_restatement(name):
    case = CASES[name]
    inputs = device_inputs(case)
    got = run_device(case, 0x7b, inputs)
    exp = check(case, got, name)
    # two launches on the same inputs give identical bytes, whatever the arrays held before
    again = run_device(case, 0xc4, inputs)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got), name
    if name == 'j':
        assert exp['flags'].tolist() == [0, 0, 2, 0]
        assert (got['trk'][2], got['cls'][2], got['rel'][2], got['score'][2]) == (0, 0, 0, 0.0) and (got['trk_score'][2] == 0).all()
        assert got['top_cls'][2].tolist() == [0, 1, 2, 3, 4] and (got['top_cls_p'][2] == 0).all()
    if name == 'k':
        assert exp['flags'].tolist() == [0, 1, 0, 0]
    if name == 'k_clip_level':
        assert exp['flags'].tolist() == [1, 0, 0, 1]
        assert 2 not in got['top_cls'][0] and 7 not in got['top_cls'][0]                         # K = 5 of 11: the NaNs stay out
        assert got['top_rel'][3].tolist()[-1] == 0 and np.isnan(got['top_rel_p'][3][-1])         # NR = K = 5: the NaN comes last


@pytest.mark.parametrize('seed', range(4))
def test_generated_cases(seed):
    rng = np.random.default_rng(100 + seed)
    B, T, Cn, NR = (int(rng.integers(1, 40)), int(rng.integers(1, 24)), int(rng.integers(1, 140)), int(rng.integers(0, 20)))
    make = PC.tie_case if seed % 2 else PC.margin_case
    case = dict(make(200 + seed, B, T, Cn, NR), K=int(rng.integers(1, 17)))
    check(case, run_device(case), (B, T, Cn, NR, case['K']))


def test_outputs_that_are_not_wanted_are_not_written():
    case = CASES['c']
    ints, rels, mem = device_inputs(case)
    B, T = case['ints'].shape[:2]
    full = run_device(case)
    for keep in (('trk',), ('trk', 'top_rel_p', 'flags'), ('trk', 'cls', 'score', 'top_cls')):
        out = {k: v for k, v in fresh_outputs(case, 0x11).items() if k in keep}
        res = ops.predict_clips(ints, rels, mem, B=B, T=T, K=case['K'], out=out)
        assert set(res) == set(keep) and all(np.array_equal(res[k].cpu().numpy(), full[k]) for k in keep)
    # without rels the two relationship lists keep what they held
    out = fresh_outputs(case, 0x11)
    ops.predict_clips(ints, None, mem, B=B, T=T, K=case['K'], out=out)
    assert (out['top_rel'].view(torch.uint8) == 0x11).all() and (out['top_rel_p'].view(torch.uint8) == 0x11).all()
    assert (out['rel'] == -1).all()
    assert ops.predict_clips(ints[:0], None, None, B=0, T=T)['trk'].numel() == 0                 # B == 0: no launch


# ---- the reference's tie fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_rels', [False, True], ids=['no_rels', 'rels'])
@pytest.mark.parametrize('name', TIE_CASES)
def test_fixture_logits_equal_joint_predictions(name, with_rels):
    differ = total = 0
    for it in range(2):
        ints, rels, mem = tie_inputs(name, it)[:3]
        rels = rels if with_rels else None
        case = dict(ints=ints, rels=rels, mem=mem, mem_f64=True, K=5)
        got = run_device(case)
        want = joint_predictions(ints.copy(), rels.copy() if with_rels else None, mem)[:3]
        same = np.ones(len(ints), dtype=bool)
        for k, w in zip(INT_FIELDS, want):
            same &= got[k] == w
        if name == 'saturated':
            # a clip may differ only where the host's own sigmoid implementations disagree among themselves
            assert same[PC.sigmoids_agree(ints, rels, mem)].all(), (name, with_rels, it)
        else:
            assert same.all(), (name, with_rels, it, np.where(~same)[0])
        differ, total = differ + int((~same).sum()), total + len(ints)
    print('%s rels=%s: %d of %d clips differ from the float32 expit restatement' % (name, with_rels, differ, total))


# ---- predict() end to end -------------------------------------------------------------------------------------------------
class Unlabelled(torch.utils.data.Dataset):
    """the clips of a dataset without any of the label keys"""

    def __init__(self, base, drop=LABEL_KEYS):
        self.base, self.drop = base, drop

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        return {k: v for k, v in self.base[i].items() if k not in self.drop}


def plain_forward_cases(ds, model, batch_size, K):
    """one case (tests/predict_cases.py) per batch: the logits of a plain forward of the same batches, copied back"""
    cases = []
    model.eval()
    with torch.no_grad():
        for batch in torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False):
            out = model(batch)
            ints = out['inters'].float().cpu().numpy()
            Cn = ints.shape[-1]
            rels = out['rels'].float().cpu().numpy() if opt.ctx == 1 else None
            if opt.tr_maximize:
                bs = ints.shape[0]
                mem = batch['mem_mask'].numpy().astype(np.float32)
                ints = ints.reshape(bs, -1, Cn)
                rels = rels.reshape(bs, ints.shape[1], -1) if rels is not None else None
            else:
                bs = batch['features'].shape[0]
                mem = None
                ints = ints.reshape(bs, -1, Cn)[:, :1]                  # row 0 of each clip's group of rows
                rels = rels.reshape(bs, 1, -1) if rels is not None else None
            cases.append(dict(ints=np.ascontiguousarray(ints), rels=rels, mem=mem, K=K))
    return cases


@pytest.mark.parametrize('kind', ['modalties', 'int_rels', 'int_ch', 'int_rel_ch'])
def test_predict_end_to_end(kind, tmp_path):
    import lirec_amd
    from lirec_amd.test import testing
    from test_gpu_loops import _setup
    mk, model, loss, optim = _setup(kind, tmp_path)
    base = mk(21, 4)                                      # 21 clips in batches of 4: the last batch is a single clip
    ds = Unlabelled(base)
    assert not set(ds[0]) & set(LABEL_KEYS)
    model.train()
    pred = lirec_amd.predict(ds, model, top_k=5)
    assert model.training and pred.n_clips == 21 and lirec_amd.predict.last['n_clips'] == 21
    cases = plain_forward_cases(ds, model, 4, 5)
    assert [len(c['ints']) for c in cases] == [4, 4, 4, 4, 4, 1]
    got = {k: getattr(pred, k) for k in pred.fields if getattr(pred, k) is not None}
    assert ('top_rel' in got) == (opt.ctx == 1)
    at = 0
    for c in cases:
        n = len(c['ints'])
        check(c, {k: v[at:at + n] for k, v in got.items()}, (kind, at))
        at += n
    assert (pred.flags == 0).all()
    for k, v in got.items():                              # predict.last: the same arrays, on the device
        t = lirec_amd.predict.last[k]
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), v, equal_nan=True)
    if opt.tr_maximize:
        mem = np.concatenate([c['mem'] for c in cases])
        assert (mem[np.arange(21), pred.trk] != 0).all() and pred.trk_score.shape == mem.shape
    else:
        assert (pred.trk == 0).all() and pred.trk_score.shape == (21, 1)
    if kind not in ('modalties', 'int_rels'):
        assert pred.pairs is None
        return
    # against testing() on the labelled clips (23: no singleton batch, which testing() skips)
    base = mk(23, 4)
    pred = lirec_amd.predict(Unlabelled(base), model, top_k=5)
    testing(base, model, loss, mode='test', verbose=False)
    last = dict(testing.last)
    labels = np.array([int(np.asarray(base[i]['labels']).reshape(-1)[0]) for i in range(23)])
    assert int((pred.top_cls[:, 0] == labels).sum()) == last['precision']._top1
    if kind == 'modalties':
        assert pred.pairs is None and pred.top_rel is None and (pred.rel == -1).all()
        return
    ra = last['relationships']
    assert len(ra._gt) > 0 and list(pred.pairs) == list(ra._gt)
    assert all(np.array_equal(pred.pairs[h][1], ra._scores[h]) and pred.pairs[h][1].dtype == ra._scores[h].dtype for h in ra._gt)
    assert [int(pred.pairs[h][0][0]) for h in ra._gt] == [int(p) for _, p in ra.preds]
    # the same dataset without its hashes: everything but the pairs
    nohash = lirec_amd.predict(Unlabelled(base, drop=LABEL_KEYS + ('hash_rel',)), model)
    assert nohash.pairs is None and np.array_equal(nohash.top_rel, pred.top_rel) and np.array_equal(nohash.cls, pred.cls)


# ---- one recorded launch --------------------------------------------------------------------------------------------------
def test_recorded_launch_replays_to_the_same_bytes():
    case = CASES['bench_shape']
    ints, rels, mem = device_inputs(case)
    B, T = case['ints'].shape[:2]
    out = fresh_outputs(case, 0x7b)
    ops.CommandList.begin()
    ops.predict_clips(ints, rels, mem, B=B, T=T, K=case['K'], out=out)
    cl = ops.CommandList.end()
    try:
        assert cl.size == 1 and cl.command(0)[1] == 0
        torch.cuda.synchronize()
        first = {k: v.cpu().numpy().tobytes() for k, v in out.items()}
        check(case, {k: v.cpu().numpy() for k, v in out.items()}, 'recorded')
        for v in out.values():
            v.view(torch.uint8).fill_(0xc4)
        cl.replay()
        torch.cuda.synchronize()
        assert all(out[k].cpu().numpy().tobytes() == first[k] for k in out)
    finally:
        cl.destroy()
