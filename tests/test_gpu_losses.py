"""The tail of the hot path against float64: lirec_margin_loss in its four forms, lirec_ce_loss, lirec_heads_loss_fwd_bwd and
lirec_eval_max_tracks, across the options of their argument structs and at the track counts where the kernels change behaviour
(T > 64: the 64-lane steps of the track softmax / sampler / argmax carry state; the evaluation kernel takes its flat-argmax
branch) and LDS need (dynamic LDS above 64 KB, up to the 160 KiB the launchers admit).

Yardstick: the oracle's own loss functions on float64 logits with autograd (loss_cases.oracle64); counters against
lirec_amd.metrics.Precision, which tests/test_metrics.py pins to the reference's counters.

Bounds: the project's own (tests/test_gpu_ops.py) -- loss rtol 1e-5 / atol 1e-6, gradients rtol 1e-4 / atol 1e-7, probabilities
1e-4 / 1e-6; integers (sel_out, counters, the arrival counter) and the -inf pattern compare exactly.  No case needed a wider one:
the worst comparison of the file uses 4.3 % of its bound (a loss at T = 65; gradients 3.1 %, probabilities 0.2 %, CE 0.8 %).
The kernel's sigmoids are float32, so a hinge term within 1e-5 of 0, or two columns of a track within 1e-5 (max variant), may be
decided the other way than in float64 and move a gradient element by a whole term: those elements (rows) are left out of the
GRADIENT comparison, at most 1e-4 of a case's elements, and no clip's positive-track argmax may be that close -- the seeds are
chosen for it from the float64 oracle alone (loss_cases.seeded; tests/test_host_losses.py asserts the caps for every case here).
The loss value is continuous in these decisions and is always compared whole.
"""
import dataclasses

import numpy as np
import pytest
import torch

import loss_cases as LC
from golden_util import assert_close
from lirec_amd import ops
from oracle import lirec_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS_TOL = (1e-5, 1e-6)
GRAD_TOL = (1e-4, 1e-7)
PROB_TOL = (1e-4, 1e-6)
PAD = 7.5                     # what the padding columns of a wide logits buffer hold


def _ids(cases):
    return [LC.case_id(c) for c in cases]


def _labels(t, loader):
    return (t.long() if loader else t.int()).to(DEV).contiguous()


def _masks(t, loader):
    return (t.double() if loader else t.float()).to(DEV).contiguous()


def _logits(t, rows, n, wide):
    """[rows, n] device logits: contiguous, or columns 3 .. 3 + n of a wider buffer filled with PAD"""
    if not wide:
        return t.reshape(rows, n).to(DEV).contiguous(), None
    buf = torch.full((rows, n + 9), PAD, device=DEV)
    buf[:, 3:3 + n] = t.reshape(rows, n).to(DEV)
    return buf[:, 3:3 + n], buf


def run_kernel(case, inp, sel=None, sample=0, loader=False, wide=False, y_stride=1, divisors=None, mask_inplace=None,
               want_probs=False, seed=LC.SAMPLE_SEED):
    """One lirec_margin_loss call for the case.  Returns host copies: loss (0-dim), d_ints [B,T,C], d_rels [B,T,NR] | None,
    sel_out [B], probs [B,T] | None, the logits after the call and -- wide -- the whole buffers."""
    B, T, C, NR = case.B, case.T, case.C, case.NR
    tracks = case.form in ('margin', 'mtr')
    ints, ibuf = _logits(inp['ints'], B * T, C, wide)
    rels, rbuf = _logits(inp['rels'], B * T, NR, wide) if case.rels else (None, None)
    y = inp['y']
    if y_stride > 1:                                   # the label in place in a [B, R+1, 1] tensor; the other rows hold OTHER valid labels
        y = torch.stack([(y + j * (1 + y)) % C if j else y for j in range(y_stride)], 1).view(B, y_stride, 1)
    r = inp['r'] if tracks else inp['r'][:, 0]
    if mask_inplace is None:
        mask_inplace = tracks
    loss, d_i, d_r, sel_out, probs = ops.margin_loss(
        ints, rels,
        _masks(inp['mem'], loader) if tracks and not case.mem_null else None,
        _masks(inp['w'], loader) if not case.w_null else None,
        _labels(y, loader), _labels(r, loader) if case.rels else None,
        _labels(inp['gt'], loader) if tracks else None,
        sel.int().to(DEV) if sel is not None else None,
        B, T, C, NR if case.rels else 0, LC.MARGIN, case.lym, case.max_neg, case.tr_correct, mask_inplace,
        case.form == 'mtmm', loader_types=loader, sample=sample, sample_seed=seed, want_probs=want_probs, divisors=divisors,
        y_stride=y_stride)
    torch.cuda.synchronize()
    cpu = lambda t, *s: None if t is None else t.cpu().reshape(s)
    return dict(loss=cpu(loss), d_ints=cpu(d_i, B, T, C), d_rels=cpu(d_r, B, T, NR), sel=sel_out.cpu().long(),
                probs=cpu(probs, B, T), ints=ints.cpu().view(B, T, C), ibuf=cpu(ibuf, B * T, C + 9),
                rbuf=cpu(rbuf, B * T, NR + 9))


def compare(case, inp, got, k=None, ref=None, scale=1.0, masked=None):
    """loss, gradients (the elements whose float64 decision stands clear of rounding), the chosen track and the masked logits of one
    call against the float64 oracle.  ``k``: the positive track given to the oracle; ``ref``: an oracle64 result computed by the
    caller (the divisor cases); ``scale``: factor on the oracle's loss and gradients."""
    rs = LC.restate(case, inp, k)
    assert LC.caps_hold(case, rs, forced=k is not None), ('float64 decisions within rounding', rs['share'], rs['gap'])
    loss, d_i, d_r, xm = ref if ref is not None else LC.oracle64(case, inp, k)
    assert_close(got['loss'], loss * scale, *LOSS_TOL, 'loss')
    keep = ~rs['ex_ints']
    assert_close(got['d_ints'][keep], (d_i * scale)[keep], *GRAD_TOL, 'd_ints')
    if case.rels:
        keep = ~rs['ex_rels']
        assert_close(got['d_rels'][keep], (d_r * scale)[keep], *GRAD_TOL, 'd_rels')
    if case.form in ('margin', 'mtr'):
        assert torch.equal(got['sel'], rs['k']), ('sel_out', got['sel'].tolist(), rs['k'].tolist())
        if case.tie_clip is not None and not case.tr_correct and k is None:
            assert int(got['sel'][case.tie_clip]) == 0                          # an exact tie: the first index
    want = xm.float() if (masked if masked is not None else case.form in ('margin', 'mtr')) else inp['ints']
    assert torch.equal(got['ints'], want.view_as(got['ints'])), 'logits after the call'
    return rs


def check(case, how=None, **kw):
    case = LC.seeded(case, how)
    inp = LC.make_inputs(case)
    compare(case, inp, run_kernel(case, inp, **kw))
    return case, inp


# ---------------------------------------------------------------------------------------------------------------------------
# the four loss forms, track counts, class counts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.FORMS, ids=_ids(LC.FORMS))
def test_four_loss_forms(case):
    check(case)


@pytest.mark.parametrize('case', LC.TRACKS, ids=_ids(LC.TRACKS))
def test_track_counts_within_64k_lds(case):
    """T = 1 .. 129: one, two and three 64-lane steps of the positive-track argmax; valid prefixes that end inside the first, the
    second and the last step; a clip with a single valid track."""
    assert LC.lds_loss(case.T, case.C, case.NR, case.rels) <= 64 * 1024
    check(case)


@pytest.mark.parametrize('case', LC.BIG_LDS, ids=_ids(LC.BIG_LDS))
def test_loss_lds_above_64k(case):
    """Supported shapes by the header's own limit (160 KiB of dynamic LDS): T = 200 and the largest T the launcher admits at
    C = 101, NR = 15, and C = 1000 at T = 20.  A launch the runtime refuses surfaces here as a LirecError."""
    need = LC.lds_loss(case.T, case.C, case.NR, case.rels)
    assert 64 * 1024 < need <= LC.LDS_LIMIT
    check(case)


def test_loss_refuses_one_track_more_than_lds_holds():
    from lirec_amd._lib import LirecError
    T = LC.T_MAX + 1
    c = LC.Case('mtr', 1, T, 101, 15)
    assert LC.lds_loss(T, 101, 15) > LC.LDS_LIMIT
    with pytest.raises(LirecError):
        run_kernel(c, LC.make_inputs(c))


@pytest.mark.parametrize('case', LC.CLASSES, ids=_ids(LC.CLASSES))
def test_class_and_relationship_counts(case):
    """C = 1 .. 1000 and NR = 1 .. 70: fewer columns than a wave, one more than a wave, more than one 64-lane step of NR + 1."""
    check(case)


# ---------------------------------------------------------------------------------------------------------------------------
# the positive track: argmax, tr_correct, forced, exact ties
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.POSITIVE, ids=_ids(LC.POSITIVE))
def test_tr_correct_with_any_ground_truth_pair(case):
    """tr_correct with gt_tracks[:, 0] != 0 and with gt_tracks[:, 0] == gt_tracks[:, 1]: the positive stays track 0, the excluded
    columns and the pair's label follow the ground-truth tracks."""
    case, inp = check(case)
    assert case.g_mode != 'rand' or (inp['gt'][:, 0] != 0).any()
    if case.g_mode == 'equal':
        assert torch.equal(inp['gt'][:, 0], inp['gt'][:, 1])


@pytest.mark.parametrize('mixed', [False, True], ids=['forced', 'mixed'])
@pytest.mark.parametrize('case', LC.SEL_CASES, ids=_ids(LC.SEL_CASES))
def test_forced_positive_track(case, mixed):
    """sel forces a track other than the argmax; sel < 0 falls back to the argmax clip by clip; sel_out is what was used."""
    how = 'sel_mixed' if mixed else 'sel'
    case = LC.seeded(case, how)
    inp = LC.make_inputs(case)
    sel = LC.forced_tracks(case, inp, mixed)
    k = LC.positive(case, inp, how)
    k_arg = LC.restate(case, inp)['k_arg']
    assert ((k != k_arg) | (inp['mem'].sum(1) == 1) | (sel < 0)).all() and (k != k_arg).any()
    compare(case, inp, run_kernel(case, inp, sel=sel), k=k)


@pytest.mark.parametrize('case', LC.TIES, ids=_ids(LC.TIES))
def test_exact_tie_takes_the_first_track(case):
    check(case)


# ---------------------------------------------------------------------------------------------------------------------------
# optional inputs, strides, dtypes, divisors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.OPTIONAL, ids=_ids(LC.OPTIONAL))
def test_mem_and_w_null(case):
    check(case)


@pytest.mark.parametrize('case', LC.FORMS[5:], ids=_ids(LC.FORMS[5:]))
def test_mask_inplace_off_leaves_the_logits(case):
    """mask_inplace = 0: same loss and gradients, `ints` untouched (mask_inplace = 1, every other test: exactly the oracle's -inf)."""
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    assert (inp['mem'] == 0).any()
    compare(case, inp, run_kernel(case, inp, mask_inplace=False), masked=False)


@pytest.mark.parametrize('case', LC.STRIDES, ids=_ids(LC.STRIDES))
def test_strided_logits_and_labels_in_place(case):
    """Logits as column slices of wider buffers (ld_ints > C, ld_rels > NR) and the label read in place from a [B, R+1, 1] tensor
    (y_stride = R + 1) whose other rows hold other labels; the padding columns are unchanged afterwards."""
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    for loader in (False, True):
        got = run_kernel(case, inp, wide=True, y_stride=4, loader=loader)
        compare(case, inp, got)
        for buf, n in ((got['ibuf'], case.C), (got['rbuf'], case.NR)):
            assert bool((buf[:, :3] == PAD).all()) and bool((buf[:, 3 + n:] == PAD).all())


@pytest.mark.parametrize('case', LC.DTYPES, ids=_ids(LC.DTYPES))
def test_loader_types_bit_identical(case):
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    a, b = run_kernel(case, inp, loader=False), run_kernel(case, inp, loader=True)
    compare(case, inp, a)
    for key in ('loss', 'd_ints', 'd_rels', 'sel', 'ints'):
        assert a[key] is None or torch.equal(a[key], b[key]), key


@pytest.mark.parametrize('case', LC.DIVISORS, ids=_ids(LC.DIVISORS))
def test_divisors_as_numbers_and_as_a_device_pair(case):
    """(batch, rels) denominators: against the oracle's dp= where the function has one (MultiTaskMaxMargin), else against the
    float64 loss and gradients rescaled by B / divisor; entries <= 0 fall back to the local counts."""
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    nvalid = LC.restate(case, inp)['nvalid']
    db, dr = 1.5 * case.B, nvalid + 2.5
    dev = lambda *v: torch.tensor(v, dtype=torch.float32, device=DEV)
    for div in ((db, dr), dev(db, dr), (0.0, dr), dev(-1.0, dr), (db, 0.0), dev(db, 0.0), (0.0, 0.0), dev(0.0, -3.0)):
        b_, r_ = (float(div[0]), float(div[1]))
        got = run_kernel(case, inp, divisors=div)
        if case.form == 'mtmm':
            compare(case, inp, got, ref=LC.oracle64(case, inp, dp=(b_ if b_ > 0 else None, r_ if r_ > 0 else None)))
        else:
            compare(case, inp, got, scale=case.B / b_ if b_ > 0 else 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the in-kernel sampler
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.SAMPLER, ids=_ids(LC.SAMPLER))
def test_sampler_probabilities_and_pick(case):
    """sample = 2 (probabilities and the draw only) at T = 20, 65, 200: probs_out against the float64 softmax (the rels mix with
    NaN -> 0; one clip's pair is labelled None), sel_out equal to the oracle's sampler on the kernel's OWN probabilities for
    several keys, padded tracks never picked."""
    case = LC.seeded(case, 'sample')
    inp = LC.make_inputs(case)
    if case.rels:
        b = case.r0_none[0]
        assert int(inp['r'][b, inp['gt'][b, 0]]) == case.NR
    p64 = LC.probs64(case, inp)
    assert bool(torch.isfinite(p64).all())
    later = 0
    for i in range(8):
        seed = LC.SAMPLE_SEED + 0x100000001 * i
        got = run_kernel(case, inp, sample=2, seed=seed)
        assert_close(got['probs'], p64, *PROB_TOL, 'probs_out')
        want = O.PhiloxTrackSampler(seed)(got['probs'])
        assert torch.equal(got['sel'], want), (seed, got['sel'].tolist(), want.tolist())
        assert bool((inp['mem'][torch.arange(case.B), got['sel']] == 1).all()), 'a padded track was picked'
        later += int((got['sel'] >= 64).sum())
    assert case.T < 128 or later > 0                 # (picks beyond the first 64-lane step did occur)


@pytest.mark.parametrize('max_neg', [False, True], ids=['sum', 'max'])
@pytest.mark.parametrize('case', LC.SAMPLER, ids=_ids(LC.SAMPLER))
def test_sampled_loss_against_the_oracle_given_the_pick(case, max_neg):
    """sample = 1: the same probabilities and pick as sample = 2, and loss and gradients equal the oracle's with that pick."""
    case = LC.seeded(dataclasses.replace(case, max_neg=max_neg), 'sample')
    inp = LC.make_inputs(case)
    draw = run_kernel(case, inp, sample=2)
    got = run_kernel(case, inp, sample=1, want_probs=True)
    assert torch.equal(got['probs'], draw['probs']) and torch.equal(got['sel'], draw['sel'])
    k = O.PhiloxTrackSampler(LC.SAMPLE_SEED)(got['probs'])
    compare(case, inp, got, k=k)


# ---------------------------------------------------------------------------------------------------------------------------
# the two forms of the finalize
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.FINALIZE, ids=_ids(LC.FINALIZE))
def test_two_launch_finalize_and_arrival_counter(case, monkeypatch):
    """arrive == NULL (the C ABI's two-launch form, which ops.margin_loss never uses): loss within the bound of float64.  With
    `arrive`: the counter is zero afterwards and ten repeated launches give a bit-identical loss."""
    case = LC.seeded(case)
    inp = LC.make_inputs(case)
    monkeypatch.setattr(ops, '_arrive_counter', lambda dev: None)             # -> a.arrive = NULL
    two = run_kernel(case, inp)
    compare(case, inp, two)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    monkeypatch.setattr(ops, '_arrive_counter', lambda dev: ctr)
    runs = []
    for _ in range(10):
        runs.append(run_kernel(case, inp))
        assert int(ctr.item()) == 0
    compare(case, inp, runs[0])
    for r_ in runs[1:]:
        assert torch.equal(r_['loss'], runs[0]['loss']) and torch.equal(r_['d_ints'], runs[0]['d_ints'])
    assert torch.equal(two['d_ints'], runs[0]['d_ints']) and torch.equal(two['d_rels'], runs[0]['d_rels'])


# ---------------------------------------------------------------------------------------------------------------------------
# heads forward + loss + heads' data gradients in one call, beyond one 64-lane step and beyond 64 KB of LDS
# ---------------------------------------------------------------------------------------------------------------------------
def _P(t):
    return t.data_ptr()


@pytest.mark.parametrize('T,with_rels', LC.FUSED)
def test_fused_heads_loss_call_equals_the_three_calls(T, with_rels):
    """tests/test_gpu_ops.py:test_heads_loss_fwd_bwd_equals_the_three_calls at T = 65 and T = 200: bit for bit."""
    g = torch.Generator().manual_seed(77 + T)
    B, C_, NR, KG, KC = 3, 101, 15, 512, 256
    n = B * T
    G = torch.randn(n, KG, generator=g).to(DEV)
    E = torch.randn(n, KC, generator=g).to(DEV)
    Wi, bi = (torch.randn(C_, KG, generator=g) / KG ** 0.5).to(DEV), torch.randn(C_, generator=g).to(DEV)
    Wc, bc = (torch.randn(NR, KC, generator=g) / KC ** 0.5).to(DEV), torch.randn(NR, generator=g).to(DEV)
    nb = torch.tensor([T, 64 + 1, 7])
    mem = (torch.arange(T)[None, :] < nb[:, None]).float().to(DEV)
    w = (torch.rand(B, C_, generator=g) < 0.95).float().to(DEV)
    y = torch.randint(0, C_, (B,), generator=g, dtype=torch.int32).to(DEV)
    r = torch.randint(0, NR + 1, (B, T), generator=g, dtype=torch.int32).to(DEV)
    gt = torch.zeros(B, 2, dtype=torch.int32, device=DEV)
    res = []
    for fused in (False, True):
        Yi, Yc = torch.empty(n, C_, device=DEV), torch.zeros(n, NR, device=DEV)
        dG, dE = torch.full((n, KG), 3.0, device=DEV), torch.full((n, KC), 3.0, device=DEV)
        dWi, dbi = torch.zeros_like(Wi), torch.zeros_like(bi)
        dWc, dbc = torch.zeros_like(Wc), torch.zeros_like(bc)
        heads = [(_P(G), KG, Wi, bi, n, KG, C_, Yi, C_)] + ([(_P(E), KC, Wc, bc, n, KC, NR, Yc, NR)] if with_rels else [])
        drop = ops.make_dropout(0, 0.0)
        back = lambda di, dc: [(di, C_, _P(G), KG, Wi, n, KG, C_, dWi, dbi, _P(dG), KG, 0, None, KG, 0, drop)] + \
            ([(dc, NR, _P(E), KC, Wc, n, KC, NR, dWc, dbc, _P(dE), KC, 0, None, KC, 0, drop)] if with_rels else [])
        kw = dict(mem=mem, w=w, y=y, r=r if with_rels else None, g=gt, sel=None, B=B, T=T, Cc=C_, NR=NR if with_rels else 0,
                  margin=0.101, lymbda=1.0, max_neg=False, tr_correct=False, mask_inplace=True, rels_mean_valid=False)
        if fused:
            loss, d_i, d_c, sel, _ = ops.margin_loss(Yi, Yc if with_rels else None, heads=heads, back=back('ints', 'rels'), **kw)
        else:
            ops.linear_fwd_group(heads)
            loss, d_i, d_c, sel, _ = ops.margin_loss(Yi, Yc if with_rels else None, **kw)
            ops.linear_bwd_group(back(d_i, d_c), parts=2)
        torch.cuda.synchronize()
        assert not dWi.any() and not dbi.any() and not dWc.any()
        res.append([t.clone() for t in (Yi, Yc, loss, d_i, dG, dE, sel)] + ([d_c.clone()] if with_rels else []))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.isfinite(res[0][2]).all() and float(res[0][4].abs().sum()) > 0
    assert bool(torch.isinf(res[0][0]).any())                              # (the -inf mask was written)


# ---------------------------------------------------------------------------------------------------------------------------
# lirec_ce_loss
# ---------------------------------------------------------------------------------------------------------------------------
def _ce_inputs(B, C, NR, seed, labels):
    g = np.random.Generator(np.random.PCG64(seed))
    ints = torch.from_numpy(g.standard_normal((B, C)).astype(np.float32)) * 2
    rels = torch.from_numpy(g.standard_normal((B, NR)).astype(np.float32)) * 2
    y = torch.from_numpy(g.integers(0, C, B))
    r = torch.from_numpy(g.integers(0, NR + 1, B))
    r[0], r[B - 1] = NR, 0
    if labels == 'none':
        r[:] = NR
    cw = torch.from_numpy(g.uniform(0.25, 4.0, C).astype(np.float32))
    return ints, rels, y, r, cw


def _ce_check(ints, rels, y, r, cw, NR, got, dp=None):
    oi, orl = ints.double().requires_grad_(True), rels.double().requires_grad_(True)
    ol = O.multitask_ce_loss({'inters': oi, 'rels': orl}, {'labels': y, 'rels_label': r}, NR,
                             weights=cw.double() if cw is not None else None, dp=dp)
    assert ol.dtype == torch.float64
    ol.backward()
    loss, d_i, d_r = got
    torch.cuda.synchronize()
    assert_close(loss.cpu(), ol.detach(), *LOSS_TOL, 'ce loss')
    assert_close(d_i.cpu(), oi.grad, *GRAD_TOL, 'd_ints')
    assert_close(d_r.cpu(), orl.grad if orl.grad is not None else torch.zeros_like(rels), *GRAD_TOL, 'd_rels')


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'class_w'])
@pytest.mark.parametrize('labels', ['mixed', 'none'])
@pytest.mark.parametrize('NR', [1, 15])
@pytest.mark.parametrize('C', [1, 101, 257, 1000])
def test_ce_loss(C, NR, labels, weighted):
    B = 9
    ints, rels, y, r, cw = _ce_inputs(B, C, NR, 2000 + C + NR, labels)
    cw = cw if weighted else None
    dv = lambda t: None if t is None else t.to(DEV)
    got = ops.ce_loss(dv(ints), dv(rels), dv(y.int()), dv(r.int()), dv(cw), B, C, NR)
    _ce_check(ints, rels, y, r, cw, NR, got)


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'class_w'])
def test_ce_loss_divisors_and_strided_logits(weighted):
    B, C, NR = 9, 101, 15
    ints, rels, y, r, cw = _ce_inputs(B, C, NR, 2100, 'mixed')
    cw = cw if weighted else None
    dv = lambda t: None if t is None else t.to(DEV)
    own = (float(cw[y].sum()) if weighted else float(B), float((r != NR).sum()))
    di, dr = 1.75 * own[0], own[1] + 2.5
    for wide in (False, True):
        i_d, ibuf = _logits(ints, B, C, wide)
        r_d, rbuf = _logits(rels, B, NR, wide)
        for div in ((di, dr), torch.tensor([di, dr], device=DEV), (0.0, dr), torch.tensor([di, -1.0], device=DEV), None):
            got = ops.ce_loss(i_d, r_d, dv(y.int()), dv(r.int()), dv(cw), B, C, NR, divisors=div)
            d0, d1 = (0.0, 0.0) if div is None else (float(div[0]), float(div[1]))
            _ce_check(ints, rels, y, r, cw, NR, got, dp=(d0 if d0 > 0 else own[0], d1 if d1 > 0 else own[1]))
        if wide:
            for buf, n, src in ((ibuf, C, ints), (rbuf, NR, rels)):
                buf = buf.cpu()
                assert bool((buf[:, :3] == PAD).all()) and bool((buf[:, 3 + n:] == PAD).all()) and torch.equal(buf[:, 3:3 + n], src)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluation counters: the T <= 64 two-stage search, the T > 64 flat argmax, LDS above 64 KB
# ---------------------------------------------------------------------------------------------------------------------------
T_EVAL_MAX = LC.largest_T(LC.lds_eval, 101, 15)        # 173


def _eval_batches(B, T, Cc, NR, quantized, seed, n=3):
    """The batches of tests/test_gpu_ops.py:test_eval_max_tracks_counters: random or quantized logits, ties, saturated rows,
    just_zeros, a clip without a second ground-truth track."""
    g = torch.Generator().manual_seed(seed)
    for it in range(n):
        ints = torch.randn(B, T, Cc, generator=g) * 3
        rels = torch.randn(B, T, NR, generator=g) * 3
        if quantized:
            vals = torch.tensor([-2.0, 0.0, 2.0, 15.0, 16.0, 17.0, 18.0, 19.0, 20.0])
            ints = vals[torch.randint(0, len(vals), (B, T, Cc), generator=g)]
            rels = vals[torch.randint(0, len(vals), (B, T, NR), generator=g)]
        ints[0, :, :] = 0.0
        ints[1 % B, 0, :] = 40.0
        nb = torch.randint(1, T + 1, (B,), generator=g)
        nb[3 % B] = T                                      # (one clip uses every track)
        mem = (torch.arange(T)[None, :] < nb[:, None]).double()
        y = torch.randint(0, Cc, (B,), generator=g)
        r = torch.randint(0, NR + 1, (B, T), generator=g)
        gt = torch.stack([torch.zeros(B, dtype=torch.int64), (torch.rand(B, generator=g) * nb).long()], 1)
        gt[2 % B, 1] = 0
        jz = torch.rand(B, generator=g) < 0.2
        jz[0] = False
        # Joint hits: with random labels the joint (track, class, relationship) prediction is right about once in T * C * (NR + 1)
        # clips, and a wrong decode of the flat argmax would count the same zeros.  Every third clip from the fourth on gets its
        # label planted as the joint maximum at the first ground-truth track, the next one at the second (any track of the clip,
        # beyond the first 64 too): random logits get one saturated entry; quantized ones -- where numpy's FIRST flat index among
        # the saturated entries decides -- lose the saturated entries in front of the planted one.
        for b in range(3, B):
            if b % 3 == 2:
                continue
            t = int(gt[b, b % 3])
            r[b, 0] = r[b, 0] % NR
            r0 = int(r[b, 0])
            if quantized:
                for x, col in ((ints, int(y[b])), (rels, r0)):
                    front = x[b, :t]
                    front[front >= 15] = -2.0
                    x[b, t, :col] = -2.0
                    x[b, t, col] = 20.0
            else:
                ints[b, t, y[b]] = 25.0
                rels[b, t, r0] = 25.0
        yield ints, rels, mem, y, r, gt, jz


def _eval_device(batches, B, T, Cc, NR, with_rels):
    counters = torch.zeros(8, dtype=torch.int64, device=DEV)
    for ints, rels, mem, y, r, gt, jz in batches:
        ops.eval_max_tracks(ints.reshape(B * T, Cc).to(DEV), rels.reshape(B * T, NR).to(DEV) if with_rels else None,
                            mem.to(DEV), y.to(DEV), r.to(DEV) if with_rels else None, gt.to(DEV), jz.to(DEV), counters,
                            B, T, Cc, NR if with_rels else 0, loader_types=True)
    torch.cuda.synchronize()
    return dict(zip(ops.EVAL_COUNTERS, counters.cpu().tolist()))


def _eval_host(batches, NR, with_rels):
    from lirec_amd.metrics import Precision
    host = Precision(n_rels=NR)
    for ints, rels, mem, y, r, gt, jz in batches:
        if with_rels:
            rels_mask = torch.nonzero(r[:, 0] - (NR + 1) + 1)
            host.update_probs_max_tracks_rels(ints.clone(), rels.clone(), y, r, gt_tracks=gt, just_zeros=jz, mask=mem,
                                              rels_mask=rels_mask)
        else:
            host.update_probs_max_tracks(ints.clone(), gt_tracks=gt, gt_classes=y, mask=mem, just_zeros=jz)
    return {k: int(getattr(host, k)) for k in ops.EVAL_COUNTERS}


def _eval_case(T, with_rels, quantized):
    B, Cc, NR = 12, 101, 15
    batches = list(_eval_batches(B, T, Cc, NR, quantized, 31 * T + int(with_rels) + 2 * int(quantized)))
    got, want = _eval_device(batches, B, T, Cc, NR, with_rels), _eval_host(batches, NR, with_rels)
    assert want['total'] > 0 and want['_top1'] >= 3 and got == want, (got, want)          # (the joint prediction has hits to count)


@pytest.mark.parametrize('quantized', [False, True], ids=['random', 'quantized'])
@pytest.mark.parametrize('with_rels', [False, True], ids=['ints', 'rels'])
@pytest.mark.parametrize('T', [63, 64, 65])
def test_eval_counters_around_64_tracks(T, with_rels, quantized):
    """T = 63, 64: the two-stage search; T = 65: the flat argmax over T * C * (NR + 1), inside 64 KB of LDS."""
    assert LC.lds_eval(T, 101, 15, with_rels) <= 64 * 1024
    _eval_case(T, with_rels, quantized)


@pytest.mark.parametrize('quantized', [False, True], ids=['random', 'quantized'])
@pytest.mark.parametrize('with_rels', [False, True], ids=['ints', 'rels'])
@pytest.mark.parametrize('T', [129, T_EVAL_MAX])
def test_eval_lds_above_64k(T, with_rels, quantized):
    """T = 129 and the largest T the launcher admits with rels (173): supported shapes by the 160 KiB limit."""
    assert 64 * 1024 < LC.lds_eval(T, 101, 15, with_rels) <= LC.LDS_LIMIT
    _eval_case(T, with_rels, quantized)


def test_eval_refuses_one_track_more_than_lds_holds():
    from lirec_amd._lib import LirecError
    T = T_EVAL_MAX + 1
    batches = list(_eval_batches(2, T, 101, 15, False, 5, n=1))
    with pytest.raises(LirecError):
        _eval_device(batches, 2, T, 101, 15, True)


@pytest.mark.parametrize('quantized', [False, True], ids=['random', 'quantized'])
@pytest.mark.parametrize('with_rels', [False, True], ids=['ints', 'rels'])
def test_eval_padding_to_65_tracks_changes_nothing(with_rels, quantized):
    """The same clips at T = 64 (two-stage search) and padded to T = 65 with one masked track of arbitrary logits (flat argmax):
    equal counters, and equal to the host's."""
    B, Cc, NR = 12, 101, 15
    a = list(_eval_batches(B, 64, Cc, NR, quantized, 4242 + int(with_rels)))
    pad = torch.Generator().manual_seed(9)
    b = []
    for ints, rels, mem, y, r, gt, jz in a:
        b.append((torch.cat([ints, torch.randn(B, 1, Cc, generator=pad) * 50], 1), torch.cat([rels, torch.randn(B, 1, NR, generator=pad) * 50], 1),
                  torch.cat([mem, torch.zeros(B, 1, dtype=mem.dtype)], 1), y, torch.cat([r, torch.zeros(B, 1, dtype=r.dtype)], 1), gt, jz))
    ga, gb = _eval_device(a, B, 64, Cc, NR, with_rels), _eval_device(b, B, 65, Cc, NR, with_rels)
    assert ga == gb == _eval_host(a, NR, with_rels), (ga, gb)
