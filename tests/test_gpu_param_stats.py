"""lirec_param_stats and FusedAdam.param_stats() / nonfinite_params() on the GPU, against the float64 yardstick of
tests/param_stats_cases.py (sums formed exactly with math.fsum; maxima and counts plain).

Tolerances (param_stats_cases.sum_bounds, derived there): counts and maxima exact; gradient and parameter sums within relative
n 2^-53 of the exact sum (n the range's length: exact non-negative terms, any order of float64 additions); update sums within
(n + 16) 2^-53 (the kernel's arithmetic needs n + 10: eleven roundings a term, n - 1 additions); the same launch twice gives the
same bits; groups not asked for are exactly 0.  Norms are taken after the root: half the sum's bound plus one rounding, plus one more
where a scale or a learning rate is multiplied on.

The kernel cases cross the lengths 0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4097 with offsets = 0, 1, 2, 3 (mod 4), from a
16-byte-aligned base and from bases 4 bytes off it; tables of 1, 2, 63 and 64 entries, adjacent and with gaps, one range of 200 001
elements among tiny ones; every value of flags; a NaN / +-Inf at the first, the last and a 4-element-boundary element of a range in
each buffer in turn, and a negative v.  No case holds more than 300 000 elements but one, test_more_blocks_than_workgroups, which
says why.  The workspace and the output are handed over filled with NaN: nothing may depend on their content."""
import numpy as np
import pytest
import torch

import param_stats_cases as PC
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt
from lirec_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)
B, LR = 4, 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel against the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def _on_device(x, off):
    """``x`` (numpy fp32) at ``off`` elements past a 16-byte boundary of device memory"""
    raw = torch.empty(x.size + 8, dtype=torch.float32, device=DEV)
    lead = ((-raw.data_ptr()) % 16) // 4 + off
    t = raw[lead:lead + x.size]
    assert (t.data_ptr() - 4 * off) % 16 == 0
    t.copy_(torch.from_numpy(x))
    return t


def _launch(bufs, entries, offs=(0, 0, 0, 0), twice=True):
    """one lirec_param_stats call (``twice``: issued again into a second table, which must hold the same bits); float64 [n, 9]"""
    dev = [None if b is None else _on_device(b, o) for b, o in zip(bufs, offs)]
    ws = torch.full((ops.param_stats_ws_bytes(len(entries)) // 8,), float('nan'), dtype=torch.float64, device=DEV)
    outs = []
    for _ in range(2 if twice else 1):
        out = torch.full((len(entries), PC.COLS), float('nan'), dtype=torch.float64, device=DEV)
        ops.param_stats(*dev, entries, out, ws)
        outs.append(out)
    torch.cuda.synchronize()
    got = outs[0].cpu().numpy()
    if twice:
        assert np.array_equal(got.view(np.int64), outs[1].cpu().numpy().view(np.int64)), 'two launches, two results'
    return got


_CROSSED = {}


def _crossed():
    """the crossed table, its buffers and its reference: computed once, shared, never changed"""
    if not _CROSSED:
        ent, extent = PC.crossed_entries()
        bufs = PC.buffers(extent + 5, 3)
        _CROSSED.update(ent=ent, bufs=bufs, want=PC.reference(*bufs, ent))
    return _CROSSED['ent'], _CROSSED['bufs'], _CROSSED['want']


@pytest.mark.parametrize('offs', [(0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (1, 0, 2, 3)],
                         ids=['aligned', 'all_4_bytes_off', 'all_12_bytes_off', 'each_off_differently'])
def test_lengths_cross_offsets_cross_bases(offs):
    """48 ranges in one table: every length at every offset modulo 4, from an aligned base (f32x4 bodies, scalar heads and tails) and
    from bases off alignment (the scalar fall-back) -- the same BITS from every base: the result follows from values and table alone"""
    ent, bufs, want = _crossed()
    got = _launch(bufs, ent, offs)
    print('PSTAT-FIGURE crossed offs=%s worst use of a sum bound %.3f' % (offs, PC.check(got, want, ent, offs)))
    aligned = _launch(bufs, ent, twice=False)
    assert np.array_equal(got.view(np.int64), aligned.view(np.int64)), 'the bits depend on where the buffers lie'


@pytest.mark.parametrize('count', [1, 2, 63, 64])
def test_table_sizes(count):
    """1, 2, 63 and 64 entries, taken from the crossed table (adjacent ranges and gaps, every alignment) from its longest ranges
    down; each row equals the row the 48-entry table gives: a range's result does not depend on its neighbours in the table"""
    ent, bufs, want = _crossed()
    order = sorted(range(len(ent)), key=lambda i: -ent[i][1])
    pick = [order[i % len(order)] for i in range(count)]          # (63 / 64: some ranges twice -- overlapping entries are legal)
    got = _launch(bufs, [ent[i] for i in pick])
    PC.check(got, want[pick], [ent[i] for i in pick], count)
    whole = _launch(bufs, ent, twice=False)
    assert np.array_equal(got.view(np.int64), whole[pick].view(np.int64))


def test_one_long_range_among_tiny_ones():
    """200 001 elements at an odd offset (196 blocks: 196 workgroups of the fixed grid hold a partial of it, the others none)
    between ranges of 0 .. 7 elements, adjacent and with gaps"""
    n = PC.LONG
    ent, at = [], 0
    for k in (1, 2, 3):
        ent.append((at, k, 7) + PC.FACTORS)
        at += k + (k % 2)
    at += 1
    ent.append((at, n, 7) + PC.FACTORS)
    at += n
    for k in (7, 0, 4, 5):
        ent.append((at, k, 7) + PC.FACTORS)
        at += k + 3 * (k % 2)
    assert at <= 300000 and ent[3][0] % 4 != 0
    bufs = PC.buffers(at, 7)
    want = PC.reference(*bufs, ent)
    for offs in ((0, 0, 0, 0), (1, 1, 1, 1)):
        got = _launch(bufs, ent, offs, twice=(offs[0] == 0))
        print('PSTAT-FIGURE long offs=%s worst use %.3f' % (offs, PC.check(got, want, ent, offs)))


def test_more_blocks_than_workgroups():
    """THE ONE CASE ABOVE 300 000 ELEMENTS, because the path exists at no smaller size: the grid is 1024 workgroups of one
    1024-element block each, so only a table of more than 2^20 elements makes a workgroup take a SECOND block (every launch at a
    real model's size does) and makes the second launch see a range that every workgroup touched.  One range of 2^20 + 2085
    elements (1027 blocks: workgroups 0 .. 2 take two), gradient and parameter columns only, and two small ranges behind it whose
    blocks land on workgroups 3 .. 5 -- the numbering wrapped round the grid."""
    n = 1024 * 1024 + 2085
    ent = [(2, n, 3), (n + 7, 1500, 7) + PC.FACTORS, (n + 1507, 3, 7) + PC.FACTORS]
    bufs = PC.buffers(n + 1510, 9)
    want = PC.reference(*bufs, ent)
    for offs in ((0, 0, 0, 0), (1, 1, 1, 1)):
        got = _launch(bufs, ent, offs, twice=(offs[0] == 0))
        print('PSTAT-FIGURE wrapped offs=%s worst use %.3f' % (offs, PC.check(got, want, ent, offs)))


@pytest.mark.parametrize('flags', [1, 2, 3, 4, 5, 6, 7, 'mixed'])
def test_flags(flags):
    """each value of flags on every range, and a table that mixes all eight; a group that is not asked for is exactly 0 and its
    buffers may be missing"""
    ent, bufs, _ = _crossed()
    ent = [e[:2] + (((i % 8) if flags == 'mixed' else flags),) + e[3:] for i, e in enumerate(ent)]
    want = PC.reference(*bufs, ent)
    PC.check(_launch(bufs, ent), want, ent, flags)
    if flags != 'mixed':
        p, g, m, v = bufs
        fewer = (p if flags & 2 else None, g if flags & 1 else None, m if flags & 4 else None, v if flags & 4 else None)
        assert np.array_equal(_launch(fewer, ent, twice=False).view(np.int64), _launch(bufs, ent, twice=False).view(np.int64))


@pytest.mark.parametrize('which', ['p', 'g', 'm', 'v'])
def test_nonfinite_values_are_counted_where_they_are(which):
    """NaN, +Inf and -Inf at the first element, at the last and at both sides of a 4-element boundary of a range, in one buffer at a
    time; the ranges start at every offset modulo 4, run past one block, and their neighbours stay clean.  v also takes a negative
    element.  Counted in the right row and column, left out of that row's sum and maximum, everything else untouched."""
    clean = PC.buffers(8 * 1100 + 64, 13, dirty=False)
    ent, at = [], 0
    for r in range(8):
        at += (r - at) % 4
        ent.append((at, 1029 + r, 7) + PC.FACTORS)
        at += 1029 + r + (r % 3)
    base = PC.reference(*clean, ent)
    assert (base[:, [2, 5, 8]] == 0).all()
    bufs = [b.copy() for b in clean]
    x = bufs['pgmv'.index(which)]
    want_bad, planted = np.zeros(len(ent)), np.zeros(len(ent), bool)
    for r, bad in zip((0, 1, 2, 3, 5, 6), (np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan)):
        off, n = ent[r][:2]
        spots = {off, off + n - 1, (off + 3) // 4 * 4 + 4, (off + 3) // 4 * 4 + 3, (off // 4) * 4 + 1024, (off // 4) * 4 + 1023}
        for s in spots:
            x[s] = bad
        want_bad[r], planted[r] = len(spots), True
    if which == 'v':
        x[ent[4][0] + 5] = -1e-6
        want_bad[4], planted[4] = 1, True
    want = PC.reference(*bufs, ent)
    col = {'g': 2, 'p': 5, 'm': 8, 'v': 8}[which]
    if which == 'v':
        # +Inf in v with a finite m gives u = 0, a finite value (include/lirec_hip.h); NaN, -Inf and the negative element give NaN
        want_bad = np.array([6, 0, 6, 6, 1, 0, 6, 0], np.float64)
    assert (want[:, col] == want_bad).all() and (np.delete(want[:, [2, 5, 8]], [2, 5, 8].index(col), axis=1) == 0).all()
    for offs in ((0, 0, 0, 0), (2, 2, 2, 2)):
        got = _launch(bufs, ent, offs, twice=False)
        PC.check(got, want, ent, (which, offs))
        assert np.isfinite(got).all()
        # the rows and groups without a planted value keep the clean table's bits
        same = np.ones_like(got, bool)
        same[planted, col - 2:col + 1] = False
        assert np.array_equal(got[same].view(np.int64), _launch(clean, ent, twice=False)[same].view(np.int64))


def test_all_special_values_in_one_range():
    x = np.array([np.nan, np.inf, -np.inf, -0.0, PC.DENORMAL, PC.FLT_MAX], np.float32)
    one = np.ones(6, np.float32)
    ent = [(0, 6, 3), (3, 2, 3), (3, 1, 3)]
    got = _launch((x, x, one, one), ent)
    PC.check(got, PC.reference(x, x, one, one, ent), ent)
    assert got[0, 0] == PC.FLT_MAX ** 2 and got[0, 1] == PC.FLT_MAX and got[0, 2] == 3      # FLT_MAX squared is summed, not counted
    assert got[1, 0] == PC.DENORMAL ** 2 > 0 and got[1, 1] == PC.DENORMAL                # a denormal is an ordinary value
    assert (got[2] == 0).all() and not np.signbit(got[2]).any()                         # -0: sum, maximum and count +0


# ---------------------------------------------------------------------------------------------------------------------------
# through the optimiser
# ---------------------------------------------------------------------------------------------------------------------------
def _make(seed=11, dropout=0.0, **flags):
    from lirec_amd import model as M
    config.recipe('int_rel_ch', joint_dim=16, dropout=dropout, dropout_seed=77, lr=LR, rels_n_clips=3, **DIMS, **flags)
    opt.device = 'cuda'
    torch.manual_seed(seed)
    model, loss, optim = M.create_model(11, n_rels=5)
    model.train()
    return model, loss, optim


def _batch(seed=21):
    from lirec_amd.data import synthetic_batch, to_device_batch
    return to_device_batch(synthetic_batch(seed, 'int_rel_ch', B, T=4, R=3, n_classes=11, n_rels=5, **DIMS), 'cuda')


def _backward(model, loss, optim, batch):
    optim.zero_grad()
    loss(model(dict(batch)), batch).backward()


def _step(model, loss, optim, batch):
    _backward(model, loss, optim, batch)
    optim.step()


def _np(t):
    return t.detach().double().cpu().numpy().ravel()


def _f32(t):
    return t.detach().float().cpu().numpy().ravel()


def _close(got, want, bound, what):
    assert (got is None) == (want is None), what
    if want is not None:
        assert abs(got - want) <= bound * abs(want), (what, got, want, bound)


def _expect(model, optim, name, steps, scale=1.0, grad=True, update=True):
    """one parameter's ParamStat from float64 arithmetic on p, p.grad and state[p] (the exact sums of the yardstick), with the bound
    of each norm; ``steps``: the updates the parameter has received"""
    p = dict(model.named_parameters())[name]
    grp = optim.param_groups[optim._group_of[name]]
    n = p.numel()
    st = optim.state[p]
    z = np.zeros(n, np.float32)
    fac = FusedAdam.stat_factors(steps, *grp['betas']) + (grp['eps'],) if steps >= 1 else (1.0, 1.0, 0.0)
    flags = 2 | (1 if grad else 0) | (4 if update and steps >= 1 else 0)
    row = PC.row(_f32(p), _f32(p.grad) if grad else z, _f32(st['exp_avg']), _f32(st['exp_avg_sq']), (0, n, flags) + fac)
    bg, bu = PC.norm_bound(n * PC.U) + PC.U, PC.norm_bound((n + 16) * PC.U) + PC.U        # (+ one rounding: the scale / the lr)
    want = dict(grad_norm=row[0] ** 0.5 * scale if grad else None, grad_absmax=row[1] * scale if grad else None,
                grad_nonfinite=int(row[2]) if grad else None, param_norm=row[3] ** 0.5, param_absmax=row[4], param_nonfinite=int(row[5]),
                update_norm=grp['lr'] * row[6] ** 0.5 if flags & 4 else None, update_absmax=grp['lr'] * row[7] if flags & 4 else None,
                update_nonfinite=int(row[8]) if flags & 4 else None)
    return want, bg, bu


def _check_param(got, want, bg, bu, name):
    for k in ('grad_nonfinite', 'param_nonfinite', 'update_nonfinite', 'param_absmax'):
        assert getattr(got, k) == want[k], (name, k, getattr(got, k), want[k])
    _close(got.grad_norm, want['grad_norm'], bg, (name, 'grad_norm'))
    _close(got.grad_absmax, want['grad_absmax'], PC.U, (name, 'grad_absmax'))
    _close(got.param_norm, want['param_norm'], bg, (name, 'param_norm'))
    _close(got.update_norm, want['update_norm'], bu, (name, 'update_norm'))
    _close(got.update_absmax, want['update_absmax'], 12 * PC.U, (name, 'update_absmax'))      # (five roundings of u, the lr's one; twice over)
    if want['update_norm'] is None or not want['param_norm']:
        assert got.update_ratio is None, name
    else:
        _close(got.update_ratio, want['update_norm'] / want['param_norm'], bg + bu + PC.U, (name, 'update_ratio'))


def test_two_eager_steps_against_float64():
    """before any step the update columns are None; after two eager steps every column of every parameter matches float64
    arithmetic on p, p.grad, exp_avg and exp_avg_sq; the table is float64 [P, 9] on the device, one row per parameter in
    named_parameters() order, and a second call gives the same bits"""
    try:
        model, loss, optim = _make()
        batch = _batch()
        names = [n for n, _ in model.named_parameters()]
        _backward(model, loss, optim, batch)
        h = optim.param_stats().host()
        assert list(h) == names
        for n in names:
            assert h[n].update_norm is None and h[n].update_absmax is None and h[n].update_nonfinite is None and h[n].update_ratio is None
            assert h[n].grad_norm is not None and h[n].param_norm is not None
        optim.step()
        _step(model, loss, optim, batch)
        st = optim.param_stats()
        assert st.names == names and st.table.is_cuda and st.table.dtype == torch.float64 and tuple(st.table.shape) == (len(names), 9)
        again = optim.param_stats()
        torch.cuda.synchronize()
        assert torch.equal(st.table.view(torch.int64), again.table.view(torch.int64))
        h = st.host()
        assert sum(v.grad_norm > 0 for v in h.values()) > len(names) // 2 and all(v.update_ratio is None or v.update_ratio > 0 for v in h.values())
        for n in names:
            _check_param(h[n], *_expect(model, optim, n, 2), n)
        noup = optim.param_stats(update=False).host()
        for n in names:
            assert noup[n].update_norm is None and noup[n].grad_norm == h[n].grad_norm and noup[n].param_norm == h[n].param_norm
    finally:
        config.reset()


def test_combined_norm_is_the_clipped_steps_norm():
    """max_grad_norm set: the root of the sum of column 0 over the trainable parameters, times the scale, is optimizer.grad_norm
    to the fp32 rounding of that scalar (relative 2^-23) -- with one parameter frozen, whose slice of the buffer is filled with
    1e30 and must stay out of both"""
    try:
        model, loss, optim = _make()
        batch = _batch()
        optim.max_grad_norm = 0.05
        optim.grad_scale = 0.5
        frozen = next(n for n, _ in model.named_parameters() if n.endswith('.weight'))
        dict(model.named_parameters())[frozen].requires_grad_(False)
        _backward(model, loss, optim, batch)
        o, k = model._offsets[frozen]
        model.flat_grads(attach=False)[o:o + k] = 1e30
        optim.step()
        st = optim.param_stats()
        torch.cuda.synchronize()
        live = torch.tensor([bool(f & _lib.STAT_GRAD) for f in st.flags], device=DEV)
        assert int((~live).sum()) == 1
        total = float(st.table[live, 0].sum().sqrt()) * st.scale
        norm = float(optim.grad_norm)
        assert norm > 0 and st.scale == 0.5 and abs(total - norm) <= 2.0 ** -23 * norm, (total, norm)
        h = st.host()
        assert abs(sum(v.grad_norm ** 2 for v in h.values() if v.grad_norm is not None) ** 0.5 - norm) <= 2.0 ** -23 * norm
    finally:
        config.reset()


def test_frozen_parameters():
    """frozen from the start: gradient and update columns None, parameter columns present; frozen after one update: no gradient
    columns, the update columns of ITS one update (t = 1) while the others are at t = 2"""
    try:
        model, loss, optim = _make()
        batch = _batch()
        names = [n for n, _ in model.named_parameters()]
        params = dict(model.named_parameters())
        never, later = names[0], names[3]
        params[never].requires_grad_(False)
        _step(model, loss, optim, batch)
        params[later].requires_grad_(False)
        _step(model, loss, optim, batch)
        h = optim.param_stats().host()
        assert h[never][:3] == (None, None, None) and h[never][6:] == (None, None, None, None) and h[never].param_norm > 0
        assert h[later][:3] == (None, None, None) and h[later].update_norm is not None
        for n in names:
            steps = {never: 0, later: 1}.get(n, 2)
            _check_param(h[n], *_expect(model, optim, n, steps, grad=n not in (never, later)), n)
    finally:
        config.reset()


def test_two_groups_use_their_own_learning_rates():
    try:
        model, loss, _ = _make()
        names = [n for n, _ in model.named_parameters()]
        w, b = [n for n in names if not n.endswith('.bias')], [n for n in names if n.endswith('.bias')]
        optim = FusedAdam(model, param_groups=[dict(params=w, lr=1e-3), dict(params=b, lr=2.5e-4, betas=(0.8, 0.99), eps=1e-6)])
        batch = _batch()
        _step(model, loss, optim, batch)
        _step(model, loss, optim, batch)
        st = optim.param_stats()
        h = st.host()
        table = st.table.cpu()
        for i, n in enumerate(names):
            lr = 2.5e-4 if n in b else 1e-3
            assert st.lrs[i] == lr and h[n].update_norm == lr * float(table[i, 6]) ** 0.5
            _check_param(h[n], *_expect(model, optim, n, 2), n)
    finally:
        config.reset()


def test_inside_an_accumulation_window():
    """accumulate_steps = 2: called inside the window (one micro-batch taken) and at its end (two, before the apply), grad_norm is
    that of the buffer -- the unscaled sum so far -- times grad_scale / 2"""
    try:
        model, loss, optim = _make(dropout=0.3)
        optim.accumulate_steps = 2
        optim.grad_scale = 0.25
        batch = _batch()
        names = [n for n, _ in model.named_parameters()]
        scale = ops.accum_scale(0.25, 2)
        assert scale == 0.125
        _step(model, loss, optim, batch)                     # a hold
        assert optim.accum_phase == 1 and optim._step == 0
        for when in ('inside', 'at the end'):
            st = optim.param_stats()
            assert st.scale == scale
            h = st.host()
            for n in names:
                _check_param(h[n], *_expect(model, optim, n, 0, scale=scale), n)
            if when == 'inside':
                first = {n: h[n].grad_norm for n in names}
                _backward(model, loss, optim, batch)         # the second micro-batch adds to the buffer
        assert any(h[n].grad_norm != first[n] for n in names)
        optim.step()
        assert optim.accum_phase == 0 and optim._step == 1
        h = optim.param_stats().host()
        for n in names:
            _check_param(h[n], *_expect(model, optim, n, 1, scale=scale), n)
    finally:
        config.reset()


def test_nan_attribution_after_a_skipped_step():
    try:
        model, loss, optim = _make()
        batch = _batch()
        optim.skip_nonfinite = True
        _step(model, loss, optim, batch)
        torch.cuda.synchronize()
        assert float(optim.found_nonfinite) == 0.0 and optim.nonfinite_params() == []
        before = tuple(t.clone() for t in (model.flat_params(), optim._m, optim._v))
        names = [n for n, _ in model.named_parameters()]
        culprit = names[5]
        _backward(model, loss, optim, batch)
        g = dict(model.named_parameters())[culprit].grad
        g.view(-1)[g.numel() // 2] = float('nan')
        optim.step()
        torch.cuda.synchronize()
        for a, b in zip(before, (model.flat_params(), optim._m, optim._v)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'the skipped step moved something'
        assert float(optim.found_nonfinite) == 1.0
        assert optim.nonfinite_params() == [culprit]
        h = optim.param_stats().host()
        assert h[culprit].grad_nonfinite == 1 and [n for n in names if h[n].grad_nonfinite] == [culprit]
        assert np.isfinite(h[culprit].grad_norm) and h[culprit].grad_norm > 0
        for n in names:                                      # (t = 1: the skipped step is no update)
            _check_param(h[n], *_expect(model, optim, n, 1), n)
        assert optim.skipped_total() == 1
    finally:
        config.reset()


def test_between_replays_of_a_recorded_step():
    """a RecordedTrainStep with the defaults (two warm-up steps, which also decide the overwrite mode; the deferred side join and the
    folded first-layer update where the step can take them) -- the recording is step 3 --, replayed three times; an eager run of the
    same six steps from the same seed on its own copy of the batch.  Parameter and update columns: the same bits; gradient columns:
    this run's own p.grad in float64; a seventh step on both afterwards still agrees bit for bit -- the call disturbed nothing."""
    from lirec_amd.graph import RecordedTrainStep
    try:
        batch1, batch = _batch(), _batch()
        m1, l1, o1 = _make(dropout=0.3)
        for _ in range(6):
            _step(m1, l1, o1, batch1)
        eager = o1.param_stats()
        m2, l2, o2 = _make(dropout=0.3)
        g = RecordedTrainStep(m2, l2, o2, batch)
        try:
            print('PSTAT-FIGURE recorded step: overwrite=%s fused=%s defer=%s' % (g.overwrite, g.fused, g.defer))
            for _ in range(3):
                g.step()
            rec = o2.param_stats()
            torch.cuda.synchronize()
            assert torch.equal(m1.flat_params().view(torch.int32), m2.flat_params().view(torch.int32)), 'eager and recorded runs differ'
            a, b = eager.table.cpu(), rec.table.cpu()
            assert torch.equal(a[:, 3:].contiguous().view(torch.int64), b[:, 3:].contiguous().view(torch.int64))
            assert rec.flags == eager.flags == [7] * len(rec.names)
            h = rec.host()
            for n in rec.names:
                _check_param(h[n], *_expect(m2, o2, n, 6), n)
            g.step()
            _step(m1, l1, o1, batch1)
            torch.cuda.synchronize()
            g.flush()
            assert torch.equal(m1.flat_params().view(torch.int32), m2.flat_params().view(torch.int32)), 'param_stats() disturbed the recorded step'
        finally:
            g.release()
    finally:
        config.reset()
