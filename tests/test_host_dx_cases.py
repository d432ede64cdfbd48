"""tests/dx_cases.py without a GPU: the float64 references are pinned to torch autograd of the plain definition (expand the tables
through the index into rows, Linear per segment, sum), the case tables are checked for what they promise, and the comparators
that tests/test_gpu_dx_pieces.py applies to the device's results are shown to reject what a wrong kernel would produce -- the
reference perturbed the way the kernel would be wrong, rounded to fp32, handed to the same comparator under both cores' bounds."""
import pytest
import torch

import dx_cases as DC
import pool_cases as PC
from test_gpu_layer1_persistent import RELU_EPS, RELU_FRAC

ALL_DX = DC.DX_CASES + [DC.DX_PLANES]
ids = lambda cs: [c.id for c in cs]


def same(a, b, what):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-12 * scale, (what, float((a - b).abs().max()), scale)


# ---------------------------------------------------------------------------------------------------------------------------
# the references against autograd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ALL_DX, ids=ids(ALL_DX))
def test_dx_reference_is_autograd(case):
    for operand in (('f32',) if case is not DC.DX_PLANES else ('hilo', 'hi')):
        inp = DC.dx_inputs(case, operand)
        X = torch.randn(case.n * case.rp1, case.D, dtype=torch.float64, generator=DC.gen(case.name, 1)).requires_grad_(True)
        loss = X.sum() * 0
        for hd in inp['heads']:
            h = hd['h']
            for s, (off, dim) in enumerate(h.segs):
                z = torch.nn.functional.linear(X[hd['prow'], off:off + dim], hd['W1'][s].double())
                loss = loss + (z * hd['dz'][:, s * h.J:(s + 1) * h.J].double()).sum()
        loss.backward()
        same(X.grad, inp['ref'], case.name)
        assert torch.equal(X.grad != 0, inp['written'] & (inp['ref'] != 0))
        if operand == 'hilo':
            hd = inp['heads'][1]
            assert torch.equal(hd['dz'], hd['hi'].float() + hd['lo'].float()) and bool((hd['lo'].float() != 0).any())


def scatter_add_loop(dz, ix, n_clip, n_track, J):
    nc1, nt1 = n_clip + 1, n_track + 1
    S = torch.zeros(nc1 + nt1, 2 * J, dtype=torch.float64)
    for r in range(dz.shape[0]):
        c, t1, t2 = (int(v) for v in ix[r])
        S[c if c >= 0 else n_clip, :2 * J] += dz[r, :2 * J].double()
        S[nc1 + (t1 if t1 >= 0 else n_track), :J] += dz[r, 2 * J:3 * J].double()
        S[nc1 + (t2 if t2 >= 0 else n_track), J:] += dz[r, 3 * J:].double()
    return S


@pytest.mark.parametrize('case', DC.DW1_CASES, ids=ids(DC.DW1_CASES))
def test_piece_references_are_autograd(case):
    """dW1 / db1 against d / d(W1, b1), and dxi_ref(S, W1) -- S the per-piece sums -- against d / d(tables)"""
    c = case
    inp = DC.dw1_inputs(c)
    J = c.J
    g = DC.gen(c.name, 2)
    clip = inp['clip'].double().requires_grad_(True)
    track = inp['track'].double().requires_grad_(True)
    flat = inp['index'].view(-1, 3)
    loss = clip.sum() * 0
    Ws, Ss, rows = [], [], []
    for hd in inp['heads']:
        W = [(torch.randn(J, d, generator=g, dtype=torch.float64) / d ** 0.5).requires_grad_(True) for d in c.dims]
        b = [torch.zeros(J, dtype=torch.float64, requires_grad=True) for _ in c.dims]
        Ws.append((W, b))
        if hd['empty']:
            Ss.append(torch.full(((c.n_clip + c.n_track + 2) * 2 * J,), DC.NAN))
            rows.append(0)
            continue
        ix = flat[hd['prow']].long()
        X = torch.cat([t[i.clamp_min(0)] * (i >= 0).double().unsqueeze(1) for t, i in ((clip, ix[:, 0]), (track, ix[:, 1]), (track, ix[:, 2]))], 1)
        for s, (off, dim) in enumerate(hd['h'].segs):
            z = torch.nn.functional.linear(X[:, off:off + dim], W[s], b[s])
            loss = loss + (z * hd['dz'][:, s * J:(s + 1) * J].double()).sum()
        Ss.append(hd['S'].reshape(-1))
        rows.append(hd['L'].numel())
        if hd['L'].numel() <= 400:
            same(hd['S'], scatter_add_loop(hd['dz'], ix, c.n_clip, c.n_track, J), c.name + ' S')
    loss.backward()
    for hd, (W, b) in zip(inp['heads'], Ws):
        if hd['empty']:
            continue
        for s in range(4):
            ini_w = 0.0 if c.overwrite else hd['g0W'][s].double()
            ini_b = 0.0 if c.overwrite else hd['g0b'][s].double()
            same(W[s].grad + ini_w, hd['dW'][s], '%s dW1[%d]' % (c.name, s))
            same(b[s].grad + ini_b, hd['db'][s], '%s db1[%d]' % (c.name, s))
    ic = DC.DxiCase(c.name, c.n_clip, c.n_track, c.td, c.vd, c.kd, J, tuple(rows))
    ref = DC.dxi_ref(ic, Ss, [[w.detach() for w in W] for W, _ in Ws])
    same(clip.grad, ref['dClip'], c.name + ' dClip')
    same(track.grad, ref['dTrack'], c.name + ' dTrack')
    assert not bool(clip.grad[-1].any()) and not bool(track.grad[-1].any())


@pytest.mark.parametrize('case', DC.L1_CASES, ids=ids(DC.L1_CASES))
def test_l1_reference_is_the_expanded_linear(case):
    inp = DC.l1_inputs(case)
    c, h = case, inp['h']
    flat = inp['index'].view(-1, 3)
    for r in range(0, inp['L'].numel(), 7):
        L = int(inp['L'][r])
        prow = (L // h.group) * c.rp1 + h.goff + L % h.group
        ci, t1, t2 = (int(v) for v in flat[prow])
        x = torch.cat([inp['clip'][ci] if ci >= 0 else torch.zeros(c.td + c.vd), inp['track'][t1] if t1 >= 0 else torch.zeros(c.kd),
                       inp['track'][t2] if t2 >= 0 else torch.zeros(c.kd)]).double()
        z = torch.cat([inp['W1'][s].double() @ x[o:o + d] + inp['b1'][s].double() for s, (o, d) in enumerate(h.segs)])
        same(inp['pre'][r], z, '%s row %d' % (c.name, r))


# ---------------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------------
def check_rows(h, n, rp1, hd):
    assert rp1 >= h.goff + h.group
    if h.mask is None:
        return
    mask, L, cstart = hd['mask'], hd['L'], hd['cstart']
    assert mask.shape == (n, h.R) and cstart.numel() == n + 1 and int(cstart[0]) == 0 and int(cstart[-1]) == L.numel()
    assert bool((L[1:] > L[:-1]).all()) and (L.numel() == 0 or (int(L[0]) >= 0 and int(L[-1]) < n * h.R))
    for cnd in range(n):
        own = L[int(cstart[cnd]):int(cstart[cnd + 1])]
        assert own.numel() == int((mask[cnd] != 0).sum()) and bool((own // h.R == cnd).all())
        assert bool((mask[cnd, own % h.R] != 0).all())


def test_dx_case_table():
    rows, widths, Js, dense_R, compact_R, gaps, kinds = set(), set(), set(), set(), set(), [], set()
    pats = set()
    for case in ALL_DX:
        inp = DC.dx_inputs(case, 'hilo' if case is DC.DX_PLANES else 'f32')
        assert case.D % 4 == 0 and 1 <= case.rp1 <= 1024 and 1 <= len(case.heads) <= 2
        owned = torch.zeros(case.rp1, dtype=torch.int32)
        for hd in inp['heads']:
            h = hd['h']
            check_rows(h, case.n, case.rp1, hd)
            owned[h.goff:h.goff + h.group] += 1
            rows.add(case.n * h.group); Js.add(h.J)
            assert h.J % 4 == 0 and 1 <= h.nseg <= 4 and (h.J % 32 == 0 or h.nseg >= 2)
            at = 0
            for off, dim in h.segs:
                assert off >= at and dim % 4 == 0 and dim >= 4 and off + dim <= case.D
                at = off + dim
                widths.add(dim)
            if h.kind == 'pooled':
                (dense_R if h.mask is None else compact_R).add(h.R)
                if h.mask is not None:
                    m = hd['mask']
                    if not bool(m.any()):
                        pats.add('all-masked batch')
                    for cnd in range(case.n):
                        v = m[cnd] != 0
                        k = int(v.sum())
                        pats.add('none' if k == 0 else ('all' if k == h.R else ('first' if k == 1 and bool(v[0]) else
                                                                                 ('last' if k == 1 and bool(v[-1]) else 'some'))))
                    if case.rp1 > 1 + h.R:
                        kinds.add('rows no head owns behind the pooled rows')
            if h.segs in (DC.GAPS_A, DC.GAPS_B):
                gaps += DC.head_gaps(h, case.D)
        assert int(owned.max()) <= 1, case.name + ': two heads own a row'
        kinds.add('both' if len(case.heads) == 2 else case.heads[0].kind + ' alone')
        if case.rp1 == 1:
            kinds.add('rp1 = 1')
    assert rows >= {1, 127, 128, 129, 300} and widths >= {4, 132, 256} and Js >= {4, 36, 100, 256}
    assert dense_R >= {1, 3, 18} and compact_R >= {1, 3, 18}
    assert kinds >= {'both', 'plain alone', 'pooled alone', 'rp1 = 1', 'rows no head owns behind the pooled rows'}
    assert pats >= {'none', 'first', 'last', 'all', 'some', 'all-masked batch'}
    assert {w for _, w in gaps} >= {1, 2, 3, 5, 8} and {s % 4 for s, _ in gaps} == {0, 1, 2, 3}
    assert any(s % 4 and w >= 8 for s, w in gaps)               # (a misaligned start in front of whole float4 groups)
    both = [c for c in DC.DX_CASES if c.heads[0].segs == DC.GAPS_A and len(c.heads) == 2]
    assert both and both[0].D > max(o + d for o, d in DC.GAPS_A + DC.GAPS_B)
    pl = DC.DX_PLANES
    assert all(h.J == 256 and h.planes and all(d % 256 == 0 for _, d in h.segs) for h in pl.heads) and pl.heads[1].R <= 64


def check_index(index, prows, n_clip, n_track, name):
    for k, npiece in ((0, n_clip), (1, n_track), (2, n_track)):
        assert int(index[..., k].min()) >= -1 and int(index[..., k].max()) < npiece, name
    used = index.view(-1, 3)[prows]
    if used.numel() == 0:
        return
    assert bool((used < 0).any()), name + ': no negative entry among the computed rows'
    assert bool((used[:, 1] == 0).all()), name + ': track piece 0 is not used by every row'
    if n_clip >= 3:
        assert not bool((index[..., 0] == n_clip - 1).any()), name
    if n_track >= 3:
        assert not bool((index[..., 1:] == n_track - 1).any()), name


def test_indexed_case_tables():
    for c in DC.DXI_CASES:
        assert c.td % 4 == 0 and c.vd % 4 == 0 and c.kd % 4 == 0 and c.J % 4 == 0 and 1 <= len(c.rows) <= 2
        inp = DC.dxi_inputs(c)
        nc1 = c.n_clip + 1
        for r, s in zip(c.rows, inp['S']):
            if r:
                sc = s[:nc1 * 2 * c.J].view(nc1, 2 * c.J)
                assert bool((sc[-1] != 0).all()) and bool((s[nc1 * 2 * c.J:].view(-1, 2 * c.J)[-1] != 0).all())   # trailing rows non-zero
            else:
                assert bool(torch.isnan(s).all())
    assert {c.n_clip for c in DC.DXI_CASES} >= {1, 127, 128, 129} and {c.n_track for c in DC.DXI_CASES} >= {1, 127, 128, 129}
    for f in ('td', 'vd', 'kd'):
        assert {getattr(c, f) for c in DC.DXI_CASES} >= {4, 132, 256}
    assert {c.J for c in DC.DXI_CASES} >= {4, 36, 256}
    assert {tuple(bool(r) for r in c.rows) for c in DC.DXI_CASES} >= {(True,), (True, True), (False, True), (False, False)}

    unused = False
    for c in DC.DW1_CASES:
        inp = DC.dw1_inputs(c)
        assert c.J % 4 == 0 and all(h.J == c.J for h in c.heads)
        owned = torch.zeros(c.rp1, dtype=torch.int32)
        for hd in inp['heads']:
            if hd['empty']:
                continue
            h = hd['h']
            owned[h.goff:h.goff + h.group] += 1
            check_rows(h, c.n, c.rp1, hd)
            check_index(inp['index'], hd['prow'], c.n_clip, c.n_track, c.name)
            if h.mask is not None:
                assert hd['L'].numel() < c.n * h.R                    # count < rows
        assert int(owned.max()) <= 1
        unused |= c.n_clip >= 3 and c.n_track >= 3
        assert not bool(inp['clip'][-1].any()) and not bool(inp['track'][-1].any())
    assert unused
    assert any((c.n_clip + 2 * c.n_track + 3) % 4 != 0 for c in DC.DW1_CASES)
    assert any(c.n * c.heads[0].group > DC.ONEHOT_STRIDE_ROWS for c in DC.DW1_CASES)
    assert {c.overwrite for c in DC.DW1_CASES} == {True, False}
    assert any(h.empty for c in DC.DW1_CASES for h in c.heads) and any(h.mask for c in DC.DW1_CASES for h in c.heads)
    assert any(h.mask == 'zero' for c in DC.DW1_CASES for h in c.heads)

    runs, seen = set(), set()
    for c in DC.L1_CASES:
        inp = DC.l1_inputs(c)
        h = inp['h']
        assert h.J % 256 == 0
        check_rows(h, c.n, c.rp1, inp)
        check_index(inp['index'], inp['prow'], c.n_clip, c.n_track, c.name)
        cnt = inp['L'].numel()
        if h.mask is not None:
            assert 0 < cnt < c.n * h.R
            runs |= set(DC.philox_units(inp['L'].tolist()))
        seen.add(('compact' if h.mask else 'plain', c.p > 0))
        seen.add(('stride', 'compact' if h.mask else 'plain') if cnt > DC.GATHER_STRIDE_ROWS else None)
        seen.add('rows % 4' if cnt % 4 else None)
        seen.add('n_clip = 1' if c.n_clip == 1 else None)
    assert runs >= DC.STRADDLE_RUNS
    assert DC.philox_units(DC.STRADDLE_IDS)[0] == (1, 2, 1) and DC.STRADDLE_IDS[:4] == (3, 4, 5, 9)
    assert seen >= {('compact', True), ('compact', False), ('plain', True), ('plain', False), ('stride', 'compact'), ('stride', 'plain'),
                    'rows % 4', 'n_clip = 1'}
    assert {d for c in DC.L1_CASES for d in c.dims} >= {4, 132}


@pytest.mark.parametrize('case', DC.L1_CASES, ids=ids(DC.L1_CASES))
def test_relu_cap_is_met_by_the_reference_alone(case):
    """were EVERY pre-activation within RELU_EPS of 0 decided otherwise on the device, the case would still be inside the cap"""
    inp = DC.l1_inputs(case)
    assert DC.near_zero(inp, RELU_EPS) <= 8 + RELU_FRAC * inp['pre'].numel()
    assert DC.near_zero(inp, RELU_EPS) <= 8
    assert not bool((inp['pre'] == 0).any())


# ---------------------------------------------------------------------------------------------------------------------------
# the comparators reject a wrong kernel
# ---------------------------------------------------------------------------------------------------------------------------
MODES = [0, 2]


def rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


def dx_got(inp, alter=None):
    """the device block a kernel would leave: the reference rounded to fp32 over a NaN pre-fill, zeros where nothing is written"""
    case = inp['case']
    got = torch.zeros(case.n * case.rp1, case.D)
    for hi_, s, prow, off, dim, K in inp['blocks']:
        hd = inp['heads'][hi_]
        a, w = hd['dz'][:, s * K:(s + 1) * K].double(), hd['W1'][s].double()
        blk = a @ w
        if alter == 'drop last k-tile':
            k1 = (K - 1) // 32 * 32
            blk = a[:, :k1] @ w[:k1]
        o = off + 1 if alter == 'c_off + 1' and off + 1 + dim <= case.D else off
        got[prow, o:o + dim] = blk.float()
    return got


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ALL_DX, ids=ids(ALL_DX))
def test_dx_comparator(case, mode):
    inp = DC.dx_inputs(case, 'hilo' if case is DC.DX_PLANES else 'f32')
    good = dx_got(inp)
    DC.check_dx(good, inp, mode, case.name)
    DC.check_dx_bf16(good.to(torch.bfloat16), good, case.name)
    if not any(hd['L'].numel() for hd in inp['heads']):
        bad = good.clone()
        bad[0, 0] = -0.0
        rejects(DC.check_dx, bad, inp, mode, case.name)          # (-0.0 is not an exact zero)
        return
    rejects(DC.check_dx, dx_got(inp, 'drop last k-tile'), inp, mode, case.name)
    rejects(DC.check_dx, dx_got(inp, 'c_off + 1'), inp, mode, case.name)
    # a surplus row of a partial tile stored: one element of a row no problem computes
    free = (~inp['written']).nonzero()
    if free.numel():
        bad = good.clone()
        bad[free[-1, 0], free[-1, 1]] = 1e-30
        rejects(DC.check_dx, bad, inp, mode, case.name)
    # an element never written
    hit = inp['written'].nonzero()[0]
    bad = good.clone()
    bad[hit[0], hit[1]] = DC.NAN
    rejects(DC.check_dx, bad, inp, mode, case.name)
    # the bf16 leaf truncated instead of rounded to nearest even
    trunc = (good.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    rejects(DC.check_dx_bf16, trunc, good, case.name)


@pytest.mark.parametrize('mode', MODES)
def test_dx_comparator_rejects_each_omitted_gap(mode):
    n_gaps = 0
    for case in DC.DX_CASES:
        inp = DC.dx_inputs(case)
        good = dx_got(inp)
        for hd in inp['heads']:
            if hd['h'].segs not in (DC.GAPS_A, DC.GAPS_B) or not hd['L'].numel():
                continue
            for start, width in DC.head_gaps(hd['h'], case.D):
                for col in range(start, start + width):                # (each column of the gap alone: a slip of dx_zero_span)
                    bad = good.clone()
                    bad[hd['prow'][-1], col] = DC.NAN
                    rejects(DC.check_dx, bad, inp, mode, case.name)
                n_gaps += 1
    assert n_gaps >= 15


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', DC.DXI_CASES, ids=ids(DC.DXI_CASES))
def test_dxi_comparator(case, mode):
    inp = DC.dxi_inputs(case)
    DC.check_dxi(inp['dClip'].float(), inp['dTrack'].float(), inp, mode, case.name)
    if inp['active'] == 0:
        bad = inp['dClip'].float()
        bad[3, 1] = -0.0
        rejects(DC.check_dxi, bad, inp['dTrack'].float(), inp, mode, case.name)
        return
    wrong = DC.dxi_ref(case, inp['S'], inp['W1'], trailing_is_piece=True)      # the trailing S row treated as a piece
    rejects(DC.check_dxi, wrong['dClip'].float(), inp['dTrack'].float(), inp, mode, case.name)
    rejects(DC.check_dxi, inp['dClip'].float(), wrong['dTrack'].float(), inp, mode, case.name)
    # the last chunk's last k-tile dropped
    k1 = (case.J - 1) // 32 * 32
    last = max(i for i, r in enumerate(case.rows) if r)
    S = [s.clone() for s in inp['S']]
    nc1 = case.n_clip + 1
    S[last][nc1 * 2 * case.J:].view(-1, 2 * case.J)[:, case.J + k1:] = 0
    S[last][:nc1 * 2 * case.J].view(-1, 2 * case.J)[:, k1:case.J] = 0
    wrong = DC.dxi_ref(case, S, inp['W1'])
    rejects(DC.check_dxi, wrong['dClip'].float(), inp['dTrack'].float(), inp, mode, case.name)
    rejects(DC.check_dxi, inp['dClip'].float(), wrong['dTrack'].float(), inp, mode, case.name)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', [c for c in DC.DW1_CASES if c.n < 1000], ids=ids([c for c in DC.DW1_CASES if c.n < 1000]))
def test_dw1_comparator(case, mode):
    c = case
    inp = DC.dw1_inputs(c)
    for hd in inp['heads']:
        if hd['empty']:
            continue
        S, dW, db = hd['S'].float().reshape(-1), [w.float() for w in hd['dW']], [b.float() for b in hd['db']]
        DC.check_dw1(S, dW, db, hd, c, mode, c.name)
        if hd['L'].numel() == 0:
            rejects(DC.check_dw1, S + 1e-30, dW, db, hd, c, mode, c.name)    # (count = 0: anything but zeros)
            continue
        # the null column's sums folded into piece 0 / a row of the index dropped
        bad = hd['S'].clone()
        bad[0] += bad[c.n_clip]
        bad[c.n_clip] = 0
        rejects(DC.check_dw1, bad.float().reshape(-1), dW, db, hd, c, mode, c.name)
        part = DC.s_ref(hd['dz'][:-1], hd['ix'][:-1], c.n_clip, c.n_track, c.J)[0]
        rejects(DC.check_dw1, part.float().reshape(-1), dW, db, hd, c, mode, c.name)
        # db1 without the rows of a negative index
        neg = hd['ix'][:, 0] < 0
        wrong = [b.clone() for b in hd['db']]
        wrong[0] -= hd['dz'][neg][:, :c.J].double().sum(0)
        rejects(DC.check_dw1, S, dW, [b.float() for b in wrong], hd, c, mode, c.name)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', DC.L1_CASES, ids=ids(DC.L1_CASES))
def test_h1_comparator(case, mode):
    inp = DC.l1_inputs(case)
    h, cnt = inp['h'], inp['L'].numel()
    rows = case.n * h.group
    keep = (torch.rand(rows, 4 * h.J, generator=DC.gen(case.name, 3)) >= case.p).to(torch.uint8)
    good = DC.h1_ref(inp, keep[inp['L']]).float()
    assert DC.check_h1(good, inp, keep[inp['L']], mode, case.name, RELU_EPS, RELU_FRAC) == 0
    if case.p > 0 and h.mask is not None:
        # the compact row number r instead of rowmap[r] as the dropout counter
        wrong = DC.h1_ref(inp, keep[:cnt]).float()
        rejects(DC.check_h1, wrong, inp, keep[inp['L']], mode, case.name, RELU_EPS, RELU_FRAC)
    if h.mask is not None:
        # the Philox block of the unit's first row kept for all four rows
        Lb = inp['L'].clone()
        for i in range(0, cnt, 4):
            Lb[i:i + 4] = (Lb[i] >> 2 << 2) + (Lb[i:i + 4] & 3)
        if case.p > 0 and not torch.equal(Lb, inp['L']):
            rejects(DC.check_h1, DC.h1_ref(inp, keep[Lb]).float(), inp, keep[inp['L']], mode, case.name, RELU_EPS, RELU_FRAC)
    # the bias left out where the index is negative
    neg = inp['ix'][:, 0] < 0
    pre = inp['pre'].clone()
    pre[neg, :h.J] -= inp['b1'][0].double()
    wrong = (torch.relu(pre) * keep[inp['L']].double() * PC.drop_scale(case.p)).float()
    rejects(DC.check_h1, wrong, inp, keep[inp['L']], mode, case.name, RELU_EPS, RELU_FRAC)
