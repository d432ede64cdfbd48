"""The proof that the criteria of tests/gemm_cases.py mean something, on the CPU: for every case and arithmetic model
  * the model is where it claims to be -- 'f32' and 'one' exact on their operands, 'x3' within 2^-16 S of the plain float64 product;
  * the fp32 yardstick meets the hard bound, and stays under its own cap with margin to spare (8 e_yardstick <= (K + 8) u wherever
    K >= 64): a device result as good as the CPU's passes both criteria;
  * every injected defect (gemm_cases.DEFECTS) that applies to a case exceeds 8 e_yardstick there, and the hard bound too on the
    cases with K <= 256 -- each test prints the cases its defect was injected in and caught on, and fails if there is none;
  * the restated split plan gives the chunk lengths the launcher's rule promises, the grouped cases take the tile orders they were
    made for, and the epilogue models agree with torch autograd of the plain definitions in float64.
Nothing here needs a GPU."""
import pytest
import torch

import gemm_cases as GC
from oracle import lirec_oracle as O

U = GC.U
ARITHS = ['f32', 'x3']
SHAPES = GC.TRIPLES + GC.SPLIT


def linear_roles(n, K, N, arith):
    """[(id, Prod, finish keywords)] of the three GEMMs of a triple, each with the epilogue its call site has"""
    d, pr = GC.linear_data(n, K, N), GC.linear_prods(n, K, N, arith)
    out = [('Y', pr['Y'], dict(bias=d['b'])), ('dW', pr['dW'], dict(prev=d['dW0'])), ('dA', pr['dA'], dict())]
    out.append(('dA-tanh', pr['dA'], dict(prev=d['dA0'], factor=GC.da_factor(d, 2, 0.3))))
    out.append(('dA-relu', pr['dA'], dict(factor=GC.da_factor(d, 1, 0.3))))
    return [('%s-%s-(%d,%d,%d)' % (arith, what, n, K, N), p, kw) for what, p, kw in out]


def gate_roles(n, K, N, split, arith):
    d, pr = GC.gate_data(n, K, N), GC.gate_prods(n, K, N, arith)
    keep_g = GC.keep_mask(GC.DROP_SEED, O.SITE_GATE, n, N, 0.3) * GC.drop_scale(0.3)
    out = [('G', pr['G'], dict(bias=d['bg'], relu=True, factor=keep_g)), ('dWg', pr['dWg'], dict(prev=d['dW0'])),
           ('dEE', pr['dEE'], dict())]
    return [('%s-gate-%s-(%d,%d,%d)' % (arith, what, n, K, N), p, kw) for what, p, kw in out]


def all_roles():
    for arith in ARITHS:
        for t in SHAPES:
            yield from linear_roles(*t, arith)
    for n, K, N, split in GC.GATE_PLAIN + GC.GATE_WS_P2 + GC.GATE_WS_P3[:1]:
        for arith in ('x3', 'one') if (n, K, N, split) in GC.GATE_WS_P3 + GC.GATE_WS_P2 else ('f32', 'x3', 'one'):
            yield from gate_roles(n, K, N, split, arith)


ROLES = list(all_roles())


def bf16_representable(x):
    return not bool((x.float().contiguous().view(torch.int32) & 0xffff).any())


def test_models_are_where_they_claim_to_be():
    for cid, p, _ in ROLES:
        if p.arith == 'f32':
            assert torch.equal(p.model, p.plain), cid
        elif p.arith == 'one':
            a, b = GC.bf16_rne(p.A), GC.bf16_rne(p.B)
            assert bf16_representable(a) and bf16_representable(b)
            assert float((a - p.A).abs().max()) <= 2.0 ** -8 * float(p.A.abs().max())
            assert torch.equal(p.model, a.double() @ b.double()), cid
        else:
            for x in (p.A, p.B):
                hi, lo = GC.split_hi_lo(x)
                assert bf16_representable(hi) and bf16_representable(lo)
                # half a bf16 ulp of hi, then half a bf16 ulp of lo: 2^-17 of the element
                assert bool(((x.double() - hi.double() - lo.double()).abs() <= 2.0 ** -17 * x.double().abs()).all()), cid
            assert bool(((p.model - p.plain).abs() <= 2.0 ** -16 * p.S).all()), cid


def test_yardstick_meets_the_hard_bound_with_margin_to_spare():
    worst = 0.0
    for cid, p, kw in ROLES:
        ref = GC.finish(p, **kw)
        n_hard, e, cap, e_y = GC.violations(ref.yard, ref)
        assert n_hard == 0, (cid, n_hard)
        assert e == e_y and e <= cap
        if p.K >= 64:
            assert GC.MARGIN * e_y <= (p.K + 8) * U, (cid, e_y / U, p.K)
            worst = max(worst, GC.MARGIN * e_y / ((p.K + 8) * U))
    for t in SHAPES:
        d = GC.linear_data(*t)
        for values in ('f32', 'x3', 'one'):
            ref = GC.colsum_ref(d['dY'], d['db0'], values)
            assert GC.violations(ref.yard, ref)[0] == 0, (t, values)
    print('largest 8 e_yardstick / ((K + 8) u) at K >= 64: %.3f' % worst)


def caught(ref, x, K):
    """is the defective output x rejected by the yardstick criterion -- and, K <= 256, by the hard bound?"""
    n_hard, e, cap, e_y = GC.violations(x, ref)
    dead_ok = GC.rel_error(x, ref)[1]
    by_yard = e > cap or not dead_ok
    return by_yard and (n_hard > 0 or K > 256), e, cap


@pytest.mark.parametrize('name', sorted(GC.PRODUCT_DEFECTS))
def test_product_defect_is_caught(name):
    hit = []
    for cid, p, kw in ROLES:
        wrong = GC.PRODUCT_DEFECTS[name](p)
        if wrong is None:
            continue
        ref = GC.finish(p, **kw)
        if kw.get('factor') is not None and name.startswith('neighbour'):
            # (a row / column that the factor zeroes entirely shows no defect: look at it before the factor)
            ref = GC.finish(p, **{k: v for k, v in kw.items() if k != 'factor'})
            kw = {k: v for k, v in kw.items() if k != 'factor'}
        if not bool((ref.D > 0).any()):
            continue                                                # (the one element of (1, 1, 1) is dropped: nothing to see)
        ok, e, cap = caught(ref, GC.finish(p, product=wrong, **kw).model, p.K)
        assert ok, '%s not caught on %s: e %.3e, cap %.3e' % (name, cid, e, cap)
        hit.append(cid)
    print('%s: injected and caught on %d cases: %s' % (name, len(hit), ' '.join(hit)))
    assert hit


def test_wrong_dropout_site_is_caught():
    hit = []
    for arith in ARITHS:
        for n, K, N in GC.TRIPLES:
            if n * K < 8:
                continue                                            # (too few elements for two masks to differ for sure)
            d, pr = GC.linear_data(n, K, N), GC.linear_prods(n, K, N, arith)
            ref = GC.da_ref(n, K, N, arith, 2, 1, 0.3)
            wrong = GC.da_ref(n, K, N, arith, 2, 1, 0.3, site=O.SITE_E_INTS)
            ok, e, cap = caught(ref, wrong.model, pr['dA'].K)
            assert ok, (arith, n, K, N, e, cap)
            hit.append('%s-dA-tanh-(%d,%d,%d)' % (arith, n, K, N))
    for n, K, N, split in GC.GATE_PLAIN:
        if split in (0, K):
            continue
        ref = GC.gate_refs(n, K, N, split, 'x3', 0.3, 1)
        wrong = GC.gate_refs(n, K, N, split, 'x3', 0.3, 1, sites=(O.SITE_E_CTX, O.SITE_E_INTS, O.SITE_E_CTX))
        for what in ('G', 'dEE'):
            ok, e, cap = caught(ref[what], wrong[what].model, ref[what].K)
            assert ok, (what, n, K, N, e, cap)
            hit.append('x3-gate-%s-(%d,%d,%d)' % (what, n, K, N))
    print('wrong_dropout_site: injected and caught on %d cases: %s' % (len(hit), ' '.join(hit)))


def test_beta_applied_is_caught():
    hit = []
    for arith in ARITHS:
        for n, K, N in SHAPES:
            d, pr = GC.linear_data(n, K, N), GC.linear_prods(n, K, N, arith)
            for what, prev, prod in (('dW', d['dW0'], pr['dW']), ('dA', d['dA0'], pr['dA'])):
                ref = GC.finish(prod)
                ok, e, cap = caught(ref, GC.finish(prod, prev=prev).model, prod.K)
                assert ok, (arith, what, n, K, N, e, cap)
                hit.append('%s-%s-(%d,%d,%d)' % (arith, what, n, K, N))
            ref = GC.colsum_ref(d['dY'])
            assert caught(ref, GC.colsum_ref(d['dY'], d['db0']).model, n)[0], ('db', n, K, N)
    print('beta_applied: injected and caught on %d cases: %s' % (len(hit), ' '.join(hit)))


def split_launches():
    """[(id, Prod, finish keywords, ksplit, kchunk)] of the split triples' launches that split at configuration 0"""
    for arith, mode in (('f32', 0), ('x3', 2)):
        for n, K, N in GC.SPLIT:
            d, pr = GC.linear_data(n, K, N), GC.linear_prods(n, K, N, arith)
            probs = GC.linear_problems(n, K, N)
            for what, layout, kw in (('Y', GC.L_NT, dict(bias=d['b'])), ('dW', GC.L_TN, dict(prev=d['dW0'])), ('dA', GC.L_NN, dict())):
                _, plans, _ = GC.plan_launch(layout, mode, 0, [probs[layout]], GC.SPLIT_SCRATCH_FLOATS)
                if plans[0][0] > 1:
                    yield '%s-%s-(%d,%d,%d)' % (arith, what, n, K, N), pr[what], kw, plans[0][0], plans[0][1]


def test_split_chunk_left_out_is_caught():
    hit = []
    for cid, p, kw, ks, kchunk in split_launches():
        ref = GC.finish(p, **kw)
        for which in (0, ks - 1):
            wrong = GC.defect_skip_chunk(p, kchunk, which)
            assert wrong is not None
            ok, e, cap = caught(ref, GC.finish(p, product=wrong, **kw).model, p.K)
            assert ok, (cid, which, e, cap)
        hit.append('%s[%dx%d]' % (cid, ks, kchunk))
    print('split_chunk_left_out: injected and caught on %d cases: %s' % (len(hit), ' '.join(hit)))
    assert len(hit) >= 6


def test_split_plan_reproduces_the_promised_chunks():
    assert GC.clamp_split(1000, 86) == (3, 352) and GC.chunk_lengths(1000, 3, 352) == [352, 352, 296]
    assert GC.clamp_split(520, 100) == (2, 288) and GC.chunk_lengths(520, 2, 288) == [288, 232]
    assert GC.clamp_split(511, 9) == (1, 512) and GC.clamp_split(100000, 99)[0] == 32
    scratch = GC.SPLIT_SCRATCH_FLOATS
    # (1000, 520, 12): the weight gradient reduces over 1000 rows in three chunks, the forward over 520 in two, at EVERY configuration
    for mode, cfg in GC.SPLIT_FORMS:
        pr = GC.linear_problems(1000, 520, 12)
        _, plans, ext = GC.plan_launch(GC.L_TN, mode, cfg, [pr[GC.L_TN]], scratch)
        assert plans == [(3, 352)] and ext == 3 * (12 * 520 + 12), (mode, cfg, plans)
        assert GC.plan_launch(GC.L_NT, mode, cfg, [pr[GC.L_NT]], scratch)[1] == [(2, 288)], (mode, cfg)
        assert GC.plan_launch(GC.L_NN, mode, cfg, [pr[GC.L_NN]], scratch)[1][0][0] == 1        # K = 12
        for t in GC.SPLIT[1:]:
            pr = GC.linear_problems(*t)
            for layout in (GC.L_NT, GC.L_TN, GC.L_NN):
                ks, kchunk = GC.plan_launch(layout, mode, cfg, [pr[layout]], scratch)[1][0]
                assert (ks > 1) == (pr[layout].K >= 512), (mode, cfg, t, layout, ks)
                lens = GC.chunk_lengths(pr[layout].K, ks, kchunk)
                assert sum(lens) == pr[layout].K and all(v > 0 for v in lens) and (ks == 1 or lens[-1] % 32 != 0), (t, layout, lens)
        # without a scratch, and with an epilogue, nothing splits
        assert GC.plan_launch(GC.L_TN, mode, cfg, [GC.linear_problems(1000, 520, 12)[GC.L_TN]], 0)[1][0][0] == 1
        assert GC.plan_launch(GC.L_NN, mode, cfg, [GC.Problem(520, 12, 1000, store=False)], scratch)[1][0][0] == 1


def test_no_tile_form_runs_the_cases_by_accident():
    """the configurations the launcher picks by itself at the cases' shapes (force_cfg = -1), and what the forced ones map to"""
    for t in GC.TRIPLES:
        for layout, p in GC.linear_problems(*t).items():
            assert GC.tile_cfg(layout, 2, -1, [p], 0)[0] == 0 and GC.tile_cfg(layout, 0, -1, [p], 0)[0] == 0
            for force in range(5):
                want = 3 if (force == 2 and layout != GC.L_TN) else force
                assert GC.tile_cfg(layout, 2, force, [p], 0)[0] == want
                assert GC.tile_cfg(layout, 0, force, [p], 0)[0] == (0 if force == 0 else 1)


def test_grouped_cases_take_the_tile_orders_they_were_made_for():
    fwd = lambda ts: [GC.linear_problems(*t)[GC.L_NT] for t in ts if t[0] > 0]
    assert GC.group_order(fwd(GC.GROUPS['pgroup']), 64, 64) == ('same', 18, 16)              # 18 row panels: one group of 16, one of 2
    assert GC.tile_cfg(GC.L_NT, 2, -1, fwd(GC.GROUPS['pgroup']), 0)[0] == 0
    kind, tier_rows, pgroup = GC.group_order(fwd(GC.GROUPS['two_tier']), 64, 64)
    assert (kind, tier_rows) == ('two', 1)
    assert len(fwd(GC.GROUPS['empty_member'])) == 3
    assert GC.group_order(fwd(GC.GROUPS['mixed_epilogues']), 64, 64)[0] == 'same'


def test_epilogue_models_agree_with_autograd():
    """relu(dropout) and tanh(dropout) layers feeding a linear layer, in float64 with torch autograd, against finish()"""
    n, K, N, p = 33, 31, 65, 0.3
    d, pr = GC.linear_data(n, K, N), GC.linear_prods(n, K, N, 'f32')
    W, b, dY = d['W'].double(), d['b'].double(), d['dY'].double()
    scale = GC.drop_scale(p)
    keep = GC.keep_mask(GC.DROP_SEED, O.SITE_E_CTX, n, K, p)
    assert 0.5 < float(keep.mean()) < 0.9
    close = lambda a, b_: bool(((a - b_).abs() <= 1e-12 * (1 + b_.abs())).all())
    for kind in ('store', 'relu', 'tanh'):
        pre = d['act'].double().clone().requires_grad_(True)
        Wp, bp = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        if kind == 'relu':
            h = torch.relu(pre) * keep * scale
        elif kind == 'tanh':
            h = torch.tanh(pre) * keep * scale
        else:
            h = pre
        Y = h @ Wp.t() + bp
        ((Y * dY).sum() + (h * d['dA0'].double()).sum()).backward()
        A32 = h.detach().float()                                  # the layer's input as the library sees it
        assert close(GC.finish(GC.Prod(A32, d['W'].t(), 'f32'), bias=d['b']).model, A32.double() @ W.t() + b)
        assert close(GC.finish(GC.Prod(d['dY'].t(), A32, 'f32')).model, dY.t() @ A32.double())
        assert close(GC.colsum_ref(d['dY']).model, bp.grad)
        if kind == 'relu':                                          # the library reads the decisions off the layer's OUTPUT
            fac = GC.relu_bwd_factor(h.detach(), p)
        elif kind == 'tanh':
            fac = GC.tanh_bwd_factor(torch.tanh(d['act']), keep, p)
        else:
            fac = None
        got = GC.finish(pr['dA'], prev=d['dA0'], factor=fac).model
        want = pre.grad
        if kind == 'tanh':                                          # (the model squares the fp32 tanh the library is handed)
            assert bool(((got - want).abs() <= 1e-6 * (1 + want.abs())).all())
        else:
            assert close(got, want), kind
    # the gate's forward: relu, then dropout
    g = GC.gate_refs(33, 64, 65, 31, 'f32', p, 0)['G'].model
    gd = GC.gate_data(33, 64, 65)
    z = gd['EE'].double() @ gd['Wg'].double().t() + gd['bg'].double()
    assert close(g, torch.relu(z) * GC.keep_mask(GC.DROP_SEED, O.SITE_GATE, 33, 65, p) * scale)


@pytest.mark.parametrize('placement', GC.PLACEMENTS)
def test_placement_guards(placement):
    data = torch.arange(15, dtype=torch.float32).view(3, 5)
    pl = GC.Placed(3, 5, placement, 'cpu', data=data)
    assert torch.equal(pl.get(), data) and pl.guards_intact()
    assert pl.ld == {'dense': 5, 'ld4': 9, 'ld1': 6, 'off1': 5}[placement]
    assert (pl.ptr % 16 == 4) == (placement == 'off1') and (placement == 'off1' or pl.ptr % 16 == 0)
    pl.poison()
    assert pl.guards_intact() and bool(torch.isnan(pl.get()).all())
    pl.buf[pl.start - 1] = 0.0
    assert not pl.guards_intact()
    pl.buf[pl.start - 1] = GC.SENTINEL
    pl.buf[pl.start + 3 * pl.ld] = 1.0                             # the first element of the guard row behind
    assert not pl.guards_intact()
    flat = GC.Placed(1, 7, placement, 'cpu', strided=False)
    assert flat.ld == 7 and GC.Placed(0, 5, placement, 'cpu').guards_intact()
