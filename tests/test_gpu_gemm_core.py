"""The on-the-fly tiled GEMM core (launch_layout_ in lirec_amd/csrc/lirec_hip.hip; gemm.hpp, gemm_bf16x3.hpp, the split-K reduce) and
the gate tiers built on it, against the float64 models of tests/gemm_cases.py at tile edges, in every tile configuration, with and
without split-K, with every operand placed densely, inside a wider buffer and off alignment, and with guard values around everything.

Every test runs inside its own ``ops.Context()``: the GEMM mode, the forced tile configuration and the split-K scratch are the
context's own, a new context has no scratch, and the default context is left as it was found -- nothing depends on test order.
A registered scratch is filled with NaN first, so the planned split factor can be read off it afterwards.

Two criteria per output tensor (gemm_cases.py), both against the model, never against another device result: the derived hard
bound (K + 8) u D + 8 u |model| on every element, and e(device) <= 8 max(e(yardstick), u) with the fp32 yardstick computed on the CPU.
e_dev, e_yardstick and their ratio go to the achieved-error log per comparison (golden_util._record).  Operands and outputs sit in
sentinel-filled buffers (pad columns, a guard row before and after): every sentinel must survive the call.  Outputs that a call
overwrites are handed over full of NaN.

A. Tile forms: gemm mode x force_cfg over the ragged and vector-friendly (n, K, N) triples, four placements each, through
   lirec_linear_fwd, lirec_linear_bwd (dW, db, dA with epilogues 0 / 1 / 2, accumulate 0 / 1, p 0 / 0.3) and the grouped entry
   points.  Mode 2 and mode 3 run force_cfg -1, 0 .. 4, mode 0 -1, 0, 1 (the f32 core has two tiles), mode 1 the naive kernels.
   Configuration 2 (256 x 256) exists for the weight gradient only: forward and data gradient run configuration 3 in its place, so
   `cfg2` adds one tile form (TN), not three.  Mode 3 must equal the MODE 2 model here: the heads are no single-pass sites.
B. Split-K: the split triples with a registered scratch, per configuration -- criteria, the planned extent of the scratch written
   and not a float more, a second run bit-identical, and the same case without a scratch.
C. Poisoned outputs under lirec_set_grad_overwrite: dW, db (and dA without accumulate, and Y) start as NaN, split and unsplit.
D. Grouped launches made to take the row-panel-major order with panel groups (ragged last group), the two-tier order, a member
   without rows, and three epilogues in one NN launch.
E. The plain gate (lirec_gate_fwd, lirec_gate_bwd_parts) in modes 0, 2, 3 (mode 3: the single-pass model), strided, both
   dropout sites of dEE against the oracle's masks, parts 0 against 1 then 2.
F. The staged gate (lirec_gate_fwd_ws / _bwd_ws): the wave-specialised tier and the persistent fallback tier, staged weights,
   parts 4 + 1 + 2, and the stride conditions that send a call back to the plain kernels.

A head without rows (n = 0) used to stop the process in plan_tiles_v -- a chunk length of 0, then a division by it -- as soon as it
reached lirec_linear_bwd(_group) or lirec_gate_bwd_parts: launch_gemm now treats an empty reduction as the zero product it is
(test_grouped_launch_with_a_member_without_rows).

Largest e_dev / max(e_yardstick, u) seen on the MI355X over every comparison of this file, per GEMM mode (the cap is 8):
  mode 0  4.79   dW of the 1100-row grouped heads: a k-sequential fp32 chain of 1100 terms against the CPU's blocked sum
  mode 1  4.79   the same element -- the naive kernel adds in the same order as the f32 MFMA chain
  mode 2  3.11   dEE of the wave-specialised gate, (128, 768, 768)
  mode 3  2.10   dEE of the gate at (32, 256, 256), single pass on the plain kernels
and the largest share of the hard bound any element used: 0.17 (mode 0), 0.15 (mode 1), 0.13 (mode 2), 0.10 (mode 3).
"""
import contextlib

import pytest
import torch

import gemm_cases as GC
from golden_util import _record
from lirec_amd import _lib, ops
from lirec_amd._lib import LirecError
from oracle import lirec_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
TINY = 1e-300
SEED = GC.DROP_SEED
RATIOS_SEEN = {}                    # gemm mode -> largest e_dev / max(e_yardstick, u) of this session


def debug_set(ablate, force_cfg):
    assert _lib.lib().lirec_debug_set(int(ablate), int(force_cfg)) == 0


def sync():
    torch.cuda.synchronize()


@contextlib.contextmanager
def core(mode, force_cfg=-1, scratch_floats=0, overwrite=False):
    """a library context of its own with the GEMM mode, the forced configuration and (optionally) a NaN-filled scratch; yields the
    scratch tensor or None"""
    ctx = ops.Context()
    try:
        with ctx:
            scratch = None
            try:
                ops.set_gemm_mode(mode)
                debug_set(0, force_cfg)
                if scratch_floats:
                    scratch = torch.full((scratch_floats,), NAN, dtype=torch.float32, device=DEV)
                    _lib.check(_lib.lib().lirec_set_scratch(scratch.data_ptr(), 4 * scratch_floats), 'lirec_set_scratch')
                if overwrite:
                    ops.set_grad_overwrite(True)
                yield scratch
                sync()
            finally:
                ops.set_grad_overwrite(False)
                debug_set(0, -1)
                _lib.lib().lirec_set_scratch(None, 0)
                ops.set_gemm_mode(_lib.default_gemm_mode())
    finally:
        ctx.close()


def check(x, ref, what, mode):
    """both criteria of gemm_cases.py for the device tensor x (already on the CPU)"""
    n_hard, e, cap, e_y = GC.violations(x, ref)
    err = (torch.nan_to_num(x.double(), nan=1e30) - ref.model).abs()
    scale = float(ref.model.abs().max()) if ref.model.numel() else 0.0
    ratio = e / max(e_y, GC.U)
    _record(what + ' :: hard bound', err, GC.hard_bound(ref) + TINY, scale)
    _record(what + ' :: e_dev', torch.tensor([e]), torch.tensor([cap]), 1.0)
    _record(what + ' :: e_yardstick', torch.tensor([e_y]), torch.tensor([max(e_y, GC.U)]), 1.0)
    _record(what + ' :: ratio', torch.tensor([ratio]), torch.tensor([GC.MARGIN]), 1.0)
    RATIOS_SEEN[mode] = max(RATIOS_SEEN.get(mode, 0.0), ratio)
    print('%s: e_dev %.3e e_yardstick %.3e ratio %.3f beyond the hard bound %d' % (what, e, e_y, ratio, n_hard))
    assert n_hard == 0, '%s: %d elements beyond the hard bound (e_dev %.3e, K %d)' % (what, n_hard, e, ref.K)
    assert e <= cap, '%s: e_dev %.3e > 8 max(e_yardstick %.3e, u)' % (what, e, e_y)


class Head:
    """the operands and outputs of one linear head, placed"""

    def __init__(self, n, K, N, placement, overwrite=False, seed=0):
        d = GC.linear_data(n, K, N, seed)
        P = lambda r, c, data=None, strided=True: GC.Placed(r, c, placement, DEV, data=data, strided=strided)
        self.n, self.K, self.N, self.d, self.overwrite, self.seed = n, K, N, d, overwrite, seed
        self.A, self.W, self.b = P(n, K, d['A']), P(N, K, d['W'], strided=False), P(1, N, d['b'].view(1, N), strided=False)
        self.dY, self.act, self.tanh = P(n, N, d['dY']), P(n, K, d['act']), P(n, K, d['tanh'])
        self.Y, self.dA = P(n, N).poison(), P(n, K).poison()
        self.dW, self.db = P(N, K, strided=False), P(1, N, strided=False)
        self.reset_grads()

    def reset_grads(self):
        if self.overwrite:
            self.dW.poison(); self.db.poison()
        else:
            self.dW.set(self.d['dW0']); self.db.set(self.d['db0'].view(1, self.N))

    def fwd_item(self):
        return (self.A.ptr, self.A.ld, self.W.t, self.b.t, self.n, self.K, self.N, self.Y.t, self.Y.ld)

    def bwd_item(self, variant=(0, 0, 0.0), with_da=True):
        mode, acc, p = variant
        if acc:
            self.dA.set(self.d['dA0'])
        else:
            self.dA.poison()
        act = {0: None, 1: self.act, 2: self.tanh}[mode]
        return (self.dY.t, self.dY.ld, self.A.ptr, self.A.ld, self.W.t, self.n, self.K, self.N, self.dW.t, self.db.t,
                self.dA.ptr if with_da else None, self.dA.ld, mode, act.ptr if act is not None else None,
                act.ld if act is not None else 0, acc, ops.make_dropout(SEED, p, 0, O.SITE_E_CTX))

    def placed(self):
        return [self.A, self.W, self.b, self.dY, self.act, self.tanh, self.Y, self.dA, self.dW, self.db]

    def guards(self, what):
        sync()
        for i, pl in enumerate(self.placed()):
            assert pl.guards_intact(), '%s: a guard value around operand %d was overwritten' % (what, i)

    def check_fwd(self, arith, what, mode):
        check(self.Y.get(), GC.linear_refs(self.n, self.K, self.N, arith, self.overwrite, self.seed)['Y'], what + ' Y', mode)

    def check_wgrad(self, arith, what, mode):
        refs = GC.linear_refs(self.n, self.K, self.N, arith, self.overwrite, self.seed)
        check(self.dW.get(), refs['dW'], what + ' dW', mode)
        check(self.db.get().view(-1), refs['db'], what + ' db', mode)

    def check_da(self, arith, variant, what, mode):
        m, acc, p = variant
        ref = GC.da_ref(self.n, self.K, self.N, arith, m, acc, p, self.seed)
        check(self.dA.get(), ref, '%s dA epi%d acc%d p%.1f' % (what, m, acc, p), mode)


def tid(t):
    return '(%s)' % ','.join(str(v) for v in t)


def form_id(f):
    return 'mode%d-cfg%d' % f


# ---------------------------------------------------------------------------------------------------------------------------
# A. tile forms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('triple', GC.TRIPLES, ids=tid)
@pytest.mark.parametrize('form', GC.TILE_FORMS, ids=form_id)
def test_linear_tile_forms(form, triple):
    mode, cfg = form
    arith = GC.arith_of(mode)
    n, K, N = triple
    with core(mode, cfg):
        for placement in GC.PLACEMENTS:
            h = Head(n, K, N, placement)
            what = 'mode%d' % mode
            ops.linear_fwd(*h.fwd_item())
            h.check_fwd(arith, what, mode)
            y1 = h.Y.get()
            h.Y.poison()
            ops.linear_fwd_group([h.fwd_item()])
            assert torch.equal(y1, h.Y.get()), 'lirec_linear_fwd_group of one head differs from lirec_linear_fwd'
            # the single-head entry point once (all three GEMMs), then the data gradient's other variants through the group's
            ops.linear_bwd(*h.bwd_item(GC.DA_VARIANTS[0]))
            h.check_wgrad(arith, what, mode)
            h.check_da(arith, GC.DA_VARIANTS[0], what, mode)
            for variant in GC.DA_VARIANTS[1:]:
                ops.linear_bwd_group([h.bwd_item(variant)], parts=2)
                h.check_da(arith, variant, what, mode)
            h.reset_grads()
            ops.linear_bwd_group([h.bwd_item(with_da=False)], parts=1)
            h.check_wgrad(arith, what + ' (parts 1)', mode)
            h.guards('%s %s' % (triple, placement))


# ---------------------------------------------------------------------------------------------------------------------------
# B. split-K
# ---------------------------------------------------------------------------------------------------------------------------
def scratch_written(scratch, prob, plan, extent, what):
    """the slabs of the planned split hold numbers, the float behind the planned extent does not"""
    sync()
    ks = plan[0]
    s = scratch.cpu()
    if ks > 1:
        assert not bool(torch.isnan(s[:ks * prob.M * prob.N]).any()), what + ': a slab element of the planned split was not written'
        if prob.dbias:
            assert not bool(torch.isnan(s[ks * prob.M * prob.N:extent]).any()), what + ': bias-gradient slab'
    assert bool(torch.isnan(s[extent:extent + 4096]).all()), what + ': the scratch was written beyond the planned extent'
    scratch.fill_(NAN)


@pytest.mark.parametrize('triple', GC.SPLIT, ids=tid)
@pytest.mark.parametrize('form', GC.SPLIT_FORMS, ids=form_id)
def test_split_k(form, triple):
    mode, cfg = form
    arith = GC.arith_of(mode)
    n, K, N = triple
    probs = GC.linear_problems(n, K, N)
    what = 'mode%d split' % mode
    runs = []
    with core(mode, cfg, GC.SPLIT_SCRATCH_FLOATS) as scratch:
        for rep in range(2):
            h = Head(n, K, N, 'dense')
            plan = lambda layout: GC.plan_launch(layout, mode, cfg, [probs[layout]], GC.SPLIT_SCRATCH_FLOATS)
            ops.linear_fwd(*h.fwd_item())
            _, pl, ext = plan(GC.L_NT)
            scratch_written(scratch, probs[GC.L_NT], pl[0], ext, what + ' Y')
            ops.linear_bwd_group([h.bwd_item(with_da=False)], parts=1)
            _, pl, ext = plan(GC.L_TN)
            scratch_written(scratch, probs[GC.L_TN], pl[0], ext, what + ' dW')
            assert pl[0][0] > 1 or probs[GC.L_TN].K < 512
            ops.linear_bwd_group([h.bwd_item((0, 1, 0.0))], parts=2)
            _, pl, ext = plan(GC.L_NN)
            scratch_written(scratch, probs[GC.L_NN], pl[0], ext, what + ' dA')
            if rep == 0:
                h.check_fwd(arith, what, mode)
                h.check_wgrad(arith, what, mode)
                h.check_da(arith, (0, 1, 0.0), what, mode)
                # an epilogue keeps the data gradient unsplit: the scratch stays untouched
                ops.linear_bwd_group([h.bwd_item((2, 0, 0.3))], parts=2)
                scratch_written(scratch, probs[GC.L_NN], (1, 0), 0, what + ' dA (tanh)')
                h.check_da(arith, (2, 0, 0.3), what, mode)
                ops.linear_bwd_group([h.bwd_item((0, 1, 0.0))], parts=2)
                sync()
                scratch.fill_(NAN)
            h.guards(what)
            runs.append([t.get() for t in (h.Y, h.dW, h.db, h.dA)])
        for a, b in zip(*runs):
            assert torch.equal(a, b), 'a second run differs'
    with core(mode, cfg):
        h = Head(n, K, N, 'dense')
        ops.linear_fwd(*h.fwd_item())
        ops.linear_bwd(*h.bwd_item((0, 1, 0.0)))
        what = 'mode%d unsplit' % mode
        h.check_fwd(arith, what, mode)
        h.check_wgrad(arith, what, mode)
        h.check_da(arith, (0, 1, 0.0), what, mode)
        h.guards(what)


# ---------------------------------------------------------------------------------------------------------------------------
# C. poisoned outputs in the overwrite mode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('triple', GC.TRIPLES + GC.SPLIT, ids=tid)
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_overwritten_outputs_start_as_nan(mode, triple):
    arith = GC.arith_of(mode)
    n, K, N = triple
    split = triple in GC.SPLIT
    for scratch_floats in ([GC.SPLIT_SCRATCH_FLOATS, 0] if split else [0]):
        for placement in (['dense'] if split else ['dense', 'ld1']):
            with core(mode, -1, scratch_floats, overwrite=True):
                what = 'mode%d overwrite%s' % (mode, ' split' if scratch_floats else '')
                h = Head(n, K, N, placement, overwrite=True)
                ops.linear_fwd(*h.fwd_item())
                h.check_fwd(arith, what, mode)
                for variant in ((0, 0, 0.0), (1, 0, 0.3), (2, 1, 0.3)):
                    h.reset_grads()
                    ops.set_grad_overwrite(True)                   # (forgets the targets of the call before)
                    ops.linear_bwd(*h.bwd_item(variant))
                    assert ops.grad_overwrite_conflicts() == 0
                    h.check_wgrad(arith, what, mode)
                    h.check_da(arith, variant, what, mode)
                h.guards(what)


# ---------------------------------------------------------------------------------------------------------------------------
# D. grouped launches
# ---------------------------------------------------------------------------------------------------------------------------
GROUP_FORMS = [(2, -1), (2, 0), (2, 3), (0, -1), (0, 1), (1, -1)]


def run_group(form, members, variants, placement='dense', overwrite=False):
    mode, cfg = form
    arith = GC.arith_of(mode)
    with core(mode, cfg, overwrite=overwrite):
        heads = [Head(*t, placement, overwrite=overwrite, seed=i + 1) for i, t in enumerate(members)]
        ops.linear_fwd_group([h.fwd_item() for h in heads])
        ops.linear_bwd_group([h.bwd_item(v) for h, v in zip(heads, variants)])
        for i, (h, v) in enumerate(zip(heads, variants)):
            what = 'mode%d group[%d]' % (mode, i)
            h.check_fwd(arith, what, mode)
            h.check_wgrad(arith, what, mode)
            h.check_da(arith, v, what, mode)
            h.guards(what)
        if overwrite:
            assert ops.grad_overwrite_conflicts() == 0


@pytest.mark.parametrize('name', ['pgroup', 'two_tier'])
@pytest.mark.parametrize('form', GROUP_FORMS, ids=form_id)
def test_grouped_tile_orders(form, name):
    """'pgroup': both problems 18 x 2 tiles of 64 x 64 -- one tier, panel groups of 16 row panels, the last one of 2;
    'two_tier': heights 40 and 1100, the short one first (tests/test_host_gemm_cases.py checks the restated rule)"""
    run_group(form, GC.GROUPS[name], [(0, 0, 0.0), (0, 1, 0.0)])


@pytest.mark.parametrize('overwrite', [False, True])
@pytest.mark.parametrize('form', GROUP_FORMS, ids=form_id)
def test_grouped_launch_with_a_member_without_rows(form, overwrite):
    """n = 0: no output rows, and weight / bias gradients that keep their value (cleared in the overwrite mode)"""
    run_group(form, GC.GROUPS['empty_member'], [(0, 0, 0.0), (0, 1, 0.0), (1, 1, 0.3), (2, 0, 0.3)], 'ld4', overwrite)


@pytest.mark.parametrize('placement', ['dense', 'ld1'])
@pytest.mark.parametrize('form', GROUP_FORMS, ids=form_id)
def test_grouped_mixed_epilogues(form, placement):
    """store, relu-backward and tanh-backward with accumulate in ONE data-gradient launch"""
    run_group(form, GC.GROUPS['mixed_epilogues'], [(0, 0, 0.0), (1, 0, 0.3), (2, 1, 0.3)], placement)


def test_single_head_without_rows():
    for mode in (0, 1, 2):
        for overwrite in (False, True):
            with core(mode, overwrite=overwrite):
                h = Head(0, 33, 31, 'dense', overwrite=overwrite)
                ops.linear_fwd(*h.fwd_item())
                ops.linear_bwd(*h.bwd_item())
                h.check_wgrad(GC.arith_of(mode), 'mode%d n=0' % mode, mode)
                h.guards('n = 0')


# ---------------------------------------------------------------------------------------------------------------------------
# E / F. the gate
# ---------------------------------------------------------------------------------------------------------------------------
class Gate:
    def __init__(self, n, K, N, split, placement, p, acc_first, out_placement=None, tn_zero=False):
        d = GC.gate_data(n, K, N)
        out_placement = out_placement or placement
        P = lambda r, c, data=None, strided=True, pl=placement: GC.Placed(r, c, pl, DEV, data=data, strided=strided)
        self.n, self.K, self.N, self.split, self.p, self.acc_first, self.d = n, K, N, split, p, acc_first, d
        self.EE, self.Wg, self.bg = P(n, K, d['EE']), P(N, K, d['Wg'], strided=False), P(1, N, d['bg'].view(1, N), strided=False)
        self.dZg = P(n, N, d['dZg'])
        self.Tn = P(n, K, torch.zeros(n, K) if tn_zero else d['Tn'], pl=out_placement)
        self.G, self.dEE = P(n, N, pl=out_placement), P(n, K, pl=out_placement)
        self.dW, self.db = P(N, K, strided=False), P(1, N, strided=False)
        self.reset()

    def reset(self):
        self.G.poison()
        self.dW.set(self.d['dW0']); self.db.set(self.d['db0'].view(1, self.N))
        start = torch.full((self.n, self.K), NAN)
        if self.acc_first:
            start[:, :self.split] = self.d['dEE0'][:, :self.split]
        self.dEE.set(start)

    def fwd(self, ws=None, weights_staged=False):
        ops.gate_fwd(self.EE.t, self.EE.ld, self.Wg.t, self.bg.t, self.n, self.K, self.N, self.G.t, self.G.ld,
                     ops.make_dropout(SEED, self.p, O.SITE_GATE), ws=ws, weights_staged=weights_staged)

    def bwd(self, parts=0, ws=None, rows_staged=False):
        ops.gate_bwd(self.dZg.t, self.dZg.ld, self.EE.t, self.EE.ld, self.Wg.t, self.n, self.K, self.N, self.split, self.Tn.t,
                     self.Tn.ld, self.dW.t, self.db.t, self.dEE.t, self.dEE.ld, self.acc_first, ops.make_dropout(SEED, self.p),
                     O.SITE_E_CTX, O.SITE_E_INTS, parts=parts, ws=ws, rows_staged=rows_staged)

    def outputs(self):
        return [t.get() for t in (self.G, self.dW, self.db, self.dEE)]

    def guards(self, what):
        sync()
        for i, pl in enumerate([self.EE, self.Wg, self.bg, self.dZg, self.Tn, self.G, self.dEE, self.dW, self.db]):
            assert pl.guards_intact(), '%s: a guard value around operand %d was overwritten' % (what, i)

    def check(self, arith, what, mode, db_values='f32', tn_zero=False, fwd=True, bwd=True):
        refs = GC.gate_refs(self.n, self.K, self.N, self.split, arith, self.p, self.acc_first, tn_zero=tn_zero, db_values=db_values)
        if fwd:
            check(self.G.get(), refs['G'], what + ' G', mode)
        if bwd:
            check(self.dW.get(), refs['dWg'], what + ' dWg', mode)
            check(self.db.get().view(-1), refs['dbg'], what + ' dbg', mode)
            check(self.dEE.get(), refs['dEE'], what + ' dEE', mode)


@pytest.mark.parametrize('acc_first', [0, 1])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('shape', GC.GATE_PLAIN, ids=tid)
@pytest.mark.parametrize('mode', [0, 2, 3])
def test_plain_gate(mode, shape, p, acc_first):
    n, K, N, split = shape
    arith = GC.arith_of(mode, gate_site=True)
    with core(mode):
        for placement in GC.PLACEMENTS:
            g = Gate(n, K, N, split, placement, p, acc_first)
            what = 'mode%d gate' % mode
            g.fwd()
            g.bwd(parts=0)
            g.check(arith, what, mode)
            whole = g.outputs()
            g.reset()
            g.fwd()
            g.bwd(parts=1)
            g.bwd(parts=2)
            for a, b in zip(whole, g.outputs()):
                assert torch.equal(a, b), 'parts 1 then 2 differ from parts 0'
            g.guards('%s %s' % (shape, placement))


def gate_ws(n, K, N, fill=None):
    ws = torch.empty(ops.gate_ws_bytes(n, K, N), dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    return ws


def staged_tier(mode, shape):
    """'p3' (wave-specialised), 'p2' (persistent fallback) or 'plain' for a dense call with a workspace"""
    n, K, N, split = shape
    if not GC.gate_q32_ok(mode, n, K, N, K):
        return 'plain'
    return 'p3' if GC.gate_p3_ok(mode, n, K, N, split) else 'p2'


@pytest.mark.parametrize('acc_first', [0, 1])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('shape', GC.GATE_WS_P3 + GC.GATE_WS_P2, ids=tid)
@pytest.mark.parametrize('mode', [2, 3])
def test_staged_gate(mode, shape, p, acc_first):
    """both tiers of lirec_gate_fwd_ws / _bwd_ws against the models (mode 3: single pass; a shape the single-pass kernels do not
    take falls back to the plain kernels -- single pass too); the bias gradient of the wave-specialised weight-gradient kernel is
    its staged operand times ones: hi + lo (mode 2) or the bf16 values (mode 3).  Tn is non-zero; with acc_first the outputs and Tn
    are views into wider buffers.  Then: staged weights, and parts 4 + 1 + 2 with rows_staged, bit for bit."""
    n, K, N, split = shape
    arith = GC.arith_of(mode, gate_site=True)
    tier = staged_tier(mode, shape)
    assert tier == ('p3' if shape in GC.GATE_WS_P3 else ('p2' if mode == 2 else 'plain'))
    db_values = {'p3': arith, 'p2': 'f32', 'plain': 'f32'}[tier]
    with core(mode):
        g = Gate(n, K, N, split, 'dense', p, acc_first, out_placement='ld4' if acc_first else 'dense')
        what = 'mode%d staged gate (%s)' % (mode, tier)
        ws = gate_ws(n, K, N)
        g.fwd(ws=ws)
        g.bwd(parts=0, ws=ws)
        g.check(arith, what, mode, db_values=db_values)
        whole = g.outputs()
        # parts 4 + 1 + 2 on rows staged once
        g.reset()
        g.fwd(ws=ws)
        g.bwd(parts=4, ws=ws)
        g.bwd(parts=1, ws=ws, rows_staged=True)
        g.bwd(parts=2, ws=ws, rows_staged=True)
        for a, b in zip(whole, g.outputs()):
            assert torch.equal(a, b), 'parts 4 + 1 + 2 differ from parts 0'
        # the weights staged by a call of their own, into a fresh workspace
        g.reset()
        ws2 = gate_ws(n, K, N, fill=0xA5)
        staged = ops.gate_stage_weights(g.Wg.t, n, K, N, ws2)
        assert staged == (tier != 'plain')
        if staged:
            g.fwd(ws=ws2, weights_staged=True)
            g.bwd(parts=0, ws=ws2)
            for a, b in zip(whole, g.outputs()):
                assert torch.equal(a, b), 'staged weights differ from the one-call form'
        else:
            with pytest.raises(LirecError):
                g.fwd(ws=ws2, weights_staged=True)
        g.guards(what)


@pytest.mark.parametrize('why', ['ldee', 'lddzg', 'split'])
def test_staged_gate_stride_fallbacks(why):
    """ldee = K + 4 (forward and backward), lddzg = N + 4 or 2 split != K (backward): the call with a workspace runs the plain
    kernels -- bit for bit the call without one --, part 4 does nothing and the workspace is not touched"""
    n, K, N, split = 96, 512, 768, (128 if why == 'split' else 256)
    mode = 2
    with core(mode):
        res = []
        for with_ws in (True, False):
            g = Gate(n, K, N, split, 'dense', 0.3, 1)
            if why == 'ldee':
                g.EE = GC.Placed(n, K, 'ld4', DEV, data=g.d['EE'])
            if why == 'lddzg':
                g.dZg = GC.Placed(n, N, 'ld4', DEV, data=g.d['dZg'])
            ws = gate_ws(n, K, N, fill=0xA5) if with_ws else None
            if why == 'ldee' or not with_ws:
                g.fwd(ws=ws)
            else:
                g.fwd(ws=gate_ws(n, K, N))                        # (the forward qualifies: it stages into a workspace of its own)
            if with_ws:
                g.bwd(parts=4, ws=ws)
                g.bwd(parts=1, ws=ws, rows_staged=True)
                g.bwd(parts=2, ws=ws, rows_staged=True)
                sync()
                assert bool((ws == 0xA5).all()), 'the workspace was written by a call that fell back'
                if why == 'ldee':
                    with pytest.raises(LirecError):
                        g.fwd(ws=ws, weights_staged=True)
            else:
                g.bwd(parts=0)
            g.check('x3', 'mode2 gate fallback (%s)' % why, mode)
            g.guards(why)
            res.append(g.outputs())
        for i, (a, b) in enumerate(zip(*res)):
            if i == 0 and why != 'ldee':
                continue                                            # (G: staged forward against plain forward -- not the same kernel)
            assert torch.equal(a, b), 'the fallback differs from the plain call'


def test_gate_stage_weights_declines():
    """shapes / modes the staged path does not take: gate_stage_weights answers False and writes nothing"""
    for mode, (n, K, N) in ((2, (33, 64, 65)), (2, (96, 500, 768)), (0, (96, 512, 768)), (3, (96, 512, 768))):
        with core(mode):
            ws = gate_ws(n, K, N, fill=0xA5)
            Wg = GC.gate_data(n, K, N)['Wg'].to(DEV)
            assert ops.gate_stage_weights(Wg, n, K, N, ws) is False
            sync()
            assert bool((ws == 0xA5).all())
