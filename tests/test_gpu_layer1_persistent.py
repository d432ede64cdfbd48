"""The persistent layer-1 kernels (gemm_p2.hpp, p2_partition.hpp: the forward K1 and the weight gradient dW1 with its
stream-K reduce and the fused first-layer Adam) at the level of an op, against a float64 reference of the same operation
computed on the GPU.

Every case drives ``ops.embed_fwd`` / ``ops.embed_bwd`` (or the two-head ``embed_fwd2`` / ``embed_bwd2``) with a ``planes``
workspace, as model.py does, and checks which path ran: the persistent path is the only one that issues the ``stage`` site in
forward and the ``embed_dW1_reduce`` site in backward (lirec_hip.hip: the fused staging launch, launch_p2<L_TN>).  The same case
is then run again with the planes path switched off (diagnostics bit 8): those sites must be absent and the results must still
meet the fp64 bounds -- or, for rows stored as q32b / q16b / q16c, which only the persistent kernels read, the call must fail.

Reference operands are rounded to bf16 wherever the storage or the mode rounds them: q16b / q16c / bf16 rows, and in the
single-pass mode (gemm mode 3) the first-layer weights as well.  The backward reference takes its relu decisions from the device's
own forward (H1 > 0), and the forward decisions may differ from the fp64 ones only where the pre-activation is within RELU_EPS of
0, in at most 8 + RELU_FRAC of the elements.

The single-pass weight gradient multiplies dZ1 rounded to bf16, and that dZ1 comes out of the data-gradient GEMM (split bf16x3
core) with ~6e-6 of its scale of error: the ~0.1 % of its elements that lie that close to a bf16 rounding midpoint round to the
other neighbour than the fp64 dZ1 does, one ulp each, which moves dW1 by ~5e-4 of its scale -- the rounding of an operand that
is right to fp32 grade, not an error of the kernel.  So in mode 3, like the relu decisions, the rounded operand is taken from
the device (its bf16 hi plane; the fp32 dZ1 rounded, where the on-the-fly kernel rounds it inside) and checked on its own: it
must be the fp64 dZ1 to the mode's bound, rounded to nearest (bit for bit the rounding of the device's fp32 dZ1 where that is
kept), differing from bf16(fp64 dZ1) in at most 8 + ROUND_FRAC of the elements; dW1 / db1 are then held to grad_close's bound
against that operand times the rows."""
import pytest
import torch

from golden_util import assert_close, grad_close
from lirec_amd import _lib, ops
from lirec_amd._lib import LirecError

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 20261016
RELU_EPS = 2e-5               # |pre-activation| within which a device relu decision may differ from the fp64 one
RELU_FRAC = 2e-5              # ... and the fraction of the elements where it may (tests/test_gpu_bench_shape.DeviceReluDecisions)
ROUND_FRAC = 1e-2             # mode 3: fraction of dZ1 elements whose bf16 rounding may differ from bf16(fp64 dZ1) (measured 0.14 %)
ABLATE_PLANES = 8             # lirec_debug_set bit: no planes path (plane_layout declines)
OUTS = [40, 24, 16, 8]        # second-layer widths of the segments (small: layer 2 is not under test here)


def tol(mode, ref):
    """the forward bound of tests/test_gpu_ops.py's split bf16x3 core (mode 2): 4e-5 of the output scale.  Mode 3 gets the same
    bound, wider than the (1e-4, 1e-5) that test_gpu_ops.tol returns for any mode but 2 (its own tests run modes 0-2): layer 2
    and the data-gradient GEMM run on that same split core in mode 3, and layer 1 -- fp32 accumulation of products of operands
    the reference rounds as well -- is held to it too."""
    if mode in (2, 3):
        return 1e-4, 4e-5 * float(ref.abs().max())
    return 1e-4, 1e-5


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


class Head:
    """one head of a call: plain (``n`` rows, row 0 of each group) or pooled (``n`` candidates x ``R`` context rows, compacted)"""

    def __init__(self, kind, n, J, dims, off0, R=1, density=1.0, hbits=False, site=(0, 2)):
        self.kind, self.n, self.J, self.dims, self.off0 = kind, n, J, list(dims), off0
        self.R, self.density, self.hbits, self.site = R, density, hbits, site
        self.offs = [off0 + sum(self.dims[:i]) for i in range(len(self.dims))]
        self.outs = OUTS[:len(self.dims)]
        self.rows = n * R if kind == 'pooled' else n
        self.n2 = n
        self.W = sum(self.outs)


def make_block(n, Rp1, D, g):
    return torch.randn(n, Rp1, D, generator=g).to(DEV)


def stored(X, storage):
    """(operand handed to the library, fp64 view of the values the kernels multiply)"""
    if storage == 'f32':
        return X, X.double()
    if storage == 'q32b':
        return ops.to_q32b(X), X.double()           # (hi + lo split, as the on-the-fly core splits fp32: within the mode's bound)
    if storage == 'q16b':
        return ops.to_q16b(X), bf(X).double()
    if storage == 'q16c':
        return ops.to_q16c(X), bf(X).double()
    if storage == 'bf16':
        return X.to(torch.bfloat16).contiguous(), bf(X).double()
    raise ValueError(storage)


def pooled_mask(h, g):
    n, R = h.n, h.R
    if h.density == 'one':
        m = torch.zeros(n, R)
        m[n // 2, R - 1] = 1.0
    elif h.density == 'none':
        m = torch.zeros(n, R)
    else:
        m = (torch.rand(n, R, generator=g) < h.density).float()
    return m.to(DEV)


def setup_head(h, X, Xref, Rp1, D, mode, p, g):
    """parameters, outputs, forward / backward argument pieces and the fp64 reference operands of one head"""
    J, ns = h.J, len(h.dims)
    s = {}
    s['W1'] = [(torch.randn(J, d, generator=g) / d ** 0.5).to(DEV) for d in h.dims]
    s['b1'] = [(torch.randn(J, generator=g) * 0.1).to(DEV) for _ in h.dims]
    s['W2'] = [(torch.randn(o, J, generator=g) / J ** 0.5).to(DEV) for o in h.outs]
    s['b2'] = [(torch.randn(o, generator=g) * 0.1).to(DEV) for o in h.outs]
    s['segs'] = ops.Segments(h.offs, h.dims, h.outs)
    if h.kind == 'plain':
        s['sel'] = (1, Rp1, 0)
        s['xrows'] = Xref[:, 0, :]
        s['pool'], s['cmp'], s['mask'] = None, None, None
    else:
        s['sel'] = (h.R, Rp1, 1)
        s['xrows'] = Xref[:, 1:h.R + 1, :].reshape(h.n * h.R, D)
        s['mask'] = pooled_mask(h, g)
        s['cmp'] = ops.compact_rows(s['mask'], h.n, h.R)
        s['Hbar'] = torch.full((h.n, ns * J), float('nan'), device=DEV)
        s['f'] = torch.full((h.n,), float('nan'), device=DEV)
        s['pool'] = (None, h.R, 1, s['Hbar'], s['f'], s['cmp'])
    s['H1'] = torch.full((h.rows, ns * J), float('nan'), device=DEV)
    s['E'] = torch.full((h.n2, h.W), float('nan'), device=DEV)
    s['Tn'] = torch.full((h.n2, h.W), float('nan'), device=DEV)
    s['hb'] = torch.empty(max(ops.hbits_bytes(h.rows, ns * J), 16), dtype=torch.uint8, device=DEV) if h.hbits else None
    gathered = isinstance(X, ops.Q32Block)
    s['planes'] = torch.full((ops.planes_bytes(h.rows, sum(h.dims), J, gathered, X.dtype == torch.bfloat16),), 0x3C,
                             dtype=torch.uint8, device=DEV)                      # (finite garbage: everything read is written first)
    s['drop'] = ops.make_dropout(SEED, p, h.site[0], h.site[1])
    s['W1ref'] = [bf(w).double() if mode == 3 else w.double() for w in s['W1']]
    return s


def fwd_args(h, s, X, D):
    return ops.embed_fwd_args(X, D, s['sel'], h.rows, h.J, s['segs'], s['W1'], s['b1'], s['W2'], s['b2'], s['H1'],
                              s['E'].data_ptr(), h.W, s['Tn'].data_ptr(), h.W, 1, s['drop'], pool=s['pool'],
                              planes=s['planes'], hbits=s['hb'])


def reference_fwd(h, s, p):
    """fp64: pre-activations Z1, H1 = relu(dropout(Z1)), and the layer-2 outputs (plain: per row; pooled: of the masked mean)"""
    ns, J = len(h.dims), h.J
    xr = s['xrows']
    Z1 = torch.cat([xr[:, o:o + d] @ w.t() + b.double() for o, d, w, b in zip(h.offs, h.dims, s['W1ref'], s['b1'])], 1)
    keep1 = ops.dropout_mask(h.rows, ns * J, SEED, p, h.site[0], DEV).bool() if p > 0 else torch.ones_like(Z1, dtype=torch.bool)
    sc = 1.0 / (1.0 - p)
    H1 = torch.relu(Z1) * keep1 * sc
    s['Z1'], s['keep1'], s['sc'] = Z1, keep1, sc
    return H1


def layer2_ref(h, s, H1, p):
    """fp64 layer 2 (+ the pooling of the pooled form) on a given H1: (Hbar, f, T, E)"""
    ns, J = len(h.dims), h.J
    Hbar, f = None, None
    A = H1
    if h.kind == 'pooled':
        m = s['mask'].double()
        div = m.sum(1, keepdim=True)
        div = torch.where(div == 0, torch.ones_like(div), div)
        Hbar = (H1.view(h.n, h.R, ns * J) * m.view(h.n, h.R, 1)).sum(1) / div
        f = (m.sum(1, keepdim=True) / div).view(-1)
        A = Hbar
    z2 = torch.cat([A[:, i * J:(i + 1) * J] @ s['W2'][i].double().t() + (f.view(-1, 1) if f is not None else 1.0) * s['b2'][i].double()
                    for i in range(ns)], 1)
    T = torch.tanh(z2)
    keep2 = ops.dropout_mask(h.n2, h.W, SEED, p, h.site[1], DEV).bool() if p > 0 else torch.ones_like(T, dtype=torch.bool)
    return Hbar, f, T, T * keep2 * (1.0 / (1.0 - p)), keep2


def device_rows(h, s):
    """(logical row ids the device computed, in H1's row order, or None = all rows; how many)"""
    if h.kind == 'pooled':
        nv = int(s['cmp'][2].item())
        return s['cmp'][0][:nv].long(), nv
    return None, h.rows


def check_forward(h, s, mode, p, tag):
    H1r = reference_fwd(h, s, p)
    rows, nv = device_rows(h, s)
    H1d = s['H1'][:nv]
    ref = H1r if rows is None else H1r[rows]
    assert torch.isfinite(H1d).all(), tag + ': H1 not written'
    assert_close(H1d, ref, *tol(mode, H1r), tag + ' H1')
    # relu decisions: the device's (H1 > 0) against the fp64 ones, apart only at rounding distance of 0
    dec = H1d > 0
    own = ref > 0
    diff = dec != own
    if bool(diff.any()):
        z = s['Z1'] if rows is None else s['Z1'][rows]
        worst = float(z[diff].abs().max())
        assert worst <= RELU_EPS, '%s: a relu decision differs at |z| = %.3e' % (tag, worst)
        assert int(diff.sum()) <= 8 + RELU_FRAC * diff.numel(), '%s: %d relu decisions differ' % (tag, int(diff.sum()))
    # layer 2 on the fp64 reference H1
    Hbar, f, T, E, keep2 = layer2_ref(h, s, H1r, p)
    if h.kind == 'pooled':
        for got, r, what in ((s['Hbar'], Hbar, 'Hbar'), (s['f'], f, 'fscale')):
            assert torch.isfinite(got).all(), tag + ': ' + what + ' not written'
            assert_close(got, r, *tol(mode, r), tag + ' ' + what)
    for got, r, what in ((s['Tn'], T, 'Tn'), (s['E'], E, 'E')):
        assert torch.isfinite(got).all(), tag + ': ' + what + ' not written'
        assert_close(got, r, *tol(mode, r), tag + ' ' + what)
    # the device relu decisions, expanded to every logical row (rows never computed: masked, decision irrelevant)
    full = torch.zeros(h.rows, len(h.dims) * h.J, dtype=torch.bool, device=DEV)
    if rows is None:
        full.copy_(dec)
    else:
        full[rows] = dec
    s['dec'] = full
    s['T'], s['keep2'] = T, keep2


def init_grads(h, s, acc, g):
    ns = len(h.dims)
    mk = (lambda t: (torch.randn(t.shape, generator=g) * 0.5).to(DEV)) if acc else (lambda t: torch.full_like(t, float('nan')))
    s['gW1'] = [mk(w) for w in s['W1']]
    s['gb1'] = [mk(b) for b in s['b1']]
    s['gW2'] = [mk(w) for w in s['W2']]
    s['gb2'] = [mk(b) for b in s['b2']]
    s['g0'] = [t.clone() for t in s['gW1'] + s['gb1'] + s['gW2'] + s['gb2']] if acc else None
    dE = torch.randn(h.n2, h.W, generator=g).to(DEV).double()
    s['dZ2'] = (dE * (1 - s['T'] ** 2) * s['keep2'] * s['sc']).float().contiguous()
    s['ws'] = torch.full((ops.workspace_bytes(h.rows + (h.n if h.kind == 'pooled' else 0), ns, h.J) // 4,), 3.0, device=DEV)


def bwd_args(h, s, X, D, adam=None):
    return ops.embed_bwd_args(X, D, s['sel'], h.rows, h.J, s['segs'], s['W2'], None if h.hbits else s['H1'], s['dZ2'].data_ptr(),
                              h.W, s['gW1'], s['gb1'], s['gW2'], s['gb2'], s['ws'], s['drop'], pool=s['pool'],
                              planes=s['planes'], hbits=s['hb'], adam=adam)


def half_ulp(x):
    """half a bf16 ulp of the bf16 values x (float64)"""
    return 2.0 ** (torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - 8)


def mode3_operand(h, s, dZ1, planes_on, tag):
    """the bf16 dZ1 the single-pass weight gradient multiplies ([rows, nseg J], 0 on rows never computed), checked against the
    fp64 dZ1: the device's fp32 dZ1 (where it is kept) to the mode's bound, the bf16 operand its round-to-nearest, and that a
    rounding of the fp64 dZ1 within the same bound"""
    ldh = len(h.dims) * h.J
    rows32 = (h.rows + 31) // 32 * 32
    rows, nv = device_rows(h, s)
    ref = dZ1 if rows is None else dZ1[rows]
    ws = s['ws']
    rt, at = tol(3, dZ1)
    f32 = None
    if h.kind == 'plain' or not planes_on:
        # (workspace: the fp32 dZ1 first -- every head of the on-the-fly path, the plain head of the planes path)
        f32 = ws[:nv * ldh].view(nv, ldh).double()
        assert_close(f32, ref, rt, at, tag + ' dZ1 (fp32)')
    if planes_on:
        # (the hi plane [rows32, nseg J]: behind the fp32 dZ1 of a plain head, at the start of a pooled head's workspace)
        base = 2 * rows32 * ldh if h.kind == 'plain' else 0
        op = ws.view(torch.bfloat16)[base:base + nv * ldh].view(nv, ldh).double()
        if f32 is not None:
            assert torch.equal(op, bf(f32)), tag + ': the hi plane is not the fp32 dZ1 rounded to nearest'
    else:
        op = bf(f32)
    err = (op - ref).abs()
    bound = half_ulp(op) + at + rt * ref.abs()
    assert bool((err <= bound).all()), '%s: bf16 dZ1 off the rounding of the fp64 one by %.3e' % (tag, float((err - bound).max()))
    flips = int((op != bf(ref)).sum())
    assert flips <= 8 + ROUND_FRAC * op.numel(), '%s: %d of %d bf16 dZ1 elements round otherwise' % (tag, flips, op.numel())
    full = torch.zeros_like(dZ1)
    if rows is None:
        full.copy_(op)
    else:
        full[rows] = op
    return full


def reference_bwd(h, s, mode, planes_on=True, tag=''):
    """fp64 gradients with the device's relu decisions: [dW1..., db1..., dW2..., db2...] (plus the initial values if accumulating)"""
    ns, J = len(h.dims), h.J
    dec = s['dec']
    H1b = s['Z1'] * dec * s['sc']                                   # (dec implies kept)
    Hbar, f, _, _, _ = layer2_ref(h, s, H1b, 0.0)
    dZ2 = s['dZ2'].double()
    A = Hbar if h.kind == 'pooled' else H1b
    dW2 = [dZ2[:, sum(h.outs[:i]):sum(h.outs[:i + 1])].t() @ A[:, i * J:(i + 1) * J] for i in range(ns)]
    fz = f.view(-1, 1) if f is not None else 1.0
    db2 = [(fz * dZ2[:, sum(h.outs[:i]):sum(h.outs[:i + 1])]).sum(0) for i in range(ns)]
    dA = torch.cat([dZ2[:, sum(h.outs[:i]):sum(h.outs[:i + 1])] @ s['W2'][i].double() for i in range(ns)], 1)
    if h.kind == 'pooled':
        m = s['mask'].double()
        div = m.sum(1, keepdim=True)
        div = torch.where(div == 0, torch.ones_like(div), div)
        dA = (dA.view(h.n, 1, ns * J) * (m / div).view(h.n, h.R, 1)).reshape(h.rows, ns * J)
    dZ1 = dA * dec * s['sc']
    xr = s['xrows']
    # (mode 3: the single-pass weight gradient multiplies dZ1 rounded to bf16; the persistent kernel also sums that for db1, the
    #  on-the-fly kernel the fp32 dZ1)
    op = mode3_operand(h, s, dZ1, planes_on, tag) if mode == 3 else dZ1
    dW1 = [op[:, i * J:(i + 1) * J].t() @ xr[:, o:o + d] for i, (o, d) in enumerate(zip(h.offs, h.dims))]
    db1 = [(op if planes_on else dZ1)[:, i * J:(i + 1) * J].sum(0) for i in range(ns)]
    out = dW1 + db1 + dW2 + db2
    if s['g0'] is not None:
        out = [r + g0.double() for r, g0 in zip(out, s['g0'])]
    return out


def check_backward(h, s, mode, tag, planes_on=True):
    ref = reference_bwd(h, s, mode, planes_on, tag)
    got = s['gW1'] + s['gb1'] + s['gW2'] + s['gb2']
    ns = len(h.dims)
    names = ['dW1[%d]' % i for i in range(ns)] + ['db1[%d]' % i for i in range(ns)] + \
        ['dW2[%d]' % i for i in range(ns)] + ['db2[%d]' % i for i in range(ns)]
    for gt, r, nm in zip(got, ref, names):
        grad_close(gt, r, '%s %s' % (tag, nm))


def prof_sites():
    torch.cuda.synchronize()
    return ops.profile_read()


def run_case(heads, storage, mode, p, acc=True, ablate=False, seed=0, refused=False):
    """One forward + backward of the given heads (one call, or the two-head call) on the planes path (ablate: with it switched
    off).  Returns the profiled sites of the forward and of the backward call.  ``refused``: the forward call must fail with
    LIREC_EINVAL before any launch (rows stored in a blocked form without the planes path), and nothing else runs."""
    g = torch.Generator().manual_seed(1000 + seed)
    Rp1 = max([h.R + 1 if h.kind == 'pooled' else 2 for h in heads])
    D = max(h.offs[-1] + h.dims[-1] for h in heads)
    D = (D + 63) // 64 * 64
    n = heads[0].n
    assert all(h.n == n for h in heads)
    X0 = make_block(n, Rp1, D, g)
    X, Xref = stored(X0, storage)
    ss = [setup_head(h, X, Xref, Rp1, D, mode, p, g) for h in heads]
    tag = '%s mode %d p %.1f%s' % (storage, mode, p, ' (planes off)' if ablate else '')
    ops.ensure_scratch(DEV)
    L = _lib.lib()
    ops.set_gemm_mode(mode)
    try:
        L.lirec_debug_set(ABLATE_PLANES if ablate else 0, -1)
        fa = [fwd_args(h, s, X, D) for h, s in zip(heads, ss)]
        ops.profile_enable(True)
        fwd = (lambda: ops.embed_fwd2(fa[0], fa[1])) if len(heads) == 2 else (lambda: ops.embed_fwd(args=fa[0]))
        if refused:
            with pytest.raises(LirecError, match=r'lirec_embed_fwd2? failed: .*\(code %d\)' % _lib.LIREC_EINVAL):
                fwd()
            launched = prof_sites()
            assert not launched, ('the refused call launched work', launched)
            assert all(bool(torch.isnan(s['H1']).all()) for s in ss), 'the refused call wrote H1'
            return None
        fwd()
        fsites = prof_sites()
        for h, s in zip(heads, ss):
            check_forward(h, s, mode, p, tag)
            init_grads(h, s, acc, g)
        ops.set_grad_overwrite(not acc)
        ba = [bwd_args(h, s, X, D) for h, s in zip(heads, ss)]
        ops.profile_enable(True)
        if len(heads) == 2:
            ops.embed_bwd2(ba[0], ba[1])
        else:
            ops.embed_bwd(args=ba[0])
        bsites = prof_sites()
        ops.set_grad_overwrite(False)
        for h, s in zip(heads, ss):
            check_backward(h, s, mode, tag, planes_on=not ablate)
    finally:
        ops.profile_enable(False)
        ops.set_grad_overwrite(False)
        L.lirec_debug_set(0, -1)
        ops.set_gemm_mode(_lib.default_gemm_mode())
    return fsites, bsites


def persistent(fsites, bsites):
    """did the forward take the persistent path (the fused staging launch) and the backward its split-K dW1 (the reduce)?"""
    return fsites.get('stage', {}).get('launches', 0) > 0, bsites.get('embed_dW1_reduce', {}).get('launches', 0) > 0


def assert_persistent(fsites, bsites):
    f, b = persistent(fsites, bsites)
    assert f and fsites['embed_l1_fwd']['launches'] == 1, ('forward did not take the persistent path', fsites)
    assert b, ('backward did not take the persistent dW1 path', bsites)


def assert_fallback(fsites, bsites):
    f, b = persistent(fsites, bsites)
    assert not f and 'embed_l1_fwd' in fsites, ('forward took the persistent path', fsites)
    assert not b and 'embed_dW1' in bsites, ('backward took the persistent dW1 path', bsites)


def run_both(heads, storage, mode, p, acc=True, seed=0):
    """the persistent path, then the same case with the planes path off: the fallback (fp32 / bf16 blocks) or an error (rows
    stored in a blocked form only the persistent kernels read)"""
    assert_persistent(*run_case(heads, storage, mode, p, acc, seed=seed))
    if storage in ('f32', 'bf16'):
        assert_fallback(*run_case(heads, storage, mode, p, acc, ablate=True, seed=seed))
    else:
        run_case(heads, storage, mode, p, acc, ablate=True, seed=seed, refused=True)


# ---------------------------------------------------------------------------------------------------------------------------
# a plain head: row counts around the 32-row k-tail and the tile edges, hidden widths, one / two / four segments
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 31, 32, 33, 257, 4097])
def test_plain_head_rows(rows):
    run_both([Head('plain', rows, 256, [256], 0)], 'f32', 2, 0.3, seed=rows)


@pytest.mark.parametrize('J', [256, 512, 1024])
@pytest.mark.parametrize('rows,p,acc', [(33, 0.0, True), (257, 0.3, False)])
def test_plain_head_hidden_width(J, rows, p, acc):
    """two segments [256, 512] from a non-zero first column (a multiple of 32); accumulate and overwrite"""
    run_both([Head('plain', rows, J, [256, 512], 32)], 'f32', 2, p, acc, seed=J + rows)


def test_plain_head_bench_rows_model_segments():
    """~ the bench shape's 8121 rows, the model's four segments"""
    run_both([Head('plain', 8121, 512, [768, 2048, 256, 256], 0)], 'f32', 2, 0.3, seed=8121)


@pytest.mark.parametrize('J,dims', [(768, [256]), (256, [384])])
def test_declined_shapes_fall_back(J, dims):
    """J = 768 (p2_grid() % 3 != 0) and in_dim = 384 are not planes shapes: the on-the-fly core runs, and matches fp64"""
    h = [Head('plain', 257, J, dims, 0)]
    assert_fallback(*run_case(h, 'f32', 2, 0.3, seed=J))


# ---------------------------------------------------------------------------------------------------------------------------
# storage forms of the rows: staged fp32, gathered q32b / q16b / q16c, a row-major bf16 block staged in the mode's form
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [33, 257])
@pytest.mark.parametrize('storage,mode', [('q32b', 2), ('q16b', 2), ('bf16', 2), ('q16c', 3), ('bf16', 3)])
def test_plain_head_storage(storage, mode, rows):
    run_both([Head('plain', rows, 256, [256, 512], 64)], storage, mode, 0.3, seed=rows + 7 * mode)


# ---------------------------------------------------------------------------------------------------------------------------
# the pooled head on compacted rows (device-side row counts, 0 included), with and without the sign bits of H1
# ---------------------------------------------------------------------------------------------------------------------------
POOLED_N = {1: 300, 18: 64, 64: 40}


@pytest.mark.parametrize('density', [1.0, 0.05, 'one', 'none'])
@pytest.mark.parametrize('R', [1, 18, 64])
def test_pooled_head_compacted(R, density):
    run_both([Head('pooled', POOLED_N[R], 256, [256, 512], 32, R=R, density=density, hbits=True, site=(1, 3))], 'f32', 2, 0.3,
             seed=R)


@pytest.mark.parametrize('density', [1.0, 0.05, 'one', 'none'])
def test_pooled_head_without_sign_bits(density):
    run_both([Head('pooled', 64, 256, [256, 512], 32, R=18, density=density, hbits=False, site=(1, 3))], 'f32', 2, 0.0,
             acc=density != 0.05, seed=5)


@pytest.mark.parametrize('storage,mode', [('q32b', 2), ('q16c', 3)])
def test_pooled_head_gathered(storage, mode):
    run_both([Head('pooled', 64, 512, [256, 512], 64, R=18, density=0.3, hbits=True, site=(1, 3))], storage, mode, 0.3, seed=9)


# ---------------------------------------------------------------------------------------------------------------------------
# two heads in one call (embed_fwd2 / embed_bwd2: one merged persistent launch over up to LIREC_MAX_PROB = 8 problems)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,mode,acc', [('f32', 2, True), ('q32b', 2, False), ('bf16', 3, True)])
def test_two_heads_four_segments_each(storage, mode, acc):
    dims = [256, 512, 256, 256]
    heads = [Head('plain', 257, 512, dims, 0, site=(0, 2)),
             Head('pooled', 257, 512, dims, 0, R=18, density=0.3, hbits=True, site=(1, 3))]
    run_both(heads, storage, mode, 0.3, acc, seed=11)


def test_two_heads_one_and_three_segments():
    heads = [Head('plain', 100, 256, [256], 0, site=(0, 2)),
             Head('pooled', 100, 256, [256, 512, 256], 256, R=5, density=0.6, hbits=True, site=(1, 3))]
    run_both(heads, 'f32', 2, 0.3, seed=13)


# ---------------------------------------------------------------------------------------------------------------------------
# the fused first-layer Adam (lirec_fused_adam) against the unfused gradient + ops.adam_step, and the q32b / q16c shadow of W1
# ---------------------------------------------------------------------------------------------------------------------------
# (the forms of the update itself, at the smallest shape: the first step from zero moments, the step read from a device counter,
#  a gradient scale, no weight decay, and no shadow of the new weights)
FUSED_ADAM_FORMS = ['step1', 'step_dev7', 'gs0125', 'wd0', 'nowq']


@pytest.mark.parametrize('J,rows,dims,storage,mode,form',
                         [pytest.param(256, 33, [256, 512], 'f32', 2, None, id='256-33-dims0-f32-2'),
                          pytest.param(1024, 257, [256], 'f32', 2, None, id='1024-257-dims1-f32-2'),
                          pytest.param(256, 257, [256, 512], 'q16c', 3, None, id='256-257-dims2-q16c-3')] +
                         [pytest.param(256, 33, [256, 512], 'f32', 2, f, id='256-33-dims0-f32-2-' + f) for f in FUSED_ADAM_FORMS])
def test_fused_first_layer_adam(J, rows, dims, storage, mode, form):
    g = torch.Generator().manual_seed(J + rows)
    h = Head('plain', rows, J, dims, 0)
    D = (sum(dims) + 63) // 64 * 64
    X0 = make_block(rows, 2, D, g)
    X, Xref = stored(X0, storage)
    ops.ensure_scratch(DEV)
    # the flat layout FusedAdam uses: every W1 256-byte aligned, then the biases
    offs, o = [], 0
    for d in dims:
        offs.append(o); o += J * d
    boffs = []
    for _ in dims:
        boffs.append(o); o += J
    n = (o + 63) // 64 * 64
    n_params = sum(J * d + J for d in dims)
    flat = torch.zeros(n, device=DEV)
    s = setup_head(h, X, Xref, 2, D, mode, 0.3, g)
    for i, d in enumerate(dims):                                     # parameters as views of the flat buffer
        flat[offs[i]:offs[i] + J * d].copy_(s['W1'][i].view(-1)); s['W1'][i] = flat[offs[i]:offs[i] + J * d].view(J, d)
        flat[boffs[i]:boffs[i] + J].copy_(s['b1'][i]); s['b1'][i] = flat[boffs[i]:boffs[i] + J]
    s['W1ref'] = [bf(w).double() if mode == 3 else w.double() for w in s['W1']]
    gflat0 = (torch.randn(n, generator=g) * 0.01).to(DEV)
    m0 = (torch.randn(n, generator=g) * 0.01).to(DEV)
    v0 = (torch.rand(n, generator=g) * 1e-4).to(DEV)
    hyper = dict(step=3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5, grad_scale=1.0, step_dev=None)
    if form == 'step1':
        hyper['step'] = 1
        m0.zero_(); v0.zero_()
    elif form == 'step_dev7':
        hyper.update(step=0, step_dev=torch.tensor([7], dtype=torch.int64, device=DEV))
    elif form == 'gs0125':
        hyper['grad_scale'] = 0.125
    elif form == 'wd0':
        hyper['weight_decay'] = 0.0
    shadow = form != 'nowq'
    L = _lib.lib()
    ops.set_gemm_mode(mode)
    try:
        p0 = flat.clone()
        fa = fwd_args(h, s, X, D)
        ops.profile_enable(True)
        ops.embed_fwd(args=fa)
        fs = prof_sites()
        check_forward(h, s, mode, 0.3, 'adam fwd')
        init_grads(h, s, True, g)
        results = []
        for fused in (False, True):
            gflat = gflat0.clone()
            s['gW1'] = [gflat[offs[i]:offs[i] + J * d].view(J, d) for i, d in enumerate(dims)]
            s['gb1'] = [gflat[boffs[i]:boffs[i] + J] for i in range(len(dims))]
            for t, t0 in zip(s['gW1'] + s['gb1'], s['g0'][:2 * len(dims)]):
                t0.copy_(t)                                          # (the initial gradients the reference adds)
            for t, t0 in zip(s['gW2'] + s['gb2'], s['g0'][2 * len(dims):]):
                t.copy_(t0)
            flat.copy_(p0)
            m, v = m0.clone(), v0.clone()
            wq = torch.full((4 * n,), 0 if shadow else 0x5A, dtype=torch.uint8, device=DEV)
            adam = ops.fused_adam_args(flat, gflat, m, v, n_params, hyper['step'], hyper['lr'], hyper['beta1'], hyper['beta2'],
                                       hyper['eps'], hyper['weight_decay'], grad_scale=hyper['grad_scale'], step_dev=hyper['step_dev'],
                                       wq=wq if shadow else None, wq_first=0) if fused else None
            ops.profile_enable(True)
            ops.embed_bwd(args=bwd_args(h, s, X, D, adam=adam))
            bs = prof_sites()
            assert_persistent(fs, bs)
            if not fused:
                check_backward(h, s, mode, 'adam (unfused) J %d rows %d' % (J, rows))
            results.append((gflat.clone(), flat.clone(), m, v, wq))
    finally:
        ops.profile_enable(False)
        L.lirec_debug_set(0, -1)
        ops.set_gemm_mode(_lib.default_gemm_mode())
    (g1, _, _, _, _), (g2, p2, m2, v2, wq) = results
    assert torch.equal(g1, g2), 'the fused call stores another gradient'
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    ops.adam_step(pr, g1, mr, vr, hyper['step'], hyper['lr'], hyper['beta1'], hyper['beta2'], hyper['eps'], hyper['weight_decay'],
                  grad_scale=hyper['grad_scale'], step_dev=hyper['step_dev'])
    if hyper['step_dev'] is not None:
        assert int(hyper['step_dev']) == 7
    rng = torch.zeros(n, dtype=torch.bool, device=DEV)
    for i, d in enumerate(dims):
        rng[offs[i]:offs[i] + J * d] = True
        rng[boffs[i]:boffs[i] + J] = True
    for got, want, what in ((p2, pr, 'parameters'), (m2, mr, 'exp_avg'), (v2, vr, 'exp_avg_sq')):
        assert torch.equal(got[rng], want[rng]), what + ' differ from ops.adam_step on the unfused gradient'
        assert torch.equal(got[~rng], (p0 if what == 'parameters' else (m0 if what == 'exp_avg' else v0))[~rng]), what + ': outside W1 / b1'
    assert bool((pr[rng] != p0[rng]).any()) and bool((vr[rng] != v0[rng]).any())
    if not shadow:
        assert bool((wq == 0x5A).all()), 'no shadow was asked for, and the buffer a shadow would go to was written'
        return
    for i, d in enumerate(dims):
        neww = pr[offs[i]:offs[i] + J * d].view(J, d).contiguous()
        if mode == 3:
            want = ops.to_q16c(neww).data[:int(L.lirec_q16b_bytes(J, d))]
        else:
            want = ops.to_q32b(neww).data[:int(L.lirec_q32b_bytes(J, d))]
        got = wq[4 * offs[i]:4 * offs[i] + want.numel()]
        assert torch.equal(got, want), 'W1[%d] shadow differs from the new weights\' %s form' % (i, 'q16c' if mode == 3 else 'q32b')
