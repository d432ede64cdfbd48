"""The pooling family without a GPU: the yardstick of tests/test_gpu_pooling.py checked on its own -- the float64 masked mean and
un-pooling of tests/pool_cases.py against torch autograd of the un-pooled definition, the compaction reference against
torch.nonzero --, the mask generator's promises, the case list's claims, and the argument checks of the calls through the C ABI
(LIREC_EINVAL) under the library's host-side dry run, which hands nothing to the HIP runtime."""
import ctypes as C

import pytest
import torch

import pool_cases as PC
from lirec_amd import _lib

DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
A0 = 0x10000000                                # fake, aligned, never dereferenced device addresses


def _addr(i):
    return A0 + 0x1000000 * i


ALL_MASKS = sorted({(c.n, c.R, c.weighted, c.clamp) for c in PC.POOL_CASES} |
                   {(n, R, True, 1) for n, R, _ in PC.COMPACT_SHAPES} | {(5, 65, True, 1), (5, 64, False, 1), (9, 65, True, 0)})


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick on its own
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,R,weighted,clamp', ALL_MASKS)
def test_references_are_autograd_of_the_unpooled_definition(n, R, weighted, clamp):
    W = 6
    g = torch.Generator().manual_seed(n * 131 + R)
    mask = PC.make_mask(n, R, weighted, clamp, seed=R)
    z = torch.randn(n, R, W, generator=g, dtype=torch.float64, requires_grad=True)
    dHbar = torch.randn(n, W, generator=g, dtype=torch.float64)
    m = mask.double()
    div = m.sum(1)
    if clamp:
        div = torch.where(div == 0, torch.ones_like(div), div)
    pooled = (z * m.unsqueeze(2)).sum(1) / div.unsqueeze(1)
    (pooled * dHbar).sum().backward()
    Hbar, f, unit, valid = PC.masked_mean(z.detach(), mask, clamp)
    assert float((Hbar - pooled.detach()).abs().max()) <= 1e-12
    assert float((f - m.sum(1) / div).abs().max()) <= 1e-12 and set(f.tolist()) <= {0.0, 1.0}
    assert torch.equal(valid, (mask != 0).sum(1))
    assert bool((unit >= Hbar.abs() - 1e-12).all())             # (sum |m z| / |div| bounds the mean itself)
    # un-pooling with every relu decision 1 and scale 1 is the gradient of the masked mean ...
    ones = torch.ones(n, R, W, dtype=torch.bool)
    assert float((PC.unpool(dHbar, mask, clamp, 1.0, ones) - z.grad).abs().max()) <= 1e-12
    # ... and with decisions and a dropout scale, the gradient through relu(z) * scale
    z2 = z.detach().clone().requires_grad_(True)
    scale = PC.drop_scale(0.3)
    h = torch.relu(z2) * scale
    (((h * m.unsqueeze(2)).sum(1) / div.unsqueeze(1)) * dHbar).sum().backward()
    assert float((PC.unpool(dHbar, mask, clamp, scale, z2.detach() > 0) - z2.grad).abs().max()) <= 1e-12
    # the older pair: tanh of the mean, dropout on top; its backward
    keep = torch.rand(n, W, generator=g) < 0.7
    Tn, E = PC.pool_fwd_ref(z.detach(), mask, clamp, keep, 0.3)
    assert float((Tn - torch.tanh(pooled.detach())).abs().max()) <= 1e-12
    assert float((E - torch.tanh(pooled.detach()) * keep / 0.7).abs().max()) <= 1e-12
    assert float((PC.pool_bwd_ref(dHbar, mask, clamp) - z.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize('n,R,weighted,clamp', ALL_MASKS)
def test_compaction_reference_is_torch_nonzero(n, R, weighted, clamp):
    mask = PC.make_mask(n, R, weighted, clamp, seed=n)
    for mk in (mask, (mask * 2).long(), mask.double(), torch.zeros(n, R), torch.ones(n, R)):
        rowmap, cstart, count, wts = PC.compact_ref(mk)
        nz = torch.nonzero(mk.reshape(-1)).view(-1)
        assert count == nz.numel() and torch.equal(rowmap.long(), nz)
        assert cstart.numel() == n + 1 and int(cstart[0]) == 0 and int(cstart[n]) == count
        assert torch.equal(cstart[1:] - cstart[:-1], (mk != 0).sum(1).int())
        assert torch.equal(wts, mk.reshape(-1)[nz].float())


def test_drop_scale_is_the_fp32_quotient():
    assert PC.drop_scale(0.0) == 1.0
    s = PC.drop_scale(0.3)
    assert s == float(torch.tensor(s).float()) and abs(s - 1 / 0.7) < 1e-7


def test_pack_sign_bits_layout():
    H = torch.zeros(3, 260)
    H[1, 0] = 1; H[1, 9] = 2; H[2, 255] = 1; H[2, 256] = 1; H[2, 259] = 3; H[0, 5] = -1
    b = PC.pack_sign_bits(H)
    assert b.shape == (3, 64) and not bool(b[0].any())
    assert b[1].tolist() == [1, 2] + [0] * 62
    assert b[2].tolist() == [0] * 31 + [128, 1 | 8] + [0] * 31


# ---------------------------------------------------------------------------------------------------------------------------
# the mask generator and the case list
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,R,weighted,clamp', ALL_MASKS)
def test_mask_generator_keeps_its_promises(n, R, weighted, clamp):
    for seed in (0, R, n, 65):
        mask = PC.make_mask(n, R, weighted, clamp, seed=seed)
        assert mask.dtype == torch.float32 and mask.shape == (n, R)
        assert set(mask.unique().tolist()) <= ({0.0, 0.5, 1.0, 2.0} if weighted else {0.0, 1.0})
        pats = PC.patterns(n, R, clamp)
        names = {name for _, name, _ in pats}
        if n >= 8:
            assert {'none' if clamp else 'one_mid', 'one_first', 'one_last', 'all'} <= names
            assert {'valid_%d' % k for k in (8, 9, 15, 16) if k <= R} <= names
        for c, name, v in pats:
            assert int((mask[c] != 0).sum()) == v, (c, name)
            if name == 'one_first':
                assert mask[c, 0] != 0
            if name == 'one_last':
                assert mask[c, R - 1] != 0
        if not clamp:
            assert bool((mask != 0).any(1).all())                # no all-zero candidate: the reference would be NaN
        # every fp32 divider is exact: the fp32 sum, in either order, equals the float64 sum
        d64 = mask.double().sum(1)
        fwd = torch.zeros(n)
        bwd = torch.zeros(n)
        for r in range(R):
            fwd = fwd + mask[:, r]
            bwd = bwd + mask[:, R - 1 - r]
        assert torch.equal(fwd.double(), d64) and torch.equal(bwd.double(), d64) and torch.equal(mask.sum(1).double(), d64)


def test_case_list_covers_what_it_claims():
    S, F = PC.STREAMING, PC.FALLBACK
    assert all(c.family == 'streaming' for c in S) and all(c.family == 'fallback' for c in F)
    assert all(c.nseg <= _lib.MAX_SEG for c in PC.POOL_CASES)
    assert {1, 8, 9, 15, 33, 63, 64} <= {c.R for c in S} and {65, 130} <= {c.R for c in F}
    assert {8, 64, 260, 1024} <= {c.W for c in S} and 18 in {c.W for c in F}
    for cases in (S, F):
        assert {c.form for c in cases} == {'dense', 'wts', 'nowts'}
        assert {c.clamp for c in cases} == {0, 1} and {c.weighted for c in cases} == {False, True}
    # each fallback kernel on its float4 and on its scalar path
    assert {(c.form == 'dense', c.vec) for c in F} == {(False, False), (False, True), (True, False), (True, True)}
    # the sign bits with a partial last column block; a partial last workgroup; the wrap of the grid-stride loop
    assert any(c.hbits and c.W % 256 for c in S) and any(c.n % 4 for c in S)
    assert any(c.n * ((c.W + 255) // 256) > 2048 * 4 for c in S)
    shapes = {(n, R): p for n, R, p in PC.COMPACT_SHAPES}
    assert shapes[(5, 65)] == 'serial-lds' and PC.serial_staged(5, 65)
    assert shapes[(600, 65)] == 'serial-global' and not PC.serial_staged(600, 65)
    assert PC.serial_staged(1100, 30) and 1100 > 1024


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def _compact2(L, **kw):
    v = dict(mask=_addr(0), mask_dtype=0, n=9, R=5, rowmap=_addr(1), cstart=_addr(2), count=_addr(3), wts=_addr(4))
    v.update(kw)
    return L.lirec_compact_rows2(*v.values(), None)


@pytest.mark.parametrize('kw', [dict(mask_dtype=3), dict(mask_dtype=-1), dict(R=0), dict(rowmap=None), dict(cstart=None),
                                dict(count=None), dict(mask=None), dict(n=-1)], ids=lambda kw: '-'.join(kw))
def test_compact_rows_argument_checks(dry, kw):
    assert _compact2(dry, **kw) == _lib.LIREC_EINVAL
    assert _compact2(dry) == 0 and _compact2(dry, wts=None) == 0 and _compact2(dry, R=65) == 0 and _compact2(dry, n=0) == 0
    old = dict(mask=_addr(0), n=9, R=5, rowmap=_addr(1), cstart=_addr(2), count=_addr(3))
    assert dry.lirec_compact_rows(*old.values(), None) == 0
    if not set(kw) & {'mask_dtype', 'wts'}:
        old.update(kw)
        assert dry.lirec_compact_rows(*old.values(), None) == _lib.LIREC_EINVAL


def _fill(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = v


def _embed_args(cls, n=5, R=4, J=16, nseg=2):
    """a valid pooled, compact head (fake addresses): lirec_embed_fwd with parts 3 / lirec_embed_bwd with parts 5 reach the
    pooling / un-pooling pass without a GEMM in front of it"""
    a = cls()
    a.X, a.ldx = _addr(0), 8 * nseg
    a.H1, a.mask, a.Hbar, a.fscale = _addr(1), _addr(2), _addr(3), _addr(4)
    a.rowmap, a.cstart, a.count, a.wts = _addr(5), _addr(6), _addr(7), _addr(8)
    _fill(a.W2, [_addr(10 + i) for i in range(nseg)])
    _fill(a.in_off, [8 * i for i in range(nseg)]); _fill(a.in_dim, [8] * nseg); _fill(a.out_dim, [4] * nseg)
    a.rows, a.nseg, a.J, a.R, a.clamp_zero = n * R, nseg, J, R, 1
    a.sel = _lib.RowSel(R, R + 1, 1)
    if cls is _lib.EmbedFwdArgs:
        _fill(a.W1, [_addr(14 + i) for i in range(nseg)]); _fill(a.b1, [_addr(18 + i) for i in range(nseg)])
        _fill(a.b2, [_addr(22 + i) for i in range(nseg)])
        a.Z2, a.ldz2, a.parts = _addr(9), 4 * nseg, 3
    else:
        a.dZ2, a.lddz2, a.parts = _addr(9), 4 * nseg, 5
        for k, arr in enumerate((a.dW1, a.db1, a.dW2, a.db2)):
            _fill(arr, [_addr(26 + 4 * k + i) for i in range(nseg)])
        a.workspace, a.workspace_bytes = _addr(44), _lib.lib().lirec_workspace_bytes(n * R + n, nseg, J)
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _dense(**kw):
    def f(a):
        a.rowmap = a.cstart = a.count = a.wts = None
        _set(**kw)(a)
    return f


EMBED_BREAKS = {
    'wts_without_rowmap': _dense(wts=_addr(8)),
    'rowmap_without_cstart': _set(cstart=None),
    'rowmap_without_count': _set(count=None),
    'cstart_without_rowmap': _set(rowmap=None, wts=None),
    'compact_without_mask_or_wts': _set(mask=None, wts=None),
    'hbits_R65': _set(hbits=_addr(50), R=65, rows=5 * 65),
    'hbits_R65_dense': _dense(hbits=_addr(50), R=65, rows=5 * 65),
    'rows_not_a_multiple_of_R': _set(rows=5 * 4 + 1),
    'R0': _set(R=0),
    'no_Hbar': _set(Hbar=None),
    'no_fscale': _set(fscale=None),
}
EMBED_OK = {
    'as_is': _set(),
    'dense': _dense(),
    'without_wts': _set(wts=None),
    'wts_without_mask': _set(mask=None),
    'hbits_R64': _set(hbits=_addr(50), R=64, rows=5 * 64),
    'R65': _set(R=65, rows=5 * 65),
    'R65_dense': _dense(R=65, rows=5 * 65),
}


def _call(L, cls, edit, **shape):
    a = _embed_args(cls, **shape)
    edit(a)
    if cls is _lib.EmbedBwdArgs:
        a.workspace_bytes = L.lirec_workspace_bytes(a.rows + 5, a.nseg, a.J)
        return L.lirec_embed_bwd(C.byref(a), None)
    return L.lirec_embed_fwd(C.byref(a), None)


@pytest.mark.parametrize('cls', [_lib.EmbedFwdArgs, _lib.EmbedBwdArgs], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('what', sorted(EMBED_BREAKS))
def test_pooled_form_argument_checks(dry, what, cls):
    assert _call(dry, cls, EMBED_BREAKS[what]) == _lib.LIREC_EINVAL


@pytest.mark.parametrize('cls', [_lib.EmbedFwdArgs, _lib.EmbedBwdArgs], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('what', sorted(EMBED_OK))
def test_pooled_form_arguments_accepted(dry, what, cls):
    """the valid neighbours of every break pass (so each break is refused for its own reason)"""
    assert _call(dry, cls, EMBED_OK[what]) == 0


@pytest.mark.parametrize('cls', [_lib.EmbedFwdArgs, _lib.EmbedBwdArgs], ids=['fwd', 'bwd'])
def test_sign_bits_need_a_width_that_is_a_multiple_of_4(dry, cls):
    """W = 3 x 6 = 18 with ``hbits``: only the streaming kernels write / read the sign bits"""
    assert _call(dry, cls, _set(hbits=_addr(50)), J=6, nseg=3) == _lib.LIREC_EINVAL
    assert _call(dry, cls, _set(), J=6, nseg=3) == 0
    assert _call(dry, cls, _set(hbits=_addr(50)), J=8, nseg=3) == 0
