"""The resident block store without a GPU: the three exports and the two struct mirrors, every LIREC_EINVAL of their contracts before
any device call (with and without the library's host-side dry run), the consumption of lirec_set_feature_rows, a numpy restatement
of the storage-row mapping against a brute-force one, ``BlockLoader.layout`` against ``default_collate`` for the four recipes, and
the refusals of ``BlockStore``.  The addresses are fake, aligned and never dereferenced."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from lirec_amd import _lib, blockstore as BS
from lirec_amd.data import SyntheticMixedFeaturesDataset, collate
from lirec_amd.loader import BlockLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
FWD = _lib.EmbedFwdArgs
N, R, J, DIMS, OUT = 33, 2, 256, (256, 512), (16, 16)          # a shape plane_layout accepts (tests/test_host_embed_heads.py: BIG)
SMALL_DIMS = dict(text_dim=32, visual_dim=32, track_dim=32)


def _addr(i, sub=0):
    return 0x10000000 + 0x4000000 * i + 0x400000 * sub


IDS, SCRATCH = _addr(60), _addr(100)


def _fill(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = v


def _head(L, pooled, slot, **edit):
    """one head reading a q32b block of N samples of R + 1 rows: the interaction head (row 0 of each) or the pooled context head"""
    nseg, b = len(DIMS), 20 * slot
    a = FWD()
    a.X, a.ldx, a.H1, a.x_q32 = _addr(0), sum(DIMS), _addr(b + 1), 1
    a.rows, a.nseg, a.J, a.R = (N * R if pooled else N), nseg, J, R
    a.sel = _lib.RowSel(R, R + 1, 1) if pooled else _lib.RowSel(1, R + 1, 0)
    a.drop = _lib.Dropout(7, 0.3, 1 + 2 * slot, 2 + 2 * slot, None)
    if pooled:
        a.rowmap, a.cstart, a.count, a.wts = (_addr(b + 2 + k) for k in range(4))
        a.Hbar, a.fscale, a.clamp_zero = _addr(b + 6), _addr(b + 7), 1
    for k, arr in enumerate((a.W2, a.W1, a.b1, a.b2)):
        _fill(arr, [_addr(b + 8 + k, i) for i in range(nseg)])
    _fill(a.in_off, [sum(DIMS[:i]) for i in range(nseg)]); _fill(a.in_dim, DIMS); _fill(a.out_dim, OUT)
    a.Z2, a.ldz2, a.Tn, a.ldtn, a.epilogue = _addr(b + 12), sum(OUT), _addr(b + 13), sum(OUT), 1
    a.planes, a.planes_bytes = _addr(b + 17), L.lirec_planes_bytes(a.rows, sum(DIMS), J, 2)
    for k, v in edit.items():
        setattr(a, k, v)
    return a


def _rows(**kw):
    fr = dict(clip_ids=IDS, n_clips=N, rows_per_clip=R + 1, store_rows=(1000 * (R + 1) + 31) // 32 * 32)
    fr.update(kw)
    return _lib.FeatureRows(fr['clip_ids'], fr['n_clips'], fr['rows_per_clip'], fr['store_rows'])


def _call(L, heads, rows='default'):
    if rows is not None:
        assert L.lirec_set_feature_rows(C.byref(_rows() if rows == 'default' else rows)) == 0
    fn = L.lirec_embed_fwd if len(heads) == 1 else L.lirec_embed_fwd2
    return fn(*[C.byref(h) for h in heads], None)


def _env(dry_run):
    """gemm mode 2 with a split-K scratch registered (what the gathered q32b path asks for); everything put back afterwards"""
    from lirec_amd import ops
    L = _lib.lib()
    mode = L.lirec_get_gemm_mode()
    if dry_run:
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_set_gemm_mode(2) == 0 and L.lirec_set_scratch(SCRATCH, 256 << 20) == 0
        yield L
    finally:
        assert L.lirec_set_feature_rows(None) == 0
        assert L.lirec_set_scratch(None, 0) == 0 and L.lirec_set_gemm_mode(mode) == 0
        ops._scratch.pop(ops._ctx_key(), None)
        assert L.lirec_debug_set(0, -1) == 0


@pytest.fixture(params=[False, True], ids=['plain', 'dry-run'])
def lib(request):
    """the refusals: with the dry run and without it (a call that got past the checks would then reach the HIP runtime)"""
    yield from _env(request.param)


@pytest.fixture
def dry():
    """calls the library accepts: under the dry run only"""
    yield from _env(True)


def test_exports_binding_and_struct_sizes():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    for name in ('lirec_set_feature_rows', 'lirec_q32b_write_rows', 'lirec_collate_fields'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert L.lirec_abi_sizeof(21) == C.sizeof(_lib.FeatureRows) == 24
    assert L.lirec_abi_sizeof(23) == C.sizeof(_lib.CollateField) == 24
    assert L.lirec_abi_sizeof(20) == -1 and L.lirec_abi_sizeof(22) == -1 and L.lirec_abi_sizeof(24) == -1
    # no existing struct moved
    assert L.lirec_abi_sizeof(0) == C.sizeof(_lib.EmbedFwdArgs) and L.lirec_abi_sizeof(17) == C.sizeof(_lib.CollateArgs)
    assert int(re.search(r'#define LIREC_FEATURE_ROWS_MAX (\d+)', hdr).group(1)) == _lib.FEATURE_ROWS_MAX == 2 ** 31 - 32


PIECES = _lib.Pieces(_addr(70), 768, 5, _addr(71), 512, 5, _addr(72), 256, 512, 512)
# name -> (edits of the lirec_feature_rows, edits of every head, environment)
BAD_ROWS = {
    'x_q32 = 0: an fp32 block': ({}, dict(x_q32=0), None),
    'x_q32 = 2: q16b storage': ({}, dict(x_q32=2), None),
    'a bf16 block': ({}, dict(x_q32=0, x_bf16=1), None),
    'pieces set': ({}, dict(pieces=C.cast(C.pointer(PIECES), C.c_void_p)), None),
    'no planes workspace: the on-the-fly path': ({}, dict(planes=None, planes_bytes=0), None),
    'planes workspace too small': ({}, dict(planes_bytes=4096), None),
    'J the q32b kernels do not take': ({}, dict(J=128), None),
    'GEMM mode 0': ({}, {}, 'mode0'),
    'GEMM mode 1': ({}, {}, 'mode1'),
    'GEMM mode 3': ({}, {}, 'mode3'),
    'no split-K scratch': ({}, {}, 'noscratch'),
    'rows no multiple of the per-clip rows': (dict(rows_per_clip=2 * (R + 1), n_clips=N // 2), {}, None),      # N = 33 candidates, 2 a clip
    'rows_per_clip no multiple of the group stride': (dict(rows_per_clip=R + 2), {}, None),
    'n_clips * rows_per_clip below the physical rows': (dict(n_clips=N - 1), {}, None),
    'n_clips * rows_per_clip above the physical rows': (dict(n_clips=N + 1), {}, None),
    'store_rows = 2^31': (dict(store_rows=1 << 31), {}, None),
    'store_rows over the limit by 32': (dict(store_rows=_lib.FEATURE_ROWS_MAX + 32), {}, None),
    'store_rows 0': (dict(store_rows=0), {}, None),
    'clip_ids NULL': (dict(clip_ids=None), {}, None),
    'clip_ids misaligned': (dict(clip_ids=IDS + 2), {}, None),
    'n_clips 0': (dict(n_clips=0), {}, None),
    'rows_per_clip 0': (dict(rows_per_clip=0), {}, None),
    'parts 2: no rows are read': ({}, dict(parts=2), None),
    'parts 3: no rows are read': ({}, dict(parts=3), None),
    'an empty head': ({}, dict(rows=0), None),
}


@pytest.mark.parametrize('nheads', [1, 2])
@pytest.mark.parametrize('what', sorted(BAD_ROWS))
def test_armed_forward_refuses_before_any_device_call(lib, what, nheads):
    """without the dry run a call that got past the checks would reach the HIP runtime, which has no device here"""
    L = lib
    fr, edit, env = BAD_ROWS[what]
    if env and env.startswith('mode'):
        assert L.lirec_set_gemm_mode(int(env[4:])) == 0
    if env == 'noscratch':
        assert L.lirec_set_scratch(None, 0) == 0
    heads = [_head(L, False, 0, **edit)] + ([_head(L, True, 1, **edit)] if nheads == 2 else [])
    assert _call(L, heads, _rows(**fr)) == EINVAL, what


@pytest.mark.parametrize('parts', [0, 1, 4])
@pytest.mark.parametrize('kind', ['plain', 'pooled', 'both', 'ungrouped'])
def test_armed_forward_is_accepted_under_the_dry_run(dry, kind, parts):
    L = dry
    if kind == 'ungrouped':
        # no row selector (group 0): every row of every sample, rows_per_clip = 3
        heads, fr = [_head(L, False, 0, sel=_lib.RowSel(0, 0, 0), rows=3 * 11, parts=parts)], _rows(n_clips=11, rows_per_clip=3)
    else:
        heads = [_head(L, k == 'pooled', s, parts=parts) for s, k in enumerate(('plain', 'pooled') if kind == 'both' else (kind,))]
        fr = _rows()
    assert _call(L, heads, fr) == 0
    # several candidates per sample (T = 3): rows_per_clip = T (R + 1), a third of the clips
    if kind != 'ungrouped':
        assert _call(L, heads, _rows(n_clips=N // 3, rows_per_clip=3 * (R + 1))) == 0


def test_setter_is_consumed_by_the_call_that_reads_it(dry):
    """a setter that makes its call fail is gone for the next one; NULL switches it off; an un-armed call is what it was"""
    L = dry
    head = [_head(L, False, 0)]
    bad = _rows(n_clips=N - 1)
    assert _call(L, head, bad) == EINVAL
    assert _call(L, head, None) == 0                      # the same head, no setter: the per-batch q32b block, accepted
    assert _call(L, head) == 0 and _call(L, head, None) == 0
    # consumed by a call that succeeds too: the second call would refuse the fp32 block if it still saw the setter
    fp32 = [_head(L, False, 0, x_q32=0, planes_bytes=L.lirec_planes_bytes(N, sum(DIMS), J, 0))]
    assert _call(L, head) == 0 and _call(L, fp32, None) == 0
    assert _call(L, fp32) == EINVAL and _call(L, fp32, None) == 0
    # NULL: off
    assert L.lirec_set_feature_rows(C.byref(bad)) == 0 and L.lirec_set_feature_rows(None) == 0
    assert _call(L, head, None) == 0
    # the backward takes no setter and consumes none: a forward after it still sees it
    assert L.lirec_set_feature_rows(C.byref(bad)) == 0
    assert L.lirec_embed_bwd(None, None) == EINVAL
    assert _call(L, head, None) == EINVAL and _call(L, head, None) == 0


SRC, DST = _addr(80), _addr(81)
BAD_WRITE = {
    'null src': dict(src=None), 'null dst': dict(dst=None), 'src_f64 = 2': dict(f64=2), 'src_f64 < 0': dict(f64=-1),
    'rows < 0': dict(rows=-1), 'cols 0': dict(cols=0), 'cols no multiple of 32': dict(cols=6900), 'ld_src < cols': dict(ld=6911),
    'dst_row0 < 0': dict(row0=-1), 'dst_rows no multiple of 32': dict(dst_rows=1000), 'dst_rows 0': dict(dst_rows=0),
    'rows past the end': dict(row0=1000, rows=25), 'row0 past the end': dict(row0=1025, rows=0),
    'dst_rows over the limit': dict(dst_rows=1 << 31), 'dst misaligned': dict(dst=DST + 128), 'src misaligned for fp32': dict(src=SRC + 2),
    'src misaligned for float64': dict(src=SRC + 4, f64=1),
}


def _write(L, **kw):
    a = dict(src=SRC, f64=0, ld=6912, rows=19, cols=6912, dst=DST, row0=5, dst_rows=1024)
    a.update(kw)
    return L.lirec_q32b_write_rows(a['src'], a['f64'], a['ld'], a['rows'], a['cols'], a['dst'], a['row0'], a['dst_rows'], None)


@pytest.mark.parametrize('what', sorted(BAD_WRITE))
def test_write_rows_refuses_before_any_device_call(lib, what):
    assert _write(lib, **BAD_WRITE[what]) == EINVAL, what


def test_write_rows_with_nothing_to_do_launches_nothing(lib):
    assert _write(lib, rows=0) == 0 and _write(lib, rows=0, row0=1024) == 0


def test_write_rows_accepts_under_the_dry_run(dry):
    L = dry
    assert _write(L) == 0 and _write(L, f64=1) == 0 and _write(L, row0=1005) == 0 and _write(L, src=SRC + 4) == 0
    assert _write(L, dst_rows=_lib.FEATURE_ROWS_MAX, row0=_lib.FEATURE_ROWS_MAX - 19) == 0


def _fields(n, over=None):
    arr = (_lib.CollateField * max(n, 1))()
    for f in range(n):
        arr[f].src, arr[f].row_bytes, arr[f].dst = SRC + 0x100000 * f, (1, 808, 4, 8, 13)[f % 5], DST + 0x100000 * f + f
    for f, o in (over or {}).items():
        for k, v in o.items():
            setattr(arr[f], k, v)
    return arr


BAD_FIELDS = {
    'B < 0': lambda L: L.lirec_collate_fields(IDS, -1, _fields(2), 2, None),
    'nf < 0': lambda L: L.lirec_collate_fields(IDS, 5, _fields(2), -1, None),
    'nf over the limit': lambda L: L.lirec_collate_fields(IDS, 5, _fields(17), 17, None),
    'null fields': lambda L: L.lirec_collate_fields(IDS, 5, None, 2, None),
    'null ids': lambda L: L.lirec_collate_fields(None, 5, _fields(2), 2, None),
    'ids misaligned': lambda L: L.lirec_collate_fields(IDS + 2, 5, _fields(2), 2, None),
    'ids misaligned, B = 0': lambda L: L.lirec_collate_fields(IDS + 2, 0, _fields(2), 2, None),
    'row_bytes 0': lambda L: L.lirec_collate_fields(IDS, 5, _fields(3, {1: dict(row_bytes=0)}), 3, None),
    'row_bytes < 0, B = 0': lambda L: L.lirec_collate_fields(IDS, 0, _fields(3, {2: dict(row_bytes=-8)}), 3, None),
    'null field src': lambda L: L.lirec_collate_fields(IDS, 5, _fields(3, {0: dict(src=None)}), 3, None),
    'null field dst': lambda L: L.lirec_collate_fields(IDS, 5, _fields(3, {2: dict(dst=None)}), 3, None),
}


@pytest.mark.parametrize('what', sorted(BAD_FIELDS))
def test_collate_fields_refuses_before_any_device_call(lib, what):
    assert BAD_FIELDS[what](lib) == EINVAL, what


def test_collate_fields_empty_batches_launch_nothing(lib):
    """B == 0: the checks come first, then no launch (NULL pointers are fine without rows to move), as lirec_collate_resident"""
    L = lib
    assert L.lirec_collate_fields(None, 0, _fields(2, {0: dict(src=None, dst=None)}), 2, None) == 0
    assert L.lirec_collate_fields(IDS, 5, None, 0, None) == 0


def test_collate_fields_is_one_recorded_launch(dry):
    L = dry
    assert L.lirec_collate_fields(IDS, 5, _fields(16), 16, None) == 0 and L.lirec_collate_fields(IDS, 1, _fields(1), 1, None) == 0
    assert L.lirec_record_begin() == 0
    h = C.c_void_p()
    rc = L.lirec_collate_fields(IDS, 64, _fields(12), 12, None)
    assert L.lirec_record_end(C.byref(h)) == 0
    n = L.lirec_cmdlist_size(h)
    assert L.lirec_cmdlist_destroy(h) == 0
    assert (rc, n) == (0, 1)


@pytest.mark.parametrize('rpc,stride,group,off', [(1, 0, 0, 0), (7, 0, 0, 0), (19, 19, 1, 0), (19, 19, 18, 1), (7 * 19, 19, 1, 0), (7 * 19, 19, 18, 1),
                                                  (5 * 3, 3, 2, 1), (9, 3, 1, 2), (11, 11, 10, 1)])
def test_storage_row_mapping_against_brute_force(rpc, stride, group, off):
    """lirec_rowsel then lirec_feature_rows, restated with numpy (blockstore.storage_rows), against the block built by brute force:
    the store's rows numbered 0, 1, 2, ..., the batch's block assembled sample by sample, the selector applied to it"""
    rng = np.random.default_rng(rpc * 131 + group)
    n_store, ids = 23, np.array([22, 3, 3, 0, 17, 9, 22], dtype=np.int64)      # out of order, the last sample, duplicates
    store = np.arange(n_store * rpc, dtype=np.int64)
    block = np.concatenate([store[i * rpc:(i + 1) * rpc] for i in ids])           # the per-batch block, by value = its storage row
    if group == 0:
        logical = np.arange(len(ids) * rpc)
        phys = logical
    else:
        n_groups = len(ids) * rpc // stride
        logical = rng.permutation(n_groups * group)
        phys = logical // group * stride + logical % group + off
    got = BS.storage_rows(ids, rpc, phys)
    assert np.array_equal(got, block[phys])
    # the header's formula, element by element
    for p, g in zip(phys.tolist(), got.tolist()):
        assert g == int(ids[p // rpc]) * rpc + p % rpc and 0 <= g < n_store * rpc


KINDS = {'modalties': {}, 'int_rels': dict(R=4), 'int_ch': dict(T=3), 'int_rel_ch': dict(T=3, R=4)}


class _Holder:
    """a dataset with a block store that is a plan only (no device)"""

    def __init__(self, ds):
        self.ds, self.block_store = ds, BS.BlockStore(ds, 'cuda', upload=False)

    def __len__(self):
        return len(self.ds)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_loader_layout_equals_default_collate(kind):
    ds = SyntheticMixedFeaturesDataset(kind, 6, seed=3, **SMALL_DIMS, **KINDS[kind])
    h = _Holder(ds)
    st = h.block_store
    assert st.data is None and st.tables is None
    want = collate([ds[i] for i in (4, 1, 1)])
    f = want.pop('features')
    assert st.n == 6 and st.feature_shape == tuple(f.shape[1:]) and st.D == f.shape[-1] == 128
    assert st.rows_per_clip == int(np.prod(f.shape[1:-1], dtype=np.int64)) and st.store_rows == (6 * st.rows_per_clip + 31) // 32 * 32
    assert st.keys == list(ds[0].keys())
    loader = BlockLoader(h, batch_size=3)
    layout, nbytes = loader.layout(3)
    assert [k for k, _, _, _, _ in layout] == list(want) + [BS.IDS_KEY]
    end = 0
    for k, off, nb, dt, shape in layout:
        assert off % 256 == 0 and off >= end
        end = off + nb
        if k == BS.IDS_KEY:
            assert (dt, shape, nb) == (np.dtype(np.int32), (3,), 12)
            continue
        assert torch.from_numpy(np.zeros(0, dtype=dt)).dtype == want[k].dtype, k
        assert shape == tuple(want[k].shape) and nb == want[k].numel() * want[k].element_size(), k
    assert nbytes >= end and nbytes % 256 == 0
    assert st.nbytes == st.store_rows * st.D * 4 + 6 * (sum(want[k][0].numel() * want[k].element_size() for k in want) + 4)
    assert loader.layout(3) is loader.layout(3) and loader.layout(2)[0] != layout
    assert len(loader) == 2 and loader.epoch_ids() == [[0, 1, 2], [3, 4, 5]]


def _samples(n=3, D=64, lead=(2,), **extra):
    return [dict({'features': np.full(lead + (D,), float(i)), 'labels': i}, **{k: v(i) for k, v in extra.items()}) for i in range(n)]


def test_block_store_refusals(monkeypatch):
    E = _lib.LirecError
    with pytest.raises(E, match='ragged'):
        s = _samples()
        s[2]['features'] = np.zeros((3, 64))
        BS.BlockStore(s, 'cuda')
    with pytest.raises(E, match='multiple of 32'):
        BS.BlockStore(_samples(D=48), 'cuda')
    with pytest.raises(E, match='not numeric'):
        BS.BlockStore(_samples(name=lambda i: 'clip%d' % i), 'cuda')
    with pytest.raises(E, match='cannot be stacked'):
        BS.BlockStore(_samples(mask=lambda i: np.zeros(2 + i)), 'cuda')
    with pytest.raises(E, match='float32 / float64'):
        s = _samples()
        s[0]['features'] = np.zeros((2, 64), dtype=np.int64)
        BS.BlockStore(s, 'cuda')
    with pytest.raises(E, match='row limit'):
        BS.BlockStore(_samples(), 'cuda', capacity=(_lib.FEATURE_ROWS_MAX + 1) // 2)
    assert BS.BlockStore(_samples(), 'cuda', capacity=_lib.FEATURE_ROWS_MAX // 2 - 1, upload=False).store_rows <= _lib.FEATURE_ROWS_MAX
    with pytest.raises(E, match='slots'):
        BS.BlockStore(_samples(), 'cuda', capacity=2)
    with pytest.raises(E, match='lives on a GPU'):
        BS.BlockStore(_samples(), 'cpu')
    # a store larger than the free memory minus the stated margin: refused before any device memory is asked for
    need = BS.BlockStore(_samples(), 'cuda', upload=False).nbytes
    monkeypatch.setattr(BS, '_free_bytes', lambda device: need + BS.MARGIN_BYTES - 1)
    with pytest.raises(E, match='MARGIN_BYTES'):
        BS.BlockStore(_samples(), 'cuda')
    assert BS.MARGIN_BYTES == 1 << 30
