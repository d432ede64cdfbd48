"""The recorded step over block-store batches without a GPU: the new export lirec_collate_fields_at (declared, bound, present; ABI
still 124 and every struct size index as before), every LIREC_EINVAL of its contract with and without the library's host-side dry
run on fake aligned addresses, ``opt.record_block_store``, ``train._recordable``'s second form condition by condition on stub
batches, and ``train._flag_key`` across the flag's values."""
import ctypes as C
import os
import re

import pytest

from lirec_amd import _lib, config, ops, parallel, train
from lirec_amd.config import opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL


def _addr(i, sub=0):
    return 0x10000000 + 0x4000000 * i + 0x400000 * sub


IDS, CUR, SRC, DST = _addr(60), _addr(61), _addr(80), _addr(81)


@pytest.fixture(params=[False, True], ids=['plain', 'dry-run'])
def lib(request):
    """the refusals: with the dry run and without it (a call that got past the checks would then reach the HIP runtime)"""
    L = _lib.lib()
    if request.param:
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_debug_set(0, -1) == 0


@pytest.fixture
def dry():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def _fields(n, over=None):
    arr = (_lib.CollateField * max(n, 1))()
    for f in range(n):
        arr[f].src, arr[f].row_bytes, arr[f].dst = SRC + 0x100000 * f, (1, 808, 4, 8, 13)[f % 5], DST + 0x100000 * f + f
    for f, o in (over or {}).items():
        for k, v in o.items():
            setattr(arr[f], k, v)
    return arr


def test_export_is_declared_bound_and_present_and_the_abi_did_not_move():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    for name in ('lirec_collate_fields_at', 'lirec_collate_fields', 'lirec_counter_add'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert int(re.search(r'#define LIREC_COLLATE_MAX_FIELDS (\d+)', hdr).group(1)) == _lib.COLLATE_MAX_FIELDS == 16
    # the indices the block store's own test pins, and every index's answer against the ctypes mirror the package checks at load
    assert L.lirec_abi_sizeof(21) == C.sizeof(_lib.FeatureRows) == 24 and L.lirec_abi_sizeof(23) == C.sizeof(_lib.CollateField) == 24
    assert L.lirec_abi_sizeof(0) == C.sizeof(_lib.EmbedFwdArgs) and L.lirec_abi_sizeof(17) == C.sizeof(_lib.CollateArgs)
    assert L.lirec_abi_sizeof(20) == -1 and L.lirec_abi_sizeof(22) == -1 and L.lirec_abi_sizeof(24) == -1
    assert [L.lirec_abi_sizeof(i) for i in range(40)] == ABI_SIZES


# lirec_abi_sizeof(0 .. 39) as the library answered before this export was added (-1: no struct at that index)
ABI_SIZES = [440, 448, 240, 32, 12, 104, 64, 144, 120, 144, 24, 32, 24, 80, -1, 144, -1, 496, -1, 24, -1, 24, -1, 24] + [-1] * 16


BAD = {
    'null ids_base': lambda L: L.lirec_collate_fields_at(None, CUR, 5, _fields(2), 2, None),
    'ids_base misaligned': lambda L: L.lirec_collate_fields_at(IDS + 2, CUR, 5, _fields(2), 2, None),
    'null cursor': lambda L: L.lirec_collate_fields_at(IDS, None, 5, _fields(2), 2, None),
    'cursor misaligned by 4': lambda L: L.lirec_collate_fields_at(IDS, CUR + 4, 5, _fields(2), 2, None),
    'cursor misaligned by 1': lambda L: L.lirec_collate_fields_at(IDS, CUR + 1, 5, _fields(2), 2, None),
    'B = 0': lambda L: L.lirec_collate_fields_at(IDS, CUR, 0, _fields(2), 2, None),
    'B < 0': lambda L: L.lirec_collate_fields_at(IDS, CUR, -1, _fields(2), 2, None),
    'nf over the limit': lambda L: L.lirec_collate_fields_at(IDS, CUR, 5, _fields(17), 17, None),
    'nf < 0': lambda L: L.lirec_collate_fields_at(IDS, CUR, 5, _fields(2), -1, None),
    'null fields': lambda L: L.lirec_collate_fields_at(IDS, CUR, 5, None, 2, None),
    'row_bytes 0': lambda L: L.lirec_collate_fields_at(IDS, CUR, 5, _fields(3, {1: dict(row_bytes=0)}), 3, None),
    'row_bytes < 0': lambda L: L.lirec_collate_fields_at(IDS, CUR, 5, _fields(3, {2: dict(row_bytes=-8)}), 3, None),
    'null field src': lambda L: L.lirec_collate_fields_at(IDS, CUR, 5, _fields(3, {0: dict(src=None)}), 3, None),
    'null field dst': lambda L: L.lirec_collate_fields_at(IDS, CUR, 5, _fields(3, {2: dict(dst=None)}), 3, None),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_collate_fields_at_refuses_before_any_device_call(lib, what):
    assert BAD[what](lib) == EINVAL, what


def test_collate_fields_at_accepted_under_the_dry_run_is_one_recorded_launch(dry):
    L = dry
    assert L.lirec_collate_fields_at(IDS, CUR, 5, _fields(16), 16, None) == 0
    assert L.lirec_collate_fields_at(IDS, CUR, 1, _fields(1), 1, None) == 0
    assert L.lirec_collate_fields_at(IDS, CUR, 5, None, 0, None) == 0          # no field: nothing to launch
    assert L.lirec_record_begin() == 0
    h = C.c_void_p()
    rc = L.lirec_collate_fields_at(IDS, CUR, 64, _fields(12), 12, None)
    inc = (C.c_int64 * 1)(64)
    rc2 = L.lirec_counter_add(CUR, inc, 1, None)                               # the cursor's advance: the existing export
    assert L.lirec_record_end(C.byref(h)) == 0
    n = L.lirec_cmdlist_size(h)
    assert L.lirec_cmdlist_destroy(h) == 0
    assert (rc, rc2, n) == (0, 0, 2)


def test_flag_defaults_to_off_and_is_part_of_the_flag_key():
    config.recipe('int_rels')
    assert opt.record_block_store == ''
    keys = []
    try:
        for v in ('', 'bind', 'list'):
            opt.record_block_store = v
            keys.append(train._flag_key())
    finally:
        opt.record_block_store = ''
    assert len(set(keys)) == 3


class _Params:
    def __init__(self, cuda):
        self.is_cuda = cuda


class _Model:
    """what ``_recordable`` asks of a model: the hot path's forward and where its parameters live"""

    def __init__(self, cuda=True):
        self._cuda = cuda

    def _run_forward(self):
        pass

    def flat_params(self):
        return _Params(self._cuda)


def _block(planes=2, with_ids=True):
    f = ops.Q32Block.__new__(ops.Q32Block)      # (no device here: the fields ``_recordable`` reads, set by hand)
    f.planes, f.clip_ids = planes, (object() if with_ids else None)
    return f


def _stub_batch(**over):
    b = {'features': _block(), 'labels': None, '_layout': [('labels', 0, 40, None, (5,))], '_dev_blob': object()}
    b.update(over)
    return {k: v for k, v in b.items() if v is not _DROP}


_DROP = object()
# one condition of the block-store form each: (what to change, how)
CONDITIONS = {
    'flag off': dict(flag=''),
    'world 2': dict(world=2),
    'no _dev_blob': dict(batch=dict(_dev_blob=_DROP)),
    'no _layout': dict(batch=dict(_layout=_DROP)),
    'features not a Q32Block': dict(batch=dict(features=object())),
    'features without clip_ids': dict(batch=dict(features=_block(with_ids=False))),
    'one-plane features': dict(batch=dict(features=_block(planes=1))),
    'layer1_planes off': dict(planes=False),
    'gemm mode 0': dict(mode=0),
    'gemm mode 1': dict(mode=1),
    'gemm mode 3': dict(mode=3),
    'parameters on the host': dict(model=_Model(cuda=False)),
    'not a hot-path model': dict(model=object()),
    'recorded_training off': dict(recorded=False),
}


@pytest.fixture
def scene(monkeypatch):
    """flags and GEMM mode a block-store batch is recordable under; everything put back afterwards"""
    config.recipe('int_rels')
    L = _lib.lib()
    mode = L.lirec_get_gemm_mode()
    assert L.lirec_set_gemm_mode(2) == 0
    opt.layer1_planes, opt.recorded_training = True, True
    try:
        yield monkeypatch
    finally:
        opt.record_block_store = ''
        assert L.lirec_set_gemm_mode(mode) == 0


@pytest.mark.parametrize('flag', ['bind', 'list'])
def test_recordable_accepts_a_block_store_batch_under_the_flag(scene, flag):
    opt.record_block_store = flag
    assert train._recordable(_Model(), _stub_batch()) is True


@pytest.mark.parametrize('what', sorted(CONDITIONS))
def test_recordable_refuses_when_one_condition_fails(scene, what):
    c = CONDITIONS[what]
    opt.record_block_store = c.get('flag', 'bind')
    opt.layer1_planes = c.get('planes', True)
    opt.recorded_training = c.get('recorded', True)
    if 'mode' in c:
        assert _lib.lib().lirec_set_gemm_mode(c['mode']) == 0
    if 'world' in c:
        scene.setattr(parallel, 'world_info', lambda group=None: (0, c['world']))
    assert train._recordable(c.get('model', _Model()), _stub_batch(**c.get('batch', {}))) is False, what


def test_piece_store_form_is_what_it_was(scene):
    """the first form does not read the new flag"""
    b = {'piece_store': object(), '_dev_blob': object(), '_layout': []}
    opt.pieces_q32b, opt.pieces_gather = True, True
    assert train._recordable(_Model(), b) is True
    opt.pieces_q32b = False
    assert train._recordable(_Model(), b) is False


def test_flag_values_outside_the_three_are_refused(scene):
    for bad in ('yes', 'List', 'BIND'):
        opt.record_block_store = bad
        with pytest.raises(ValueError, match='record_block_store'):
            train._recordable(_Model(), _stub_batch())
