"""The recorded evaluation / prediction step without a GPU: the three new exports (declared, bound, present; ABI still 124 and every
struct size index as before), every LIREC_EINVAL of their contracts with and without the library's host-side dry run on fake
aligned addresses, ``opt.record_eval``'s default, when ``EvalStepper`` is asked for at all, and ``BlockLoader``'s host account of
its device cursor over a mixed sequence of in-list and eager batches (a store that is a plan only, the cursor word on the host)."""
import ctypes as C
import os
import re

import pytest

from lirec_amd import _lib, blockstore as BS, config, graph
from lirec_amd.config import opt
from lirec_amd.data import SyntheticMixedFeaturesDataset
from lirec_amd.loader import BlockLoader, ThreadedLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
NEW = ('lirec_predict_clips_at', 'lirec_rows_copy_at', 'lirec_scalar_accumulate')


def _addr(i, sub=0):
    return 0x10000000 + 0x4000000 * i + 0x400000 * sub


INTS, RELS, MEM, CUR, SRC, DST, ACC, VAL = (_addr(i) for i in (50, 51, 52, 61, 80, 81, 82, 83))
OUT = {k: _addr(53, j) for j, k in enumerate(('trk', 'cls', 'rel', 'score', 'trk_score', 'top_cls', 'top_cls_p', 'top_rel', 'top_rel_p', 'flags'))}


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


def _pargs(**over):
    a = _lib.PredictArgs()
    a.ints, a.ld_ints, a.rels, a.ld_rels, a.mem = INTS, 101, RELS, 15, MEM
    for k, v in OUT.items():
        setattr(a, k, v)
    a.B, a.T, a.C, a.NR, a.K, a.loader_types = 5, 4, 101, 15, 5, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_exports_are_declared_bound_and_present_and_the_abi_did_not_move():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    for name in NEW + ('lirec_predict_clips', 'lirec_counter_add'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert L.lirec_abi_sizeof(15) == C.sizeof(_lib.PredictArgs) == 144       # the struct both prediction exports take: unchanged
    assert [L.lirec_abi_sizeof(i) for i in range(40)] == ABI_SIZES


# lirec_abi_sizeof(0 .. 39) as the library answered before these exports were added (-1: no struct at that index)
ABI_SIZES = [440, 448, 240, 32, 12, 104, 64, 144, 120, 144, 24, 32, 24, 80, -1, 144, -1, 496, -1, 24, -1, 24, -1, 24] + [-1] * 16


PREDICT_BAD = {
    'null cursor': lambda L: L.lirec_predict_clips_at(C.byref(_pargs()), None, None),
    'cursor misaligned by 4': lambda L: L.lirec_predict_clips_at(C.byref(_pargs()), CUR + 4, None),
    'cursor misaligned by 1': lambda L: L.lirec_predict_clips_at(C.byref(_pargs()), CUR + 1, None),
    'null struct': lambda L: L.lirec_predict_clips_at(None, CUR, None),
    # ... and the cases of lirec_predict_clips, one of each kind
    'null ints': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(ints=None)), CUR, None),
    'null trk': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(trk=None)), CUR, None),
    'B < 0': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(B=-1)), CUR, None),
    'T < 1': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(T=0)), CUR, None),
    'K over the limit': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(K=_lib.PREDICT_MAX_K + 1)), CUR, None),
    'ld_ints < C': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(ld_ints=100)), CUR, None),
    'rels with NR < 1': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(NR=0)), CUR, None),
    'ld_rels < NR': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(ld_rels=14)), CUR, None),
    'misaligned cls': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(cls=OUT['cls'] + 2)), CUR, None),
    'score not 8-byte aligned': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(score=OUT['score'] + 4)), CUR, None),
    'mem not 8-byte aligned under loader_types': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(mem=MEM + 4)), CUR, None),
    'a clip over the LDS limit': lambda L: L.lirec_predict_clips_at(C.byref(_pargs(T=343)), CUR, None),
}

ROWS_BAD = {
    'null src': lambda L: L.lirec_rows_copy_at(None, 15, 5, 15, DST, 15, CUR, None),
    'null dst': lambda L: L.lirec_rows_copy_at(SRC, 15, 5, 15, None, 15, CUR, None),
    'null cursor': lambda L: L.lirec_rows_copy_at(SRC, 15, 5, 15, DST, 15, None, None),
    'cursor misaligned': lambda L: L.lirec_rows_copy_at(SRC, 15, 5, 15, DST, 15, CUR + 4, None),
    'src misaligned': lambda L: L.lirec_rows_copy_at(SRC + 2, 15, 5, 15, DST, 15, CUR, None),
    'dst misaligned': lambda L: L.lirec_rows_copy_at(SRC, 15, 5, 15, DST + 1, 15, CUR, None),
    'cols 0': lambda L: L.lirec_rows_copy_at(SRC, 15, 5, 0, DST, 15, CUR, None),
    'cols < 0': lambda L: L.lirec_rows_copy_at(SRC, 15, 5, -3, DST, 15, CUR, None),
    'rows < 0': lambda L: L.lirec_rows_copy_at(SRC, 15, -1, 15, DST, 15, CUR, None),
    'ld_src < cols': lambda L: L.lirec_rows_copy_at(SRC, 14, 5, 15, DST, 15, CUR, None),
    'ld_dst < cols': lambda L: L.lirec_rows_copy_at(SRC, 15, 5, 15, DST, 14, CUR, None),
}

ACC_BAD = {
    'null acc': lambda L: L.lirec_scalar_accumulate(None, 0, VAL, None),
    'null v': lambda L: L.lirec_scalar_accumulate(ACC, 1, None, None),
    'fp32 acc misaligned': lambda L: L.lirec_scalar_accumulate(ACC + 2, 0, VAL, None),
    'float64 acc on a 4-byte boundary': lambda L: L.lirec_scalar_accumulate(ACC + 4, 1, VAL, None),
    'v misaligned': lambda L: L.lirec_scalar_accumulate(ACC, 0, VAL + 1, None),
}


@pytest.mark.parametrize('what', sorted(PREDICT_BAD))
def test_predict_clips_at_refuses_before_any_device_call(lib, what):
    assert PREDICT_BAD[what](lib) == EINVAL, what


@pytest.mark.parametrize('what', sorted(ROWS_BAD))
def test_rows_copy_at_refuses_before_any_device_call(lib, what):
    assert ROWS_BAD[what](lib) == EINVAL, what


@pytest.mark.parametrize('what', sorted(ACC_BAD))
def test_scalar_accumulate_refuses_before_any_device_call(lib, what):
    assert ACC_BAD[what](lib) == EINVAL, what


def test_accepted_calls_under_the_dry_run_are_one_recorded_launch_each(dry):
    L = dry
    assert L.lirec_predict_clips_at(C.byref(_pargs(B=0)), CUR, None) == 0                   # no clip: nothing to launch
    assert L.lirec_rows_copy_at(SRC, 15, 0, 15, DST, 15, CUR, None) == 0                    # no row: nothing to launch
    assert L.lirec_scalar_accumulate(ACC + 4, 0, VAL, None) == 0                            # an fp32 accumulator needs 4 bytes only
    assert L.lirec_record_begin() == 0
    h = C.c_void_p()
    rcs = [L.lirec_predict_clips_at(C.byref(_pargs()), CUR, None),
           L.lirec_predict_clips_at(C.byref(_pargs(rels=None, mem=None, T=1, cls=None, score=None, flags=None, loader_types=0)), CUR, None),
           L.lirec_rows_copy_at(SRC, 19 * 15, 5, 15, DST, 15, CUR, None),                  # a strided source
           L.lirec_rows_copy_at(SRC, 101, 1, 101, DST, 101, CUR, None),
           L.lirec_scalar_accumulate(ACC, 0, VAL, None), L.lirec_scalar_accumulate(ACC, 1, VAL, None),
           L.lirec_predict_clips_at(C.byref(_pargs(B=0)), CUR, None), L.lirec_rows_copy_at(SRC, 15, 0, 15, DST, 15, CUR, None),
           L.lirec_counter_add(CUR, (C.c_int64 * 1)(5), 1, None)]                          # the output cursor's move: the existing export
    assert L.lirec_record_end(C.byref(h)) == 0
    n = L.lirec_cmdlist_size(h)
    assert L.lirec_cmdlist_destroy(h) == 0
    assert rcs == [0] * 9 and n == 7


def test_flag_defaults_to_off_and_the_stepper_is_asked_for_by_the_flag_alone():
    config.recipe('int_rels')
    assert opt.record_eval is False and config.defaults()['record_eval'] is False
    ds = SyntheticMixedFeaturesDataset('int_rels', 6, seed=3, R=4, text_dim=32, visual_dim=32, track_dim=32)
    block, other = BlockLoader(_Holder(ds), batch_size=3, device='cpu'), ThreadedLoader(ds, batch_size=3)
    assert not graph.EvalStepper.wanted(block) and not graph.EvalStepper.wanted(other)
    try:
        opt.record_eval = True
        assert graph.EvalStepper.wanted(block) and graph.EvalStepper.wanted(block, world=1)
        assert not graph.EvalStepper.wanted(block, world=2)           # one process only
        assert not graph.EvalStepper.wanted(other)                    # a block store only
    finally:
        opt.record_eval = False


class _Holder:
    """a dataset with a block store that is a plan only (no device)"""

    def __init__(self, ds):
        self.ds, self.block_store = ds, BS.BlockStore(ds, 'cuda', upload=False)

    def __len__(self):
        return len(self.ds)


def test_cursor_account_over_a_mixed_sequence_of_in_list_and_eager_batches(monkeypatch):
    """13 samples in batches of 3: [eager, eager (the list is recorded on it), in-list, in-list, eager singleton], then a second
    epoch [in-list x 4, eager singleton], a lost cursor in the middle.  The cursor word lives on the host here and the 'list' is
    played by the test: it must find the offset of the batch it is about to draw, every time."""
    ds = SyntheticMixedFeaturesDataset('int_rels', 13, seed=3, R=4, text_dim=32, visual_dim=32, track_dim=32)
    loader = BlockLoader(_Holder(ds), batch_size=3, device='cpu')
    loader.stable_ids = True
    collated = []
    monkeypatch.setattr(BlockLoader, 'collate_ids', lambda self, ids, B: collated.append(ids.tolist()) or {'_layout': self.layout(B)[0], '_dev_blob': 'own'})
    monkeypatch.setattr(BlockLoader, '_batch_of', lambda self, layout, blob, B: ({'_layout': layout, '_dev_blob': blob}, []))
    lay3, blob = loader.layout(3)[0], object()
    drawn = []

    def the_list_runs():
        """what collate_at's two launches do on the device: read the ids at the word, move the word on"""
        at = int(loader.cursor)
        drawn.append(loader.ids_base[at:at + 3].tolist())
        loader.cursor.add_(3)

    for epoch in range(2):
        for i, batch in enumerate(loader):
            at, B, in_list = loader._last
            assert (at, B) == (3 * i, 3 if i < 4 else 1)
            if epoch == 0 and i == 1:
                # the recording: the cursor to this batch, the draw runs (collate_at: launches + advanced), the buffer is bound
                assert not in_list and loader.can_draw_last_in_list()
                loader.cursor_to_last()
                assert int(loader.cursor) == 3
                the_list_runs()
                loader._cursor.advanced(3)
                loader.bind(lay3, blob, in_list=True)
            elif in_list:
                assert batch['_dev_blob'] is blob and loader.last_in_list
                assert int(loader.cursor) == at == loader._cursor.at - 3, (epoch, i)
                the_list_runs()
                if epoch == 1 and i == 1:
                    loader.cursor_lost()          # (a recording elsewhere failed half-way: the word is written again)
                    loader.cursor.fill_(-7)
            else:
                assert batch['_dev_blob'] == 'own' and not loader.last_in_list
    assert drawn == [[3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    assert collated == [[0, 1, 2], [3, 4, 5], [12], [12]]
    assert loader.n_in_list == 6 and int(loader.cursor) == 12 == loader._cursor.at
    # a batch left to a list that will not run is collated after all, and the account is void until the next in-list batch
    loader.bind(lay3, blob, in_list=True)
    it = iter(loader)
    b = next(it)
    assert loader.last_in_list and b['_dev_blob'] is blob
    b = loader.materialise(b)
    assert b['_dev_blob'] == 'own' and collated[-1] == [0, 1, 2] and not loader.last_in_list and loader._cursor.at is None
    next(it)
    assert loader.last_in_list and int(loader.cursor) == 3
