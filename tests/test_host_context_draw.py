"""Train-mode context sampling without a GPU: the draw rule (``features.draw_context``) against an independent restatement, the
package's Philox, ``PiecesDataset(context_draw='random')`` against the strided dataset and against the lists it draws from, the
distribution of a draw, the refusals, the C ABI's argument checks, and the default mode left as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import context_draw_cases as DC
from lirec_amd import _lib, features as F
from lirec_amd._lib import LirecError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
R = DC.WORLD_R
SEED = 0x5eed00000007


# ---- the rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,k', DC.RUNS)
def test_draw_context_equals_the_restatement(name, k):
    case = DC.CASES[name]
    seed, epoch = case['runs'][k]
    table = DC.sentinel_table(case)
    out = F.draw_context(case['slot_dst'], case['slot_off'], case['pool_rows'], table, case['R'], seed, epoch)
    assert out is table                                        # in place
    want = DC.restate(case, seed, epoch)
    assert np.array_equal(table, want)
    assert (table[~DC.slot_rows_mask(case)] == DC.SENTINEL).all()
    # the epoch is a 32-bit counter word
    again = F.draw_context(case['slot_dst'], case['slot_off'], case['pool_rows'], DC.sentinel_table(case), case['R'], seed, epoch + (1 << 32))
    assert np.array_equal(again, want)


def test_the_packages_philox_known_answers():
    """the two vectors of tests/test_oracle_golden.py::test_philox_known_answer (Random123 kat_vectors)"""
    z = np.zeros(1, np.uint32)
    assert [int(x[0]) for x in F.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = np.full(1, 0xFFFFFFFF, np.uint32)
    assert [int(x[0]) for x in F.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_an_empty_pool_draws_nothing():
    t = np.full((2, 3, 4, 3), 5, dtype=np.int32)
    F.draw_context(np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros((0, 3), np.int32), t, 3, 1, 2)
    assert (t == 5).all()


# ---- the dataset against the reference's semantics ------------------------------------------------------------------------
_memo = {}


def world():
    if 'world' not in _memo:
        _memo['world'] = F.synthetic_world(**DC.WORLD)
    return _memo['world']


def strided():
    if 'strided' not in _memo:
        _memo['strided'] = F.PiecesDataset(world(), R, pin_memory=False)
    return _memo['strided']


def full_lists():
    """{(sample, candidate): [L, 3] rows} of every over-long list WHOLE, by another way than the dataset's pool: the same world
    assembled with room for the longest list (R' = 19), where ``assemble_sample`` + ``world_rows`` write every list out"""
    if 'full' not in _memo:
        big = F.PiecesDataset(world(), 19, pin_memory=False)
        rows, mask = big._stacked['index_rows'], big._stacked['rels_mask']
        small = strided()._stacked
        out = {}
        for s in range(len(big)):
            for c in range(F.T_MAX):
                L = int(mask[s, c].sum())
                # (a context candidate: rows 1.. differ from row 0's clip; a tiled candidate repeats one row and has mask[0] only)
                if L > R and int(small['rels_mask'][s, c].sum()) == R:
                    assert L <= 19
                    out[(s, c)] = rows[s, c, 1:1 + L].copy()
        _memo['full'] = out
    return _memo['full']


def random_ds(seed=SEED, **kw):
    return F.PiecesDataset(world(), R, pin_memory=False, context_draw='random', context_seed=seed, **kw)


def test_the_world_has_the_slots_counted_on():
    w, full = world(), full_lists()
    assert len(w.interactions) == 72
    rel_lists, none_lists, _ = w.context_lists(R)
    long = [l for l in list(rel_lists.values()) + list(none_lists.values()) if len(l) > R]
    assert len(long) == 19 and max(len(l) for l in long) == 19
    assert len(full) >= 10
    ds = random_ds()
    # the pool is those lists, slot for slot and entry for entry
    assert ds.slot_dst.dtype == np.int32 and ds.slot_off.dtype == np.int32 and ds.pool_rows.dtype == np.int32
    assert ds.slot_dst.shape == (len(full),) and ds.slot_off.shape == (len(full) + 1,) and ds.pool_rows.shape == (int(ds.slot_off[-1]), 3)
    assert sorted(ds.slot_dst.tolist()) == sorted(s * F.T_MAX + c for s, c in full)
    for i, slot in enumerate(ds.slot_dst.tolist()):
        assert np.array_equal(ds.pool_rows[ds.slot_off[i]:ds.slot_off[i + 1]], full[divmod(slot, F.T_MAX)]), slot


def test_random_equals_strided_but_for_rows_drawn_from_the_slots_lists():
    st, ds, full = strided(), random_ds(), full_lists()
    in_slot = np.zeros((len(st), F.T_MAX, R + 1), dtype=bool)
    for s, c in full:
        in_slot[s, c, 1:] = True
    seen = []
    for epoch in (0, 1, 2):
        ds.epoch = epoch
        rows = np.stack([ds[i]['index_rows'] for i in range(len(ds))])
        assert rows.dtype == np.int32 and np.array_equal(rows, ds.epoch_rows()) and np.array_equal(rows, ds._stacked['index_rows'])
        assert np.array_equal(rows[~in_slot], st._stacked['index_rows'][~in_slot])
        for i in range(len(ds)):
            a, b = ds[i], st[i]
            assert 'feature_index' not in a and 'track_keys' not in a and a['_id'] == b['_id'] == i
            for k in F._FIELDS:
                assert np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, (i, k)
        for k in F._FIELDS:
            assert np.array_equal(ds._stacked[k], st._stacked[k]) and ds._stacked[k].dtype == st._stacked[k].dtype, k
        for (s, c), lst in full.items():
            drawn = rows[s, c, 1:]
            # (entries of a list are distinct clips: column 0 names the entry)
            assert len(set(lst[:, 0].tolist())) == len(lst)
            at = [lst[:, 0].tolist().index(v) for v in drawn[:, 0].tolist()]
            assert len(set(at)) == R and np.array_equal(lst[at], drawn), (epoch, s, c)
        seen.append(rows)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # the stored strided table is what it was
    assert np.array_equal(ds._base_rows, st._stacked['index_rows'])


def test_the_same_seed_and_epoch_give_the_same_draw_twice_and_from_a_second_object():
    a, b = random_ds(), random_ds()
    a.epoch = 1
    first = a.epoch_rows().copy()
    a.epoch = 2
    other = a.epoch_rows().copy()
    a.epoch = 1
    b.epoch = 1
    assert np.array_equal(a.epoch_rows(), first) and np.array_equal(b.epoch_rows(), first) and not np.array_equal(other, first)
    c = random_ds(seed=SEED + 1)
    c.epoch = 1
    assert not np.array_equal(c.epoch_rows(), first)
    # the rule itself: the dataset's draw is draw_context over its own pool
    want = F.draw_context(a.slot_dst, a.slot_off, a.pool_rows, strided()._stacked['index_rows'].copy(), R, SEED, 1)
    assert np.array_equal(first, want)


def test_context_seed_defaults_to_opt_seed():
    from lirec_amd import config
    from lirec_amd.config import opt
    try:
        opt.seed = 1234
        assert F.PiecesDataset(world(), R, pin_memory=False, context_draw='random').context_seed == 1234
    finally:
        config.reset()
    with pytest.raises(ValueError):
        F.PiecesDataset(world(), R, pin_memory=False, context_draw='shuffled')


def test_tiled_features_are_the_gather_of_the_drawn_rows():
    ds, tiled = random_ds(), random_ds(emit='tiled')
    assert tiled.collate_fn is None
    for epoch in (0, 2):
        ds.epoch = tiled.epoch = epoch
        rows = ds.epoch_rows()
        for i in range(0, len(ds), 5):
            sm = tiled[i]
            assert 'index_rows' not in sm and sm['features'].dtype == np.float64
            want = F.gather_reference(F.collate(world(), [{**strided()[i], 'index_rows': rows[i]}]))[0].numpy()
            assert np.array_equal(sm['features'], want), (epoch, i)
    assert not np.array_equal(np.stack([tiled[i]['features'] for i in range(len(ds))]),
                              np.stack([F.PiecesDataset(world(), R, emit='tiled')[i]['features'] for i in range(len(ds))]))


def test_host_loaders_read_the_epochs_draw_made_once_under_worker_threads(monkeypatch):
    from lirec_amd.loader import ThreadedLoader
    ds = random_ds()
    calls = []
    real = F.draw_context
    monkeypatch.setattr(F, 'draw_context', lambda *a: (calls.append(a[-1]), real(*a))[1])
    tl = ThreadedLoader(ds, batch_size=5, num_workers=3, collate_fn=ds.collate_fn)
    twin = random_ds()
    for epoch in (0, 1, 1, 2):
        ds.epoch = twin.epoch = epoch
        got = list(tl)
        assert len(got) == 15
        for k, b in enumerate(got):
            idx = list(range(5 * k, min(5 * k + 5, len(ds))))
            want = F.collate(world(), [strided()[i] for i in idx], stacked=dict(strided()._stacked, index_rows=twin.epoch_rows()))
            assert set(b) == set(want)
            for key in want:
                if torch.is_tensor(want[key]):
                    assert torch.equal(b[key], want[key]), (epoch, k, key)
    assert calls == [0, 0, 1, 1, 2, 2]                                            # once per epoch and dataset (ds, then twin)
    # a collate of old samples after the epoch moved on reads the new epoch's rows, not a stale table
    old = [ds[i] for i in range(5)]
    ds.epoch = twin.epoch = 7
    assert torch.equal(ds.collate_fn(old)['feature_index'], twin.collate_fn([twin[i] for i in range(5)])['feature_index'])


def test_a_dataset_with_clip_weights_draws_too():
    w = np.linspace(0.5, 2.0, 72)
    ds, twin = random_ds(clip_weight=w), random_ds()
    ds.epoch = twin.epoch = 3
    assert ds[4][F.CLIP_WEIGHT] == w[4] and np.array_equal(ds[4]['index_rows'], twin.epoch_rows()[4])
    b = ds.collate_fn([ds[i] for i in (4, 9, 70)])
    assert torch.equal(b['feature_index'], twin.collate_fn([twin[i] for i in (4, 9, 70)])['feature_index'])
    assert b[F.CLIP_WEIGHT].tolist() == w[[4, 9, 70]].tolist()


# ---- the distribution -----------------------------------------------------------------------------------------------------
def test_ordered_pairs_of_a_draw_are_uniform():
    """L = 5, R = 2: 20 ordered pairs, 4000 epochs -> 200 expected each; chi^2 below the 0.999 quantile at 19 degrees of freedom
    (43.82).  The rule gives 16.2 for this seed (13.8 and 27.1 for seeds 0 and 12345)."""
    off, pool = np.array([0, 5], np.int32), np.repeat(np.arange(5, dtype=np.int32)[:, None], 3, axis=1)
    slot = np.array([37], np.int32)
    counts = np.zeros((5, 5), dtype=np.int64)
    for epoch in range(4000):
        t = np.full((2, 20, 3, 3), -9, dtype=np.int32)
        F.draw_context(slot, off, pool, t, 2, SEED, epoch)
        a, b = t[1, 17, 1:, 0].tolist()
        assert a != b and 0 <= a < 5 and 0 <= b < 5                # no entry twice in a draw
        counts[a, b] += 1
    assert counts.sum() == 4000 and (np.diag(counts) == 0).all()
    chi2 = float((((counts[~np.eye(5, dtype=bool)] - 200.0) ** 2) / 200.0).sum())
    print('chi^2 = %.2f' % chi2)
    assert chi2 < 43.82, chi2


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _long_world(n):
    """one scene of ``n`` interactions between two related characters: their context list has ``n`` entries"""
    inters = [F.Interaction('tt1', 0, 'act0', ['anna', 'bert'], {0: 'anna', 1: 'bert'}, rel='rel0', empty_tracks=('anna', 'bert'))
              for _ in range(n)]
    return F.World(inters, ['rel0'], ['act0'], {'tt1': {('anna', 'bert'): {0: 'rel0'}}}, text_dim=4, visual_dim=4, track_dim=4)


def test_a_list_of_4097_entries_is_refused():
    w = _long_world(4097)
    assert len(w.context_lists(18)[0][('tt1', 'anna', 'bert', 'rel0')]) == 4097
    with pytest.raises(LirecError, match=r'anna.*bert.*4097'):
        F.PiecesDataset(w, 18, pin_memory=False, context_draw='random')
    assert F.CONTEXT_LIST_MAX == _lib.CONTEXT_LIST_MAX == 4096


def test_slot_ids_beyond_32_bits_are_refused_when_planned():
    most = ((1 << 32) - 1) // F.T_MAX
    F.check_context_slots(most)
    F.check_context_slots(72)
    for n in (most + 1, 1 << 28, 1 << 40):
        with pytest.raises(LirecError, match='32-bit'):
            F.check_context_slots(n)
    F.check_context_slots((1 << 32) - 1, 1)
    with pytest.raises(LirecError):
        F.check_context_slots(1 << 32, 1)


def test_a_block_store_over_a_random_dataset_is_refused():
    from lirec_amd.blockstore import ResidentBlockDataset
    with pytest.raises(LirecError, match='context_draw'):
        ResidentBlockDataset(random_ds(emit='tiled'), device='cuda')


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
DST, OFF, POOL, ROWS = (0x10000000 * k for k in range(1, 5))       # fake, aligned, never dereferenced


def _args(**kw):
    a = _lib.DrawContextArgs()
    a.slot_dst, a.slot_off, a.pool_rows, a.index_rows = DST, OFF, POOL, ROWS
    a.seed, a.epoch, a.S, a.R, a.E = SEED, 3, 300, 18, 20 * 19
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_export_binding_struct_and_site():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    assert re.search(r'\blirec_draw_context\s*\(', hdr) and 'lirec_draw_context' in _lib.EXPORTS and hasattr(L, 'lirec_draw_context')
    assert re.search(r'LIREC_SITE_CONTEXT_DRAW\s*=\s*6\b', hdr) and re.search(r'#define LIREC_CONTEXT_LIST_MAX 4096\b', hdr)
    assert _lib.SITE_CONTEXT_DRAW == F.SITE_CONTEXT_DRAW == DC.SITE == 6
    assert L.lirec_abi_sizeof(41) == C.sizeof(_lib.DrawContextArgs) == 56 and L.lirec_abi_sizeof(40) == L.lirec_abi_sizeof(42) == -1
    assert L.lirec_version() == _lib.ABI_VERSION == 124


BAD = {'null slot_dst': dict(slot_dst=None), 'null slot_off': dict(slot_off=None), 'null pool_rows': dict(pool_rows=None),
       'null index_rows': dict(index_rows=None), 'S < 0': dict(S=-1), 'R < 1': dict(R=0), 'R < 0': dict(R=-3), 'E < R + 1': dict(E=18),
       'E < 0': dict(E=-1), 'R at the top of int32': dict(R=0x7fffffff, E=0x7fffffff),
       'slot_dst misaligned': dict(slot_dst=DST + 2), 'slot_off misaligned': dict(slot_off=OFF + 1),
       'pool_rows misaligned': dict(pool_rows=POOL + 2), 'index_rows misaligned': dict(index_rows=ROWS + 3)}


@pytest.mark.parametrize('dry', [False, True], ids=['plain', 'dry-run'])
@pytest.mark.parametrize('what', sorted(BAD))
def test_invalid_arguments_are_refused_before_any_device_call(what, dry):
    """without the dry run a call that got past the checks would reach the HIP runtime, which has no device here"""
    L = _lib.lib()
    if dry:
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_draw_context(C.byref(_args(**BAD[what])), None) == EINVAL, what
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def test_null_struct_no_slots_and_a_recorded_dry_call():
    L = _lib.lib()
    assert L.lirec_draw_context(None, None) == EINVAL
    assert L.lirec_draw_context(C.byref(_args(S=0)), None) == 0                                   # no launch: no device here
    assert L.lirec_draw_context(C.byref(_args(S=0, slot_dst=None, slot_off=None, pool_rows=None, index_rows=None)), None) == 0
    for what in ('R < 1', 'E < R + 1', 'index_rows misaligned'):
        assert L.lirec_draw_context(C.byref(_args(S=0, **BAD[what])), None) == EINVAL, what       # (the checks come first)
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_draw_context(C.byref(_args()), None) == 0
        assert L.lirec_draw_context(C.byref(_args(E=19, S=1, epoch=0xFFFFFFFF, seed=0xFFFFFFFFFFFFFFFF)), None) == 0
        assert L.lirec_record_begin() == 0
        assert L.lirec_draw_context(C.byref(_args()), None) == 0
        assert L.lirec_draw_context(C.byref(_args(S=0)), None) == 0                               # (no launch: nothing recorded)
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0
        assert L.lirec_cmdlist_size(h) == 1                                                       # one launch
        assert L.lirec_cmdlist_replay(h, 0, -1) == 0
        assert L.lirec_cmdlist_destroy(h) == 0
    finally:
        assert L.lirec_debug_set(0, -1) == 0


# ---- the default mode -----------------------------------------------------------------------------------------------------
def test_strided_is_the_dataset_as_it_was():
    """the constructor's work before the mode existed, restated: assemble_sample + world_rows per sample, stacked"""
    w = world()
    for ds in (strided(), F.PiecesDataset(w, R, pin_memory=False, context_draw='strided', context_seed=99)):
        assert ds.context_draw == 'strided'
        for k in ('slot_dst', 'slot_off', 'pool_rows', '_base_rows', '_drawn', 'context_seed'):
            assert not hasattr(ds, k), k
        class_of = {n: k for k, n in enumerate(w.inter_names)}
        samples = []
        for i in range(len(w.interactions)):
            sm = F.assemble_sample(w, i, R, len(w.inter_names), class_of)
            sm['index_rows'], sm['_id'] = F.world_rows(w, sm), i
            samples.append(sm)
            got = ds[i]
            assert got is ds._samples[i] and list(got) == list(sm)                                # the stored dict, the same keys in order
            for k in sm:
                assert (got[k] == sm[k]) if k == 'track_keys' else np.array_equal(got[k], sm[k]), (i, k)
        assert list(ds._stacked) == list(F._FIELDS) + ['index_rows']
        for k in F._FIELDS:
            want = np.array([sm[k] for sm in samples])
            assert ds._stacked[k].dtype == want.dtype and np.array_equal(ds._stacked[k], want), k
        want = np.stack([sm['index_rows'] for sm in samples])
        assert ds._stacked['index_rows'].dtype == np.int32 and np.array_equal(ds._stacked['index_rows'], want)
        for epoch in (0, 5):                                                                      # the epoch changes nothing
            ds.epoch = epoch
            assert ds.epoch_rows() is ds._stacked['index_rows']
            idx = [3, 17, 44, 71]
            a = ds.collate_fn([ds[i] for i in idx])
            b = F.collate(w, [samples[i] for i in idx])
            assert tuple(a['_layout']) == tuple(b['_layout']) and torch.equal(a['_blob'], b['_blob'])
            assert torch.equal(a['clip_table'], b['clip_table']) and torch.equal(a['track_table'], b['track_table'])
        assert getattr(ds.collate_fn, 'refresh', None) is None
