"""lirec_collate_resident without a GPU: the two exports and the struct, every LIREC_EINVAL of the contract before any device call
(with and without the library's host-side dry run), the workspace formula, the numpy restatement of the kernels against
``features._dedup`` and against ``features.collate(static_layout=True)``, ``ResidentLoader``'s batch order against
``ThreadedLoader``'s, the factored buffer layout, and a dry run of the loader that counts the launches."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import collate_cases as CC
from lirec_amd import _lib, config, features as F
from lirec_amd.config import opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL
# fake, aligned, never dereferenced
IDS, ROWS, FI, CR, TR, CNT, WS, SRC, DST = (0x10000000 * k for k in range(1, 10))
R = 18


def _args(nf=2, **kw):
    a = _lib.CollateArgs()
    a.ids, a.index_rows, a.feature_index, a.clip_rows, a.track_rows, a.counts, a.workspace = IDS, ROWS, FI, CR, TR, CNT, WS
    a.n_clip_all, a.n_track_all, a.n_clip_list, a.n_track_list = 2048, 5000, 2049, 5001
    a.workspace_bytes = CC.workspace_bytes(2048, 5000)
    a.B, a.E, a.nf = 64, 380, nf
    for f in range(max(min(nf, _lib.COLLATE_MAX_FIELDS), 0)):
        a.fields[f].src, a.fields[f].row_bytes, a.fields[f].dst = SRC + 0x100000 * f, (1, 808)[f % 2], DST + 0x100000 * f + f
    fields = kw.pop('fields', {})
    for k, v in kw.items():
        setattr(a, k, v)
    for f, over in fields.items():
        for k, v in over.items():
            setattr(a.fields[f], k, v)
    return a


def test_exports_binding_and_struct_size():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'lirec_hip.h')).read()
    for name in ('lirec_collate_resident', 'lirec_collate_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lirec_abi_sizeof(17) == C.sizeof(_lib.CollateArgs) == 112 + 24 * _lib.COLLATE_MAX_FIELDS
    assert C.sizeof(_lib.CollateField) == 24 and _lib.COLLATE_MAX_FIELDS == 16
    assert L.lirec_abi_sizeof(16) == -1 and L.lirec_abi_sizeof(18) == -1
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert 'device_collate' in config.defaults() and config.defaults()['device_collate'] is False


BAD = {
    'null ids': dict(ids=None), 'null index_rows': dict(index_rows=None), 'null feature_index': dict(feature_index=None),
    'null clip_rows': dict(clip_rows=None), 'null track_rows': dict(track_rows=None), 'null counts': dict(counts=None),
    'null workspace': dict(workspace=None), 'null field src': dict(fields={1: dict(src=None)}), 'null field dst': dict(fields={0: dict(dst=None)}),
    'B < 0': dict(B=-1), 'E < 0': dict(E=-1), 'E < 1': dict(E=0), 'nf < 0': dict(nf=-1), 'nf over the limit': dict(nf=17),
    'n_clip_all < 0': dict(n_clip_all=-1), 'n_track_all < 0': dict(n_track_all=-5), 'workspace_bytes < 0': dict(workspace_bytes=-1),
    'row_bytes 0': dict(fields={0: dict(row_bytes=0)}), 'row_bytes < 0': dict(fields={1: dict(row_bytes=-8)}),
    'n_clip_list < 2': dict(n_clip_list=1), 'n_track_list < 2': dict(n_track_list=0), 'n_track_list < 0': dict(n_track_list=-3),
    'workspace one byte short': dict(workspace_bytes=CC.workspace_bytes(2048, 5000) - 1),
    'workspace of a smaller world': dict(workspace_bytes=CC.workspace_bytes(2048, 4000)),
    'workspace misaligned': dict(workspace=WS + 8),
    'stores beyond int32': dict(n_clip_all=1 << 31, workspace_bytes=1 << 40),
}
BAD.update({'%s misaligned' % k: {k: v + 2} for k, v in (('ids', IDS), ('index_rows', ROWS), ('feature_index', FI), ('clip_rows', CR),
                                                         ('track_rows', TR), ('counts', CNT))})


@pytest.mark.parametrize('dry', [False, True], ids=['plain', 'dry-run'])
@pytest.mark.parametrize('what', sorted(BAD))
def test_invalid_arguments_are_refused_before_any_device_call(what, dry):
    """without the dry run a call that got past the checks would reach the HIP runtime, which has no device here"""
    L = _lib.lib()
    if dry:
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_collate_resident(C.byref(_args(**BAD[what])), None) == EINVAL, what
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def test_null_struct_and_empty_batch():
    L = _lib.lib()
    assert L.lirec_collate_resident(None, None) == EINVAL
    assert L.lirec_collate_resident(C.byref(_args(B=0)), None) == 0                              # no launch: no device here
    nulls = dict(ids=None, index_rows=None, feature_index=None, clip_rows=None, track_rows=None, counts=None, E=0)
    assert L.lirec_collate_resident(C.byref(_args(B=0, **nulls)), None) == 0                     # (nothing is needed for no batch)
    for what in ('nf over the limit', 'row_bytes 0', 'n_clip_list < 2', 'workspace one byte short', 'ids misaligned', 'E < 0'):
        assert L.lirec_collate_resident(C.byref(_args(B=0, **BAD[what])), None) == EINVAL, what  # (the checks come first)


def test_valid_calls_in_the_dry_mode_are_four_commands_each():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_collate_resident(C.byref(_args()), None) == 0
        assert L.lirec_collate_resident(C.byref(_args(nf=0)), None) == 0
        assert L.lirec_collate_resident(C.byref(_args(nf=16)), None) == 0
        assert L.lirec_collate_resident(C.byref(_args(B=1, E=1, n_clip_all=0, n_track_all=0, n_clip_list=2, n_track_list=2,
                                                      workspace_bytes=CC.workspace_bytes(0, 0))), None) == 0
        assert L.lirec_collate_resident(C.byref(_args(workspace_bytes=1 << 30)), None) == 0      # (a larger workspace is fine)
        assert L.lirec_record_begin() == 0
        assert L.lirec_collate_resident(C.byref(_args()), None) == 0
        assert L.lirec_collate_resident(C.byref(_args(B=0)), None) == 0                          # (no launch: nothing recorded)
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0
        assert L.lirec_cmdlist_size(h) == 4            # the clear, the marks, the two scans in one launch, the index + the fields
        assert L.lirec_cmdlist_replay(h, 0, -1) == 0
        assert L.lirec_cmdlist_destroy(h) == 0
    finally:
        assert L.lirec_debug_set(0, -1) == 0


def test_workspace_bytes_is_monotone_and_sufficient():
    L = _lib.lib()
    assert L.lirec_collate_workspace_bytes(-1, 4) == -1 and L.lirec_collate_workspace_bytes(4, -1) == -1
    sizes = (0,) + CC.SIZES + (299999, 300000, 10 ** 7)
    for a in sizes:
        for b in sizes:
            got = L.lirec_collate_workspace_bytes(a, b)
            assert got == CC.workspace_bytes(a, b) and got % 256 == 0
            # a byte and an int32 per row of either store, the zero rows included
            assert got >= 5 * (a + 1) + 5 * (b + 1)
    for a, b in zip(sizes, sizes[1:]):
        assert L.lirec_collate_workspace_bytes(a, 7) <= L.lirec_collate_workspace_bytes(b, 7)
        assert L.lirec_collate_workspace_bytes(7, a) <= L.lirec_collate_workspace_bytes(7, b)
    for case in CC.CASES.values():
        # the scan reads whole 16-byte words of the map: they lie inside its share of the workspace
        for n in (case['n_clip_all'], case['n_track_all']):
            assert (n + 15) // 16 * 16 <= (n + 1 + 255) // 256 * 256


def test_binding_refuses_host_tensors():
    from lirec_amd import ops
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises((_lib.LirecError, AssertionError)):
        ops.collate_resident(i32(2), i32(3, 4, 3), 5, 5, i32(2, 4, 3), i32(6), i32(6), i32(2), [], torch.zeros(4096, dtype=torch.uint8))


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    for k in ('feature_index', 'clip_rows', 'track_rows', 'counts'):
        assert got[k].dtype == want[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    assert len(got['fields']) == len(want['fields'])
    for f, (a, b) in enumerate(zip(got['fields'], want['fields'])):
        assert np.array_equal(a, b), (what, f)


@pytest.mark.parametrize('name', sorted(CC.CASES))
def test_the_restatement_equals_dedup(name):
    case = CC.CASES[name]
    want = CC.expected(case)
    _same(CC.restate(case), want, name)
    _same(CC.restate(case, chunk=16), want, name)               # (a carry in every case, whatever its size)
    # the facts about the cases the GPU test relies on
    n_c, n_t = CC.list_lengths(case['B'], case['E'], case['n_clip_all'], case['n_track_all'])
    assert want['clip_rows'].shape == (n_c,) and want['track_rows'].shape == (n_t,) and n_c >= 2 and n_t >= 2
    assert want['counts'][0] <= n_c and want['counts'][1] <= n_t


def test_the_cases_cover_what_they_are_meant_to():
    E = {n: CC.expected(c) for n, c in CC.CASES.items()}
    assert {c['n_clip_all'] for c in CC.CASES.values()} >= set(CC.SIZES) and {c['B'] for c in CC.CASES.values()} >= {1, 2, 3, 64}
    assert (E['no_clip_piece']['feature_index'][..., 0] == -1).all() and E['no_clip_piece']['counts'][0] == 2
    assert (E['no_clip_piece']['clip_rows'] == 40).all() and E['no_clip_piece']['counts'][1] > 2
    assert (E['no_piece_at_all']['feature_index'] == -1).all() and list(E['no_piece_at_all']['counts']) == [2, 2]
    for name, (nc, nt) in (('every_row', (33, 50)), ('every_row_one_round', (16384, 16385))):
        assert np.array_equal(E[name]['clip_rows'], np.arange(nc + 1)) and np.array_equal(E[name]['track_rows'], np.arange(nt + 1))
    assert len(set(CC.CASES['one_id_repeated']['ids'])) == 1 and (CC.CASES['all_ids_last']['ids'] == 6).all()
    big = CC.CASES['rounds_with_carry']
    assert big['n_clip_all'] > 18 * CC.SCAN_CHUNK and E['rounds_with_carry']['clip_rows'][:-1].max() > 17 * CC.SCAN_CHUNK
    assert sum(v.nbytes for v in [big['index_rows']] + big['fields']) < 1 << 20
    assert CC.CASES['real_T20_R18']['E'] == 20 * 19 and any((c['index_rows'] == -1).any() for c in CC.CASES.values())


def _world(seed=5, n_scenes=5, per_scene=5):
    return F.synthetic_world(seed, n_scenes=n_scenes, per_scene=per_scene)


def test_the_restatement_equals_collate_on_a_synthetic_world():
    """the stacked tables of a PiecesDataset as a case: the restatement gives ``collate(static_layout=True)``, field by field"""
    world = _world()
    ds = F.PiecesDataset(world, R, pin_memory=False, resident=True)
    clip_all, track_all, _ = world.piece_matrices()
    st = ds._stacked
    N = len(ds)
    for ids in ([3, 0, 7, 7, 12], [N - 1], list(range(N)), [4, 4, 4]):
        batch = ds.collate_fn([ds[i] for i in ids])
        assert 'piece_counts' in batch and batch['clip_rows'].dtype == torch.int32
        fields = [np.ascontiguousarray(st[k]).reshape(N, -1).view(np.uint8) for k in F._FIELDS]
        case = dict(name='world', n_clip_all=clip_all.shape[0], n_track_all=track_all.shape[0], B=len(ids), E=F.T_MAX * (R + 1), N=N,
                    ids=np.asarray(ids, dtype=np.int32), index_rows=st['index_rows'].reshape(N, -1, 3), fields=fields)
        got = CC.restate(case)
        assert np.array_equal(got['feature_index'].reshape(batch['feature_index'].shape), batch['feature_index'].numpy())
        assert np.array_equal(got['clip_rows'], batch['clip_rows'].numpy()) and np.array_equal(got['track_rows'], batch['track_rows'].numpy())
        assert tuple(got['counts']) == tuple(batch['piece_counts'])
        for k, g in zip(F._FIELDS, got['fields']):
            want = batch[k].numpy()
            assert np.array_equal(g.reshape(-1), np.ascontiguousarray(want).reshape(-1).view(np.uint8)), k


@pytest.mark.parametrize('B', [1, 2, 5, 8, 64])
def test_batch_layout_reproduces_collates_layout(B):
    from lirec_amd.loader import ResidentLoader
    world = _world(6, n_scenes=4, per_scene=4)
    for resident in (True, False):
        ds = F.PiecesDataset(world, R, pin_memory=False, resident=resident)
        ids = [i % len(ds) for i in range(B)]
        batch = ds.collate_fn([ds[i] for i in ids])
        clip_all, track_all, _ = world.piece_matrices()
        fields = [(k, ds._stacked[k].dtype, (B,) + ds._stacked[k].shape[1:]) for k in F._FIELDS]
        shape = (B,) + ds._stacked['index_rows'].shape[1:]
        layout, nbytes = F.batch_layout(shape, fields, n_all=(clip_all.shape[0], track_all.shape[0]) if resident else None)
        assert layout == batch['_layout'] and nbytes == batch['_blob'].numel()
        if resident:
            loader = ResidentLoader(ds, batch_size=B, device='cpu')              # (no device is touched before the first batch)
            assert tuple(loader.layout(B)[0]) == tuple(batch['_layout']) and loader.layout(B)[1] == nbytes
            # the dynamic form: the lists as long as the batch needs them
            dyn = F.collate(world, [ds[i] for i in ids], stacked=ds._stacked, store=ds.store)
            assert dyn['_layout'] == F.batch_layout(shape, fields, n_rows=dyn['piece_counts'])[0]
            views = F.layout_views(batch['_blob'], layout)
            assert all(torch.equal(views[k], batch[k]) for k in F._FIELDS + ('feature_index', 'clip_rows', 'track_rows'))


def test_device_tables_validate_the_index_once():
    world = _world(7, n_scenes=3, per_scene=3)
    ds = F.PiecesDataset(world, R, pin_memory=False, resident=True)
    tabs = ds.device_tables('cpu')
    assert tabs is ds.device_tables('cpu') and tabs['index_rows'].dtype == torch.int32
    assert tabs['n_all'] == tuple(m.shape[0] for m in world.piece_matrices()[:2])
    assert all(torch.equal(tabs[k], torch.from_numpy(ds._stacked[k])) for k in F._FIELDS)
    for col, bad in ((0, tabs['n_all'][0]), (1, tabs['n_all'][1]), (2, -2)):
        other = F.PiecesDataset(world, R, pin_memory=False, resident=True)
        other._stacked['index_rows'][1, 0, 0, col] = bad
        with pytest.raises(ValueError):
            other.device_tables('cpu')


# ---- the order of the batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('drop_last', [False, True])
@pytest.mark.parametrize('how', ['sequential', 'shuffled', 'shard-sampler'])
def test_resident_loader_draws_the_batches_threaded_loader_draws(how, drop_last):
    from lirec_amd.loader import ResidentLoader, ThreadedLoader
    from lirec_amd.parallel import ShardSampler
    ds = F.PiecesDataset(_world(8), R, pin_memory=False, resident=True)

    def kw():
        if how == 'shard-sampler':
            s = ShardSampler(len(ds), 4, shuffle=True, seed=3, pad=True)
            s.set_epoch(1)
            return dict(sampler=s)
        return dict(shuffle=how == 'shuffled')
    rl = ResidentLoader(ds, batch_size=4, drop_last=drop_last, device='cpu', **kw())
    tl = ThreadedLoader(ds, batch_size=4, drop_last=drop_last, num_workers=1, collate_fn=lambda samples: [s['_id'] for s in samples], **kw())
    assert len(rl) == len(tl)
    for _ in range(2):                                       # (two epochs: the generator moves on the same way)
        torch.manual_seed(17)
        got = rl.epoch_ids()
        torch.manual_seed(17)
        want = list(tl)
        assert got == want and len(got) == len(rl)
    if how == 'shuffled':
        assert got != [sorted(b) for b in got] or len(ds) < 3
    with pytest.raises(ValueError):
        ResidentLoader(F.PiecesDataset(_world(8), R, pin_memory=False), batch_size=4)


def test_the_flag_falls_back_without_complaint():
    from lirec_amd.loader import device_collate_in_force
    ds = F.PiecesDataset(_world(8), R, pin_memory=False, resident=True)
    try:
        config.reset()
        assert not device_collate_in_force(ds, 'cuda')                               # off by default
        opt.device_collate = True
        assert device_collate_in_force(ds, 'cuda') and device_collate_in_force(ds, 'cuda:1')
        assert not device_collate_in_force(ds, 'cpu')
        assert not device_collate_in_force(F.PiecesDataset(_world(8), R, pin_memory=False), 'cuda')      # host tables
        assert not device_collate_in_force(F.PiecesDataset(_world(8), R, emit='tiled', resident=True), 'cuda')
        assert not device_collate_in_force(torch.utils.data.TensorDataset(torch.zeros(3)), 'cuda')
        for flag in ('pieces_gather', 'pieces_q32b', 'layer1_planes'):
            setattr(opt, flag, False)
            assert not device_collate_in_force(ds, 'cuda'), flag
            setattr(opt, flag, True)
    finally:
        config.reset()


# ---- the loader in the library's dry run: launches handed to nobody ---------------------------------------------------------
def test_dry_run_of_the_resident_loader_counts_the_launches():
    """a process of its own: the dry run patches torch and switches the library process-wide"""
    code = ('import ctypes as C\n'
            'import host_dryrun as H, torch\n'
            'from lirec_amd import _lib, ops, features as F\n'
            'from lirec_amd.config import opt\n'
            'from lirec_amd.loader import ResidentLoader, device_collate_in_force\n'
            'L = _lib.lib(); assert L.lirec_debug_set(H.DRY, -1) == 0; H.patch()\n'
            'opt.device_collate = True\n'
            'ds = F.PiecesDataset(F.synthetic_world(9, n_scenes=4, per_scene=4), 18, pin_memory=False, resident=True)\n'
            'assert device_collate_in_force(ds, "cuda")\n'
            'loader = ResidentLoader(ds, batch_size=5, shuffle=True, device="cpu")\n'
            'assert len(loader) == 4\n'
            'ops.CommandList.begin()\n'
            'batches = list(loader)\n'
            'cmds = ops.CommandList.end()\n'
            'assert cmds.size == 4 * len(loader) and loader.n_collate == 4 and loader.n_in_place == 0, (cmds.size, loader.n_collate)\n'
            'cmds.replay(); cmds.destroy()\n'
            'ref = ds.collate_fn([ds[0], ds[1], ds[2], ds[3], ds[4]])\n'
            'assert [len(b["labels"]) for b in batches] == [5, 5, 5, 1]\n'
            'b = batches[0]\n'
            'assert tuple(b["_layout"]) == tuple(ref["_layout"]) and b["piece_store"] is ds.store\n'
            'assert not ({"_blob", "_slots", "piece_counts"} & set(b))\n'
            'assert set(b) == (set(ref) - {"_blob", "_slots", "piece_counts"}) | {"_dev_blob"}\n'
            'for k in F._FIELDS + ("feature_index", "clip_rows", "track_rows"):\n'
            '    assert b[k].dtype == ref[k].dtype and b[k].shape == ref[k].shape, k\n'
            '# a bound buffer: batches of its layout are written there, the short one into a buffer of its own\n'
            'blob = b["_dev_blob"]\n'
            'loader.bind(b["_layout"], blob)\n'
            'again = list(loader)\n'
            'assert [x["_dev_blob"] is blob for x in again] == [True, True, True, False]\n'
            'assert loader.n_collate == 8 and loader.n_in_place == 3\n'
            'loader.unbind()\n'
            'assert not any(x["_dev_blob"] is blob for x in loader) and loader.n_in_place == 3\n'
            'assert L.lirec_debug_set(0, -1) == 0\n'
            'print("collate dry run ok")\n')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'collate dry run ok' in r.stdout, r.stdout[-4000:]
