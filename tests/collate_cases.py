"""Inputs and expected sides for lirec_collate_resident (include/lirec_hip.h) -- shared by tests/test_host_collate.py and
tests/test_gpu_collate.py.  Not a test module.

A case is a set of synthetic stacked sample tables (no World): ``index_rows`` int32 [N, E, 3] with E = T * (R + 1), column 0 drawn
from [-1, n_clip_all), columns 1 and 2 from [-1, n_track_all) with a share of -1, a list of B sample ids, and five byte fields of
row_bytes 1, 8, 16, 160 and 808 (the bool field ... ``multilab_weights`` at 101 classes).  The expected side is
``lirec_amd.features._dedup`` plus the takes of ``features.collate`` -- never a run of the kernel.  ``restate`` says the same the way
the kernels do it (byte map -> exclusive scan in chunks with a carry -> ranks), in numpy.

Store sizes: 1, 2, 31, 32, 33, 255, 256, 257 and one below, at and above every granule of the rank scan (csrc/kernels.hpp,
collate_rank_kernel): 16 rows a thread (15, 16, 17), 1024 rows a wave (1023, 1024, 1025), COLLATE_SCAN_CHUNK = 16384 rows a round
(16383, 16384, 16385: one round, exactly one, two with a carry); 300000 / 299999 rows: 19 rounds.  The clip and the track store of
a case get different sizes from that list.  B in {1, 2, 3, 4, 64}: the field destinations lie back to back, so B = 1, 2, 3 put
them at odd addresses (byte moves), B = 4 at multiples of 4, B = 64 at multiples of 16 (16-byte moves; 808 = 8 * 101: 8-byte)."""
import numpy as np

from lirec_amd import features as F

SCAN_CHUNK = 16384
FIELD_BYTES = (1, 8, 16, 160, 808)
SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385)


def list_lengths(B, E, n_clip_all, n_track_all):
    """the static layout's row-list lengths (features.batch_layout)"""
    return min(B * E, n_clip_all) + 1, min(2 * B * E, n_track_all) + 1


def make(name, n_clip_all, n_track_all, B, T=3, R=2, N=7, seed=0, neg=0.25, ids=None, clip=None, track=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    E = T * (R + 1)
    rows = np.empty((N, E, 3), dtype=np.int32)
    rows[..., 0] = rng.integers(0, n_clip_all, size=(N, E))
    rows[..., 1:] = rng.integers(0, n_track_all, size=(N, E, 2))
    rows[rng.random((N, E, 3)) < neg] = -1
    if clip is not None:
        rows[..., 0] = np.asarray(clip, dtype=np.int32).reshape(N, E)
    if track is not None:
        rows[..., 1:] = np.asarray(track, dtype=np.int32).reshape(N, E, 2)
    ids = rng.integers(0, N, size=B) if ids is None else np.asarray(ids)
    assert ids.shape == (B,) and ids.min() >= 0 and ids.max() < N
    assert rows[..., 0].max() < n_clip_all and rows[..., 1:].max() < n_track_all and rows.min() >= -1
    fields = [rng.integers(0, 256, size=(N, rb), dtype=np.uint8) for rb in FIELD_BYTES]
    return dict(name=name, n_clip_all=int(n_clip_all), n_track_all=int(n_track_all), B=int(B), E=E, N=N, ids=ids.astype(np.int32),
                index_rows=rows, fields=fields)


def _cases():
    out = []
    bs = (1, 2, 3, 64, 4)
    for k, n in enumerate(SIZES):
        out.append(make('n%d' % n, n, SIZES[len(SIZES) - 1 - k], bs[k % len(bs)], seed=100 + k))
    out.append(make('rounds_with_carry', 300000, 299999, 64, N=70, seed=1))
    out.append(make('real_T20_R18', 2048, 5000, 64, T=20, R=18, N=40, seed=2))
    out.append(make('real_T20_R18_odd', 257, 33, 3, T=20, R=18, N=5, seed=3))
    N, E = 7, 9
    out.append(make('no_clip_piece', 40, 50, 3, seed=4, clip=np.full(N * E, -1)))
    out.append(make('no_piece_at_all', 40, 50, 3, seed=5, clip=np.full(N * E, -1), track=np.full(N * E * 2, -1)))
    out.append(make('every_row', 33, 50, 7, seed=6, ids=np.arange(7), clip=np.arange(N * E) % 33, track=np.arange(N * E * 2) % 50))
    out.append(make('every_row_one_round', 16384, 16385, 64, N=64, T=16, R=15, seed=7, ids=np.arange(64),
                    clip=np.arange(64 * 256) % 16384, track=np.arange(64 * 512) % 16385))
    out.append(make('one_id_repeated', 257, 255, 64, seed=8, ids=np.full(64, 3)))
    out.append(make('all_ids_last', 31, 32, 3, seed=9, ids=np.full(3, 6)))
    out.append(make('single_sample_table', 17, 15, 2, N=1, seed=10, ids=np.zeros(2, dtype=np.int64)))
    return out


CASES = {c['name']: c for c in _cases()}


def expected(case):
    """feature_index [B, E, 3], clip_rows, track_rows (whole lists), counts [2], the five field arrays [B, row_bytes]"""
    ids = case['ids'].astype(np.int64)
    glob = case['index_rows'][ids]
    cu, cpos = F._dedup(np.ascontiguousarray(glob[..., 0]), case['n_clip_all'])
    tu, tpos = F._dedup(np.ascontiguousarray(glob[..., 1:]), case['n_track_all'])
    n_c, n_t = list_lengths(case['B'], case['E'], case['n_clip_all'], case['n_track_all'])
    fi = np.empty(glob.shape, dtype=np.int32)
    fi[..., 0] = cpos
    fi[..., 1:] = tpos
    lists = []
    for u, n_list, n_all in ((cu, n_c, case['n_clip_all']), (tu, n_t, case['n_track_all'])):
        r = np.full(n_list, n_all, dtype=np.int32)
        r[:u.size] = u
        lists.append(r)
    counts = np.array([max(cu.size, 1) + 1, max(tu.size, 1) + 1], dtype=np.int32)
    return dict(feature_index=fi, clip_rows=lists[0], track_rows=lists[1], counts=counts, fields=[f[ids] for f in case['fields']])


def restate(case, chunk=SCAN_CHUNK):
    """the same as the kernels go about it: marks in a byte map, an exclusive scan of the map chunk by chunk with a carry, the rank
    table, the row list written from the ranks, the padding, the counts"""
    ids = case['ids'].astype(np.int64)
    glob = case['index_rows'][ids]
    fi = np.full(glob.shape, -1, dtype=np.int32)
    lists, counts = [], []
    n_lists = list_lengths(case['B'], case['E'], case['n_clip_all'], case['n_track_all'])
    for t, (sl, n_all) in enumerate(((slice(0, 1), case['n_clip_all']), (slice(1, 3), case['n_track_all']))):
        v = glob[..., sl]
        seen = np.zeros((n_all + 1 + 255) // 256 * 256, dtype=np.uint8)
        seen[v[v >= 0]] = 1
        rank = np.full(n_all + 1, -(2 ** 31), dtype=np.int64)              # (only the marked rows are ever written, or read)
        rows = np.full(n_lists[t], -7, dtype=np.int32)
        carry = 0
        for base in range(0, (n_all + 15) // 16 * 16, chunk):
            part = seen[base:base + chunk].astype(np.int64)
            excl = np.cumsum(part) - part + carry
            for i in np.flatnonzero(part):
                rank[base + i] = excl[i]
                rows[excl[i]] = base + i
            carry += int(part.sum())
        rows[carry:] = n_all
        fi[..., sl] = np.where(v >= 0, rank[np.maximum(v, 0)], -1)
        lists.append(rows)
        counts.append(max(carry, 1) + 1)
    return dict(feature_index=fi, clip_rows=lists[0], track_rows=lists[1], counts=np.array(counts, dtype=np.int32),
                fields=[f[ids] for f in case['fields']])


def workspace_bytes(n_clip_all, n_track_all):
    """lirec_collate_workspace_bytes, restated: a byte map (+ the zero row) and an int32 rank table per store, each rounded to 256"""
    up = lambda n: (n + 255) // 256 * 256
    return up(n_clip_all + 1) + up(n_track_all + 1) + up(4 * (n_clip_all + 1)) + up(4 * (n_track_all + 1))
