"""Inputs and expected sides for lirec_draw_context (include/lirec_hip.h) and ``lirec_amd.features.draw_context`` -- shared by
tests/test_host_context_draw.py and tests/test_gpu_context_draw.py.  Not a test module.

A kernel case is a set of synthetic tables (no World): an ``index_rows`` table int32 [N, T, R + 1, 3] pre-filled with a sentinel, S
slots at chosen (sample, candidate) places with their lists in CSR form (``slot_dst``, ``slot_off``, ``pool_rows`` of random rows in
[-1, 1000)), and the (seed, epoch) pairs it is run at.  ``restate`` is the draw rule written independently of the package: the
oracle's Philox, Python integers for the keys, ``sorted`` for the order.

List lengths at R = 18: R + 1, one below / at / above a wave (63, 64, 65), the workgroup (255, 256, 257), four rounds of it (1023,
1024, 1025) and the limit (4095, 4096); L = 2 at R = 1 and L = 3 at R = 2, the smallest draws there are.  Placement: one slot alone;
slots at the table's very first and very last (sample, candidate); 300 slots of mixed lengths (more workgroups than the device has
compute units).  Epochs 0, 1, 2^31 and 2^32 - 1 (the counter word's sign bit and its last value); seeds 0 and 0x5eed00000007 (both
key halves in use)."""
import numpy as np

from oracle import lirec_oracle as O

SITE = 6                                        # LIREC_SITE_CONTEXT_DRAW
SENTINEL = -77
SEEDS = (0, 0x5eed00000007)
EPOCHS = (0, 1, 1 << 31, (1 << 32) - 1)
LENGTHS_R18 = (19, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)

# the world of the reference-semantics tests (tests/test_host_context_draw.py, tests/test_gpu_context_draw.py)
WORLD = dict(seed=3, n_scenes=12, per_scene=6, n_chars=5, text_dim=8, visual_dim=16, track_dim=16, n_inter_names=9, n_rel_names=3)
WORLD_R = 3


def make(name, N, T, R, slots, lengths, runs, seed=0):
    """``slots``: slot ids (sample * T + candidate), ``lengths``: their list lengths, ``runs``: the (seed, epoch) pairs"""
    rng = np.random.Generator(np.random.PCG64(seed))
    slots, lengths = np.asarray(slots, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    assert slots.shape == lengths.shape and len(set(slots.tolist())) == slots.size
    assert slots.min() >= 0 and slots.max() < N * T and lengths.min() > R >= 1 and lengths.max() <= 4096
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    pool = rng.integers(-1, 1000, size=(int(off[-1]), 3)).astype(np.int32)
    return dict(name=name, N=N, T=T, R=R, slot_dst=slots.astype(np.uint32).view(np.int32), slot_off=off, pool_rows=pool, runs=tuple(runs))


def _cases():
    rng = np.random.Generator(np.random.PCG64(9))
    out = []
    # every length of the list, the first and the last slot of the table among them; every epoch and both seeds
    N, T = 2, 8
    places = [0, N * T - 1] + list(range(2, 2 + len(LENGTHS_R18) - 2))
    out.append(make('lengths_R18', N, T, 18, places, LENGTHS_R18, [(s, e) for s in SEEDS for e in EPOCHS], seed=1))
    out.append(make('one_slot', 3, 4, 18, [6], [65], [(SEEDS[0], 1), (SEEDS[1], 1 << 31)], seed=2))
    N, T = 40, 20
    places = rng.permutation(N * T)[:300]
    mixed = np.concatenate([rng.integers(19, 600, size=300 - len(LENGTHS_R18)), LENGTHS_R18])
    out.append(make('slots_300', N, T, 18, places, rng.permutation(mixed), [(SEEDS[1], 0), (SEEDS[0], (1 << 32) - 1)], seed=3))
    out.append(make('L2_R1', 2, 3, 1, [0, 5, 2], [2, 2, 2], [(SEEDS[0], 0), (SEEDS[1], (1 << 32) - 1)], seed=4))
    out.append(make('L3_R2', 2, 3, 2, [5, 0], [3, 3], [(SEEDS[1], 1), (SEEDS[0], 1 << 31)], seed=5))
    return out


CASES = {c['name']: c for c in _cases()}
RUNS = [(name, k) for name in sorted(CASES) for k in range(len(CASES[name]['runs']))]


def sentinel_table(case):
    return np.full((case['N'], case['T'], case['R'] + 1, 3), SENTINEL, dtype=np.int32)


def restate(case, seed, epoch):
    """the sentinel table after the draw of (seed, epoch), by the rule as the issue words it: key_j = (word 0 of
    philox4x32_10(counter = (j, slot, SITE, epoch), key = (seed lo, seed hi)) << 32) | j, the R smallest in ascending order"""
    R = case['R']
    table = sentinel_table(case).reshape(-1, R + 1, 3)
    off, pool = case['slot_off'], case['pool_rows']
    for i, slot in enumerate(case['slot_dst'].view(np.uint32).tolist()):
        L = int(off[i + 1] - off[i])
        j = np.arange(L, dtype=np.uint32)
        full = lambda v: np.full(L, v, dtype=np.uint32)
        words = O.philox4x32_10(j, full(slot), full(SITE), full(epoch % (1 << 32)), seed & 0xFFFFFFFF, seed >> 32)[0]
        keys = [(int(w) << 32) | k for k, w in enumerate(words.tolist())]
        assert len(set(keys)) == L
        for p, k in enumerate(sorted(range(L), key=keys.__getitem__)[:R]):
            table[slot, 1 + p] = pool[int(off[i]) + k]
    return table.reshape(case['N'], case['T'], R + 1, 3)


def slot_rows_mask(case):
    """True on rows 1 .. R of the slots: everything a draw may write"""
    m = np.zeros((case['N'] * case['T'], case['R'] + 1), dtype=bool)
    m[case['slot_dst'].view(np.uint32).astype(np.int64), 1:] = True
    return m.reshape(case['N'], case['T'], case['R'] + 1)
