"""The hot path's switches as a test matrix (no test module: tests/test_host_flag_matrix.py checks the matrix itself on the host,
tests/test_gpu_flag_matrix.py runs it on the device against the float64 oracle).

FACTORS are the perf flags of ``lirec_amd.config.defaults()`` that ``_run_forward`` / ``_run_backward`` (lirec_amd/model.py),
``StepLanes`` (lirec_amd/lanes.py), ``FusedAdam.step`` (lirec_amd/optim.py) and ``RecordedTrainStep`` (lirec_amd/graph.py) branch
on, plus the storage of the feature block (``to_device_batch(feature_dtype=)``: an fp32 block staged as q32b every step, or the
block stored as q32b and gathered).  ROWS is a literal list:

  * the default row;
  * one row per factor with that factor alone flipped;
  * ``all_flags_off``: every flag flipped on an fp32 block (the literal all-flipped row is refused, see REFUSALS);
  * a pairwise covering set over the pairs of factor values that can both take effect (``moot`` below).  Construction, for the
    record: start from the rows above; over all 2^10 rows that are not refused, in the order of ``itertools.product`` with the
    default value first, repeatedly take the first row that covers the most still uncovered pairs -- three rows;
  * ``all_flipped``: refused by the model (q32b storage without the q32b layer-1 kernels), asserted by its message.

The host test recomputes the required pairs from ``moot`` and fails when a row is lost or a flag is added without a decision.
"""
import itertools

FLAGS = ('compact_ctx_rows', 'layer1_planes', 'gate_q32', 'h1_sign_bits', 'gate_stage_on_side', 'wgrad_side_stream',
         'adam_on_side_stream', 'defer_side_join', 'fuse_dw1_adam')
STORAGE = 'feature_storage'                 # not an ``opt`` field: 'f32' (to_device_batch's default) or 'q32'
FACTORS = FLAGS + (STORAGE,)
VALUES = {f: (True, False) for f in FLAGS}  # (default, flipped)
VALUES[STORAGE] = ('f32', 'q32')

T, F = True, False
#                     compact planes gate_q32 h1_bits stage_side wgrad_side adam_side defer fuse_dw1 storage
ROWS = [
    ('default',            (T, T, T, T, T, T, T, T, T, 'f32')),
    ('compact_ctx_rows',   (F, T, T, T, T, T, T, T, T, 'f32')),
    ('layer1_planes',      (T, F, T, T, T, T, T, T, T, 'f32')),
    ('gate_q32',           (T, T, F, T, T, T, T, T, T, 'f32')),
    ('h1_sign_bits',       (T, T, T, F, T, T, T, T, T, 'f32')),
    ('gate_stage_on_side', (T, T, T, T, F, T, T, T, T, 'f32')),
    ('wgrad_side_stream',  (T, T, T, T, T, F, T, T, T, 'f32')),
    ('adam_on_side_stream', (T, T, T, T, T, T, F, T, T, 'f32')),
    ('defer_side_join',    (T, T, T, T, T, T, T, F, T, 'f32')),
    ('fuse_dw1_adam',      (T, T, T, T, T, T, T, T, F, 'f32')),
    ('feature_storage',    (T, T, T, T, T, T, T, T, T, 'q32')),
    ('all_flags_off',      (F, F, F, F, F, F, F, F, F, 'f32')),
    ('cover_1',            (F, T, T, F, F, T, F, F, F, 'q32')),      # side lane and staged gate kept, everything around them flipped
    ('cover_2',            (T, T, F, T, T, F, T, T, F, 'q32')),      # q32b layer 1 unfused on q32b storage, without side lane or staged gate
    ('cover_3',            (T, F, T, T, F, T, T, T, T, 'f32')),      # the gate's weights staged on the step's stream beside the on-the-fly layer 1
    ('all_flipped',        (F, F, F, F, F, F, F, F, F, 'q32')),
]
SINGLE_FLIPS = FACTORS                      # (the single-flip rows carry their factor's name)


def row(rid):
    """{factor: value} of row ``rid``"""
    return dict(zip(FACTORS, dict(ROWS)[rid]))


def moot(r, overwrite=True):
    """The factors that cannot take effect in row ``r`` whatever their own value (lirec_amd/model.py, graph.py):
      * gate_stage_on_side without a side lane (wgrad_side_stream) or without the staged gate (gate_q32): model.py, `gws` / `lane`;
      * fuse_dw1_adam without layer1_planes: graph.py, `self.fused` needs `model.last_layer1_planes`;
      * defer_side_join without the overwrite mode: graph.py, `self.defer` (``overwrite``: single GPU, no accumulation -- every
        recorded step of the matrix);
      * q32b storage without layer1_planes: nothing else reads it (model.py `_stage_plain` refuses, REFUSALS)."""
    m = set()
    if not (r['wgrad_side_stream'] and r['gate_q32']):
        m.add('gate_stage_on_side')
    if not r['layer1_planes']:
        m.update(('fuse_dw1_adam', STORAGE))
    if not overwrite:
        m.add('defer_side_join')
    return frozenset(m)


def effective(r, overwrite=True):
    """Row ``r`` as the code takes it: a moot flag reads False (its feature is not in force).  One more flag is inert without the
    side lane -- adam_on_side_stream (lanes.py `take_after_backward` asks for both) -- and reads False here too; it is NOT in
    ``moot``, so the covering requirement still asks for its pairs with wgrad_side_stream."""
    e = dict(r)
    for f in moot(r, overwrite):
        if f != STORAGE:
            e[f] = False
    e['adam_on_side_stream'] = bool(r['adam_on_side_stream'] and r['wgrad_side_stream'])
    return e


# the refusal a row meets instead of a step, by its message; predicted from ``moot`` alone
Q32_WITHOUT_PLANES = 'q32 feature storage is read by the q32b layer-1 kernels (opt.layer1_planes) only'
REFUSALS = {'all_flipped': Q32_WITHOUT_PLANES}


def refusal(r):
    """the LirecError message row ``r`` is refused with, or None"""
    return Q32_WITHOUT_PLANES if (r[STORAGE] == 'q32' and STORAGE in moot(r)) else None


def pairs_covered(r):
    """the (factor, value, factor, value) pairs row ``r`` covers: both factors in force"""
    m = moot(r)
    if refusal(r) is not None:
        return set()
    return {(a, r[a], b, r[b]) for a, b in itertools.combinations(FACTORS, 2) if a not in m and b not in m}


def pairs_required():
    """every pair of factor values that can take effect together in some row that is not refused"""
    req = set()
    for vals in itertools.product(*(VALUES[f] for f in FACTORS)):
        req |= pairs_covered(dict(zip(FACTORS, vals)))
    return req


def numeric_class(r):
    """Rows of one class compute the same bits.  The key holds the three factors that change arithmetic: which context rows
    layer 1 runs on and in which order the pooling sums them (compact_ctx_rows), the layer-1 kernels (layer1_planes: the
    persistent q32b kernels or the on-the-fly split core, another k order) and the gate's kernels (gate_q32).  Every other factor
    moves work between streams, launches or buffers: the sign bits are [H1 > 0] (tests/pool_cases.py: pack_sign_bits), q32b
    storage holds what the staging pass writes (tests/test_gpu_planes.py), the side streams run the same launches elsewhere
    (same file), the folded update and the deferred join are the eager update bit for bit
    (tests/test_gpu_recorded_bench_shape.py)."""
    return (r['compact_ctx_rows'], r['layer1_planes'], r['gate_q32'])


# Every other boolean or mode flag of the "build-side additions" block of config.defaults(), and why the matrix leaves it out
_OWN = 'has its own files: '
EXCLUDED = {
    'dp_shard_eval': 'evaluation under torch.distributed, no train step (tests/test_gpu_eval_loop.py, test_parallel_cpu.py)',
    'device_metrics': 'evaluation counters, no train step (tests/test_gpu_eval_topk.py, test_gpu_eval_loop.py)',
    'use_ce_loss': 'another loss module, not a switch of the step (tests/test_gpu_losses.py, test_gpu_parity.py)',
    'dropout_seed': 'a key, not a switch; every case sets it',
    'layer1_planes_eval': 'forward-only steps (tests/test_gpu_planes.py::test_forward_only_on_the_persistent_kernels)',
    'pieces_q32b': 'piece-table inputs: ' + _OWN + 'tests/test_gpu_feature_path.py, test_gpu_pieces_input_grad.py',
    'pieces_gather': 'piece-table inputs: ' + _OWN + 'tests/test_gpu_feature_path.py, test_gpu_loops.py',
    'recorded_training': 'training() over a resident store: ' + _OWN + 'tests/test_gpu_loops.py, test_host_train_loop.py',
    'device_collate': 'the loader\'s collate call: ' + _OWN + 'tests/test_gpu_collate.py, test_host_collate.py',
    'record_block_store': 'block-store batches: ' + _OWN + 'tests/test_gpu_blockstore_recorded.py, test_host_blockstore_recorded.py',
    'decoupled_weight_decay': 'FusedAdam feature, ' + _OWN + 'tests/test_gpu_adamw.py, test_host_adamw.py',
    'skip_nonfinite': 'FusedAdam feature, ' + _OWN + 'tests/test_gpu_nonfinite.py, test_gpu_guard.py',
    'ema_decay': 'FusedAdam feature, ' + _OWN + 'tests/test_gpu_ema.py, test_host_ema.py',
    'accumulate_steps': 'FusedAdam feature, ' + _OWN + 'tests/test_gpu_accum.py, test_host_accum.py',
    'param_stats_every': 'a printout of training(), ' + _OWN + 'tests/test_gpu_param_stats.py',
    'eval_ema': 'which weights training() evaluates, ' + _OWN + 'tests/test_gpu_ema.py',
    'clip_weight_norm': 'per-clip loss weights, ' + _OWN + 'tests/test_gpu_clip_weights.py, test_host_clip_weights.py',
    'class_balance': 'per-clip loss weights of training(), ' + _OWN + 'tests/test_host_clip_weights.py',
    'clip_grad_norm': 'FusedAdam feature, ' + _OWN + 'tests/test_gpu_clip.py, test_host_clip.py',
}

# ---- the shapes (full default dimensions: J = 512, 6912-d) and the rows each runs ---------------------------------------------
_ALL = tuple(rid for rid, _ in ROWS)
SHAPES = {
    #      recipe        B   T   R   rows                                                                     recorded
    'S1': ('int_rel_ch', 4, 8, 18, _ALL, True),                                   # n = 32: staged gate, gemm_p2 tier; part of 576 context rows masked
    'S2': ('int_rel_ch', 8, 16, 18, ('default', 'gate_q32', 'gate_stage_on_side', 'wgrad_side_stream'), False),   # n = 128: gemm_p3 tier
    'S3': ('int_rel_ch', 3, 5, 18, ('default', 'all_flags_off', 'all_flipped'), False),                          # n = 15: no gate workspace, ragged row blocks
    # R = 65: no sign bits, H1_c kept -- and no q32b layer 1: the library declines a pooled head with R > 64, so the model asks for no
    # workspace and a recorded step folds no update (it did, and was refused: recorded here for that)
    'S4': ('int_rel_ch', 2, 16, 65, ('default',), True),
    'S5': ('int_rels', 32, 1, 18, ('default',) + SINGLE_FLIPS, True),                                              # no max over tracks
    'S6': ('int_ch', 4, 8, 0, ('default', 'layer1_planes', 'wgrad_side_stream', 'adam_on_side_stream'), False),   # no context head, no gate
}
CASES = [(s, rid) for s, spec in SHAPES.items() for rid in spec[4]]
