"""ctypes binding of ``liblirec_hip.so`` (C ABI: include/lirec_hip.h).

The library is the product's only compute path: there is no PyTorch or CPU
fallback.  ``lib()`` raises if the shared object is missing (run
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C lirec_amd/csrc``),
and every call checks the returned status code.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LIREC_LIB_PATH: another build of the same library -- the host-side sanitizer build of tests/test_host_asan.py)
LIB_PATH = os.environ.get('LIREC_LIB_PATH') or os.path.join(_HERE, 'liblirec_hip.so')
MAX_SEG = 4
DEFAULT_GEMM_MODE = 2          # 0 exact f32-input MFMA, 1 naive cross-check, 2 split-precision bf16x3 MFMA (default), 3 single-pass bf16 on the large GEMMs

SITE_H1_INTS, SITE_H1_CTX, SITE_E_INTS, SITE_E_CTX, SITE_GATE, SITE_TRACK_SAMPLE, SITE_CONTEXT_DRAW = 0, 1, 2, 3, 4, 5, 6
ABI_VERSION = 124
LIREC_EINVAL = 10001

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class RowSel(C.Structure):
    _fields_ = [('group', _i32), ('group_stride', _i32), ('group_off', _i32)]


class Dropout(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('p', _f32), ('site', _i32), ('site2', _i32), ('seed_dev', _vp)]


class EmbedFwdArgs(C.Structure):
    _fields_ = [('X', _vp), ('ldx', _i64),
                ('W1', _vp * MAX_SEG), ('b1', _vp * MAX_SEG), ('W2', _vp * MAX_SEG), ('b2', _vp * MAX_SEG),
                ('H1', _vp), ('Z2', _vp), ('ldz2', _i64), ('Tn', _vp), ('ldtn', _i64),
                ('mask', _vp), ('Hbar', _vp), ('fscale', _vp),
                ('rowmap', _vp), ('cstart', _vp), ('count', _vp), ('wts', _vp),
                ('in_off', _i32 * MAX_SEG), ('in_dim', _i32 * MAX_SEG), ('out_dim', _i32 * MAX_SEG),
                ('rows', _i32), ('nseg', _i32), ('J', _i32), ('epilogue', _i32),
                ('R', _i32), ('clamp_zero', _i32),
                ('sel', RowSel), ('drop', Dropout), ('x_bf16', _i32), ('parts', _i32),
                ('planes', _vp), ('planes_bytes', _i64), ('pieces', _vp), ('hbits', _vp), ('x_q32', _i32), ('rows_staged', _i32),
                ('W1q', _vp * MAX_SEG)]


class EmbedBwdArgs(C.Structure):
    _fields_ = [('X', _vp), ('ldx', _i64), ('W2', _vp * MAX_SEG), ('H1', _vp), ('dZ2', _vp), ('lddz2', _i64),
                ('dW1', _vp * MAX_SEG), ('db1', _vp * MAX_SEG), ('dW2', _vp * MAX_SEG), ('db2', _vp * MAX_SEG),
                ('workspace', _vp), ('workspace_bytes', _i64),
                ('mask', _vp), ('Hbar', _vp), ('fscale', _vp),
                ('rowmap', _vp), ('cstart', _vp), ('count', _vp), ('wts', _vp),
                ('in_off', _i32 * MAX_SEG), ('in_dim', _i32 * MAX_SEG), ('out_dim', _i32 * MAX_SEG),
                ('rows', _i32), ('nseg', _i32), ('J', _i32), ('parts', _i32),
                ('R', _i32), ('clamp_zero', _i32),
                ('sel', RowSel), ('drop', Dropout), ('x_bf16', _i32), ('reserved2_', _i32),
                ('planes', _vp), ('planes_bytes', _i64), ('hbits', _vp), ('pieces', _vp), ('x_q32', _i32), ('reserved3_', _i32),
                ('adam', _vp)]


class FusedAdamArgs(C.Structure):
    """lirec_fused_adam: the first-layer parameters' update folded into the weight-gradient reduce (include/lirec_hip.h)."""
    _fields_ = [('p', _vp), ('g', _vp), ('m', _vp), ('v', _vp), ('wq', _vp), ('wq_first', _i64), ('n', _i64), ('n_params', _i64),
                ('step', _i32), ('lr', _f32), ('beta1', _f32), ('beta2', _f32), ('eps', _f32), ('weight_decay', _f32),
                ('grad_scale', _f32), ('step_dev', _vp)]


class EmbedDxArgs(C.Structure):
    """lirec_embed_dx_args (ABI 123): the input-feature gradient of the first layers"""
    _fields_ = [('heads', C.POINTER(EmbedBwdArgs) * 2), ('nh', _i32), ('out_bf16', _i32), ('W1', (_vp * MAX_SEG) * 2),
                ('dX', _vp), ('ldx', _i64), ('n', _i32), ('rp1', _i32), ('D', _i32), ('reserved_', _i32)]


class MarginLossArgs(C.Structure):
    _fields_ = [('ints', _vp), ('ld_ints', _i64), ('rels', _vp), ('ld_rels', _i64),
                ('mem', _vp), ('w', _vp), ('y', _vp), ('r', _vp), ('g', _vp), ('sel', _vp),
                ('d_ints', _vp), ('ld_dints', _i64), ('d_rels', _vp), ('ld_drels', _i64),
                ('loss', _vp), ('partial', _vp), ('sel_out', _vp),
                ('B', _i32), ('T', _i32), ('C', _i32), ('NR', _i32),
                ('margin', _f32), ('lymbda', _f32),
                ('max_neg', _i32), ('tr_correct', _i32), ('mask_inplace', _i32), ('rels_mean_valid', _i32),
                ('loader_types', _i32), ('sample', _i32),
                ('sample_seed', C.c_uint64), ('sample_seed_dev', _vp), ('probs_out', _vp), ('arrive', _vp),
                ('batch_divisor', _f32), ('rels_divisor', _f32), ('divisors_dev', _vp), ('y_stride', _i32), ('reserved_', _i32)]


class ClipWeights(C.Structure):
    """lirec_clip_weights: per-clip weights and per-clip loss values of the fused losses"""
    _fields_ = [('w', _vp), ('w_f64', _i32), ('norm', _i32), ('clip_loss', _vp)]


CLIP_WEIGHT_NORMS = {'sum': 0, 'count': 1}


class Pieces(C.Structure):
    """lirec_pieces: the de-duplicated piece tables and the index of a batch (lirec_amd/features.py)."""
    _fields_ = [('clip', _vp), ('ld_clip', _i64), ('n_clip', _i32), ('track', _vp), ('ld_track', _i64), ('n_track', _i32),
                ('index', _vp), ('text_dim', _i32), ('visual_dim', _i32), ('track_dim', _i32),
                ('clip_q', _vp), ('track_q', _vp), ('clip_rows', _vp), ('track_rows', _vp)]


class EmbedDxIndexedArgs(C.Structure):
    """lirec_embed_dx_indexed_args (ABI 124): the gradient of the piece tables"""
    _fields_ = [('heads', C.POINTER(EmbedBwdArgs) * 2), ('nh', _i32), ('reserved_', _i32), ('S', _vp * 2),
                ('W1', (_vp * MAX_SEG) * 2), ('pieces', C.POINTER(Pieces)),
                ('dClip', _vp), ('ld_clip', _i64), ('dTrack', _vp), ('ld_track', _i64)]


class AdamRange(C.Structure):
    """lirec_adam_range: one range of the flat buffers and the steps its parameters sat out (lirec_adam_step_ranges)"""
    _fields_ = [('offset', _i64), ('length', _i64), ('lag', _i32), ('reserved_', _i32)]


class AdamHyper(C.Structure):
    """lirec_adam_hyper: one row of a table of per-group hyper-parameters in device memory (32 bytes)"""
    _fields_ = [('lr', _f32), ('beta1', _f32), ('beta2', _f32), ('eps', _f32), ('weight_decay', _f32), ('decoupled', _f32),
                ('reserved_', _f32 * 2)]


class AdamGroupRange(C.Structure):
    """lirec_adam_group_range: lirec_adam_range with the group whose row of the table the range is updated with"""
    _fields_ = [('offset', _i64), ('length', _i64), ('lag', _i32), ('group', _i32)]


ADAM_MAX_GROUPS = 8           # LIREC_ADAM_MAX_GROUPS
ADAM_MAX_RANGES = 64
ADAM_MAP_MAX = 16             # LIREC_ADAM_MAP_MAX: the entries of lirec_set_adam_hyper_map
CLIP_PARTIALS = 1024          # LIREC_CLIP_PARTIALS: the doubles lirec_grad_sq_partials writes
EMA_MAX_BLOCKS = 2048         # LIREC_EMA_MAX_BLOCKS: the grid cap of lirec_ema_step (256 threads x one f32x4 a workgroup and pass)


class ParamStatEntry(C.Structure):
    """lirec_param_stat_entry: one range of the flat buffers and the column groups asked of it (lirec_param_stats)"""
    _fields_ = [('offset', _i64), ('length', _i64), ('flags', _i32), ('inv_bc1', _f32), ('inv_sqrt_bc2', _f32), ('eps', _f32)]


PARAM_STATS_MAX_RANGES = 64   # LIREC_PARAM_STATS_MAX_RANGES
PARAM_STATS_COLS = 9          # LIREC_PARAM_STATS_COLS: (sum of squares, largest magnitude, non-finite count) x (gradient, parameter, update)
STAT_GRAD, STAT_PARAM, STAT_UPDATE = 1, 2, 4      # lirec_param_stat_entry::flags


class LinearFwdArgs(C.Structure):
    _fields_ = [('A', _vp), ('lda', _i64), ('W', _vp), ('b', _vp), ('Y', _vp), ('ldy', _i64),
                ('n', _i32), ('K', _i32), ('N', _i32), ('reserved_', _i32)]


class LinearBwdArgs(C.Structure):
    _fields_ = [('dY', _vp), ('lddy', _i64), ('A', _vp), ('lda', _i64), ('W', _vp), ('dW', _vp), ('db', _vp), ('dA', _vp),
                ('ldda', _i64), ('act', _vp), ('ldact', _i64), ('n', _i32), ('K', _i32), ('N', _i32), ('mode', _i32),
                ('accumulate', _i32), ('parts', _i32), ('drop', Dropout)]


class EvalArgs(C.Structure):
    _fields_ = [('ints', _vp), ('ld_ints', _i64), ('rels', _vp), ('ld_rels', _i64), ('mem', _vp), ('y', _vp), ('r', _vp),
                ('g', _vp), ('just_zeros', _vp), ('counters', _vp), ('B', _i32), ('T', _i32), ('C', _i32), ('NR', _i32),
                ('loader_types', _i32), ('reserved_', _i32)]


class EvalTopkArgs(C.Structure):
    """lirec_eval_topk_args: the clip-level top-k counters (lirec_eval_clip_topk)"""
    _fields_ = [('logits', _vp), ('ld_logits', _i64), ('y', _vp), ('y_stride', _i64), ('soft', _vp), ('ld_soft', _i64),
                ('counters', _vp), ('conf', _vp), ('B', _i32), ('C', _i32), ('n_soft', _i32), ('loader_types', _i32)]


EVAL_TOPK_MAX_C = 4096        # LIREC_EVAL_TOPK_MAX_C


class PredictArgs(C.Structure):
    """lirec_predict_args: per-clip predictions without labels (lirec_predict_clips)"""
    _fields_ = [('ints', _vp), ('ld_ints', _i64), ('rels', _vp), ('ld_rels', _i64), ('mem', _vp),
                ('trk', _vp), ('cls', _vp), ('rel', _vp), ('score', _vp), ('trk_score', _vp),
                ('top_cls', _vp), ('top_cls_p', _vp), ('top_rel', _vp), ('top_rel_p', _vp), ('flags', _vp),
                ('B', _i32), ('T', _i32), ('C', _i32), ('NR', _i32), ('K', _i32), ('loader_types', _i32)]


PREDICT_MAX_K = 16            # LIREC_PREDICT_MAX_K
COLLATE_MAX_FIELDS = 16       # LIREC_COLLATE_MAX_FIELDS


class CollateField(C.Structure):
    _fields_ = [('src', _vp), ('row_bytes', _i64), ('dst', _vp)]


class CollateArgs(C.Structure):
    """lirec_collate_args: a resident-store batch buffer written by the device (lirec_collate_resident)"""
    _fields_ = [('ids', _vp), ('index_rows', _vp), ('feature_index', _vp), ('clip_rows', _vp), ('track_rows', _vp), ('counts', _vp),
                ('workspace', _vp), ('workspace_bytes', _i64), ('n_clip_all', _i64), ('n_track_all', _i64), ('n_clip_list', _i64),
                ('n_track_list', _i64), ('B', _i32), ('E', _i32), ('nf', _i32), ('reserved_', _i32),
                ('fields', CollateField * COLLATE_MAX_FIELDS)]


class DrawContextArgs(C.Structure):
    """lirec_draw_context_args: the per-epoch draw from over-long context lists, in place in the resident index (lirec_draw_context)"""
    _fields_ = [('slot_dst', _vp), ('slot_off', _vp), ('pool_rows', _vp), ('index_rows', _vp), ('seed', C.c_uint64),
                ('epoch', C.c_uint32), ('S', _i32), ('R', _i32), ('E', _i32)]


CONTEXT_LIST_MAX = 4096       # LIREC_CONTEXT_LIST_MAX


class FeatureRows(C.Structure):
    """lirec_feature_rows: the batch's sample ids into a resident block store (lirec_set_feature_rows)"""
    _fields_ = [('clip_ids', _vp), ('n_clips', _i32), ('rows_per_clip', _i32), ('store_rows', _i64)]


FEATURE_ROWS_MAX = 2147483616  # LIREC_FEATURE_ROWS_MAX: the most rows a q32b store may hold (int32 row lists)


class LirecError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes)
_PROTOS = {
    'lirec_version': (_i32, []),
    'lirec_abi_sizeof': (_i32, [_i32]),
    'lirec_set_gemm_mode': (_i32, [_i32]),
    'lirec_get_gemm_mode': (_i32, []),
    'lirec_set_grad_overwrite': (_i32, [_i32]),
    'lirec_grad_overwrite_conflicts': (_i32, []),
    'lirec_ctx_create': (_i32, [C.POINTER(_vp)]),
    'lirec_ctx_destroy': (_i32, [_vp]),
    'lirec_ctx_set_current': (_i32, [_vp]),
    'lirec_ctx_get_current': (_vp, []),
    'lirec_debug_set': (_i32, [_i32, _i32]),
    'lirec_record_begin': (_i32, []),
    'lirec_record_mark': (_i32, []),
    'lirec_record_end': (_i32, [C.POINTER(_vp)]),
    'lirec_cmdlist_size': (_i32, [_vp]),
    'lirec_cmdlist_replay': (_i32, [_vp, _i32, _i32]),
    'lirec_cmdlist_replay_lagged': (_i32, [_vp, _i32, _i32, _i32, _i64]),
    'lirec_cmdlist_command': (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(_i32)]),
    'lirec_cmdlist_destroy': (_i32, [_vp]),
    'lirec_stream_wait': (_i32, [_vp, _vp]),
    'lirec_stream_wait_many': (_i32, [C.POINTER(C.c_void_p), _i32, _vp]),
    'lirec_memset_zero': (_i32, [_vp, _i64, _vp]),
    'lirec_zero_count': (_i32, [_vp, _i64, _vp, C.POINTER(C.c_int64), _i32, _vp]),
    'lirec_snapshot': (_i32, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int64), _i32, _vp, _vp]),
    'lirec_error_string': (C.c_char_p, [_i32]),
    'lirec_workspace_bytes': (_i64, [_i32, _i32, _i32]),
    'lirec_planes_bytes': (_i64, [_i32, _i32, _i32, _i32]),
    'lirec_hbits_bytes': (_i64, [_i32, _i32]),
    'lirec_q32b_bytes': (_i64, [_i64, _i64]),
    'lirec_to_q32b': (_i32, [_vp, _i64, _i64, _i64, _vp, _vp]),
    'lirec_q16b_bytes': (_i64, [_i64, _i64]),
    'lirec_to_q16b': (_i32, [_vp, _i64, _i64, _i64, _vp, _vp]),
    'lirec_to_q16c': (_i32, [_vp, _i64, _i64, _i64, _vp, _vp]),
    'lirec_q32b_write_rows': (_i32, [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp]),
    'lirec_set_feature_rows': (_i32, [C.POINTER(FeatureRows)]),
    'lirec_embed_fwd': (_i32, [C.POINTER(EmbedFwdArgs), _vp]),
    'lirec_embed_bwd': (_i32, [C.POINTER(EmbedBwdArgs), _vp]),
    'lirec_embed_fwd2': (_i32, [C.POINTER(EmbedFwdArgs), C.POINTER(EmbedFwdArgs), _vp]),
    'lirec_embed_dw1_indexed': (_i32, [C.POINTER(C.POINTER(EmbedBwdArgs)), _i32, C.POINTER(Pieces), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    'lirec_embed_l1_indexed': (_i32, [C.POINTER(C.POINTER(EmbedFwdArgs)), _i32, C.POINTER(Pieces), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    'lirec_embed_bwd2': (_i32, [C.POINTER(EmbedBwdArgs), C.POINTER(EmbedBwdArgs), _vp]),
    'lirec_embed_dx': (_i32, [C.POINTER(EmbedDxArgs), _vp]),
    'lirec_embed_dx_indexed': (_i32, [C.POINTER(EmbedDxIndexedArgs), _vp]),
    'lirec_linear_fwd_group': (_i32, [C.POINTER(LinearFwdArgs), _i32, _vp]),
    'lirec_linear_bwd_group': (_i32, [C.POINTER(LinearBwdArgs), _i32, _vp]),
    'lirec_compact_rows': (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    'lirec_compact_rows2': (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    'lirec_pool_fwd': (_i32, [_vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i64, C.POINTER(Dropout), _vp]),
    'lirec_pool_bwd': (_i32, [_vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    'lirec_gate_fwd': (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _i64, C.POINTER(Dropout), _vp]),
    'lirec_gate_bwd': (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64,
                              _i32, C.POINTER(Dropout), _i32, _i32, _vp]),
    'lirec_gate_bwd_parts': (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64,
                                    _i32, C.POINTER(Dropout), _i32, _i32, _i32, _vp]),
    'lirec_gate_ws_bytes': (_i64, [_i32, _i32, _i32]),
    'lirec_gate_fwd_ws': (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _i64, C.POINTER(Dropout), _vp, _i64, _i32, _vp]),
    'lirec_gate_stage_weights': (_i32, [_vp, _i32, _i32, _i32, _vp, _i64, _vp]),
    'lirec_gate_bwd_ws': (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64,
                                 _i32, C.POINTER(Dropout), _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    'lirec_linear_fwd': (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp]),
    'lirec_linear_bwd': (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i64,
                                _i32, C.POINTER(Dropout), _vp]),
    'lirec_margin_loss': (_i32, [C.POINTER(MarginLossArgs), _vp]),
    'lirec_heads_loss_fwd_bwd': (_i32, [C.POINTER(LinearFwdArgs), C.POINTER(LinearBwdArgs), _i32, C.POINTER(MarginLossArgs), _vp]),
    'lirec_ce_loss': (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _f32, _f32, _vp, _vp]),
    'lirec_margin_loss_weighted': (_i32, [C.POINTER(MarginLossArgs), C.POINTER(ClipWeights), _vp]),
    'lirec_heads_loss_fwd_bwd_weighted': (_i32, [C.POINTER(LinearFwdArgs), C.POINTER(LinearBwdArgs), _i32, C.POINTER(MarginLossArgs),
                                                 C.POINTER(ClipWeights), _vp]),
    'lirec_ce_loss_weighted': (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _f32, _f32,
                                      _vp, C.POINTER(ClipWeights), _vp]),
    'lirec_adam_step': (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _f32, _f32, _f32, _f32, _f32, _vp, _vp]),
    'lirec_adam_step_counted': (_i32, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _i32, _vp]),
    'lirec_adam_step_ranges': (_i32, [_vp, _vp, _vp, _vp, C.POINTER(AdamRange), _i32, _i32, _f32, _f32, _f32, _f32, _f32, _f32,
                                      _vp, _vp, _vp, _i32, _vp]),
    'lirec_adam_hyper_write': (_i32, [_vp, C.POINTER(AdamHyper), _i32, _vp]),
    'lirec_adam_step_groups': (_i32, [_vp, _vp, _vp, _vp, C.POINTER(AdamGroupRange), _i32, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _i32,
                                      _vp]),
    'lirec_set_adam_hyper_row': (_i32, [_vp]),
    'lirec_set_adam_hyper_map': (_i32, [_vp, C.POINTER(AdamGroupRange), _i32]),
    'lirec_counter_add': (_i32, [_vp, C.POINTER(C.c_int64), _i32, _vp]),
    'lirec_grad_sq_partials': (_i32, [_vp, C.POINTER(AdamRange), _i32, _vp, _vp]),
    'lirec_clip_finalize': (_i32, [_vp, _vp, _i32, _f32, _f32, _vp, _vp]),
    'lirec_set_adam_clip': (_i32, [_vp]),
    'lirec_clip_finalize_guard': (_i32, [_vp, _vp, _i32, _f32, _f32, _vp, _vp, _i32, _vp]),
    'lirec_set_adam_guard': (_i32, [_vp, _vp]),
    'lirec_accum_begin': (_i32, [_vp, _i64, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i32, _vp, _i32, _vp]),
    'lirec_set_adam_hold': (_i32, [_vp, _i32]),
    'lirec_ema_step': (_i32, [_vp, _vp, _i64, _f32, _vp, _vp]),
    'lirec_param_stats_ws_bytes': (_i64, [_i32]),
    'lirec_param_stats': (_i32, [_vp, _vp, _vp, _vp, C.POINTER(ParamStatEntry), _i32, _vp, _vp, _i64, _vp]),
    'lirec_eval_max_tracks': (_i32, [C.POINTER(EvalArgs), _vp]),
    'lirec_eval_clip_topk': (_i32, [C.POINTER(EvalTopkArgs), _vp]),
    'lirec_predict_clips': (_i32, [C.POINTER(PredictArgs), _vp]),
    'lirec_predict_clips_at': (_i32, [C.POINTER(PredictArgs), _vp, _vp]),
    'lirec_rows_copy_at': (_i32, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp]),
    'lirec_scalar_accumulate': (_i32, [_vp, _i32, _vp, _vp]),
    'lirec_collate_workspace_bytes': (_i64, [_i64, _i64]),
    'lirec_collate_resident': (_i32, [C.POINTER(CollateArgs), _vp]),
    'lirec_collate_fields': (_i32, [_vp, _i32, C.POINTER(CollateField), _i32, _vp]),
    'lirec_collate_fields_at': (_i32, [_vp, _vp, _i32, C.POINTER(CollateField), _i32, _vp]),
    'lirec_draw_context': (_i32, [C.POINTER(DrawContextArgs), _vp]),
    'lirec_cast_f64_f32': (_i32, [_vp, _vp, _i64, _vp]),
    'lirec_grid_pool': (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i64, _vp]),
    'lirec_rows_max': (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _vp, _i64, _vp]),
    'lirec_gather_features': (_i32, [_vp, _i64, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _i64, _vp]),
    'lirec_gather_features_bf16': (_i32, [_vp, _i64, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _i64, _vp]),
    'lirec_dropout_mask': (_i32, [_vp, _i32, _i32, C.POINTER(Dropout), _i32, _vp]),
    'lirec_set_scratch': (_i32, [_vp, _i64]),
    'lirec_profile_enable': (_i32, [_i32]),
    'lirec_profile_sites': (_i32, []),
    'lirec_profile_site_name': (C.c_char_p, [_i32]),
    'lirec_profile_read': (_i32, [_i32, C.POINTER(C.c_double), C.POINTER(_i64), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]),
}

EXPORTS = tuple(_PROTOS)


def _bind_torch_hip_runtime():
    """PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so); device pointers and
    streams are only meaningful inside the runtime that created them, so the library's hip*
    symbols must resolve to that same instance.  Importing torch and re-opening its runtime
    RTLD_GLOBAL *before* our dlopen puts it first in the lookup scope (our DT_NEEDED on the
    system libamdhip64.so.7 then stays unused).  A non-torch host links the system runtime."""
    try:
        import torch
    except ImportError:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load (once) and return the shared library; fail loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LirecError('HIP extension %s not found: build it first (python -c "import __graft_entry__ as g; '
                         'g.build()"). There is no fallback path.' % LIB_PATH)
    _bind_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(L, name)          # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    for which, st in list(enumerate((EmbedFwdArgs, EmbedBwdArgs, MarginLossArgs, Dropout, RowSel))) + [(8, EmbedDxArgs),
                                                                                                      (9, EmbedDxIndexedArgs),
                                                                                                      (10, AdamRange), (11, AdamHyper),
                                                                                                      (12, AdamGroupRange), (13, EvalTopkArgs),
                                                                                                      (15, PredictArgs), (17, CollateArgs),
                                                                                                      (19, ClipWeights), (21, FeatureRows),
                                                                                                      (23, CollateField), (41, DrawContextArgs),
                                                                                                      (43, ParamStatEntry)]:
        if L.lirec_abi_sizeof(which) != C.sizeof(st):
            raise LirecError('ABI mismatch for %s: library %d bytes, binding %d bytes'
                             % (st.__name__, L.lirec_abi_sizeof(which), C.sizeof(st)))
    mode = os.environ.get('LIREC_GEMM_MODE', str(DEFAULT_GEMM_MODE))
    if L.lirec_set_gemm_mode(int(mode)) != 0:
        raise LirecError('LIREC_GEMM_MODE=%s is not a valid GEMM core (0 f32 MFMA, 1 naive, 2 bf16x3, 3 single-pass bf16)' % mode)
    _lib = L
    return L


def default_gemm_mode() -> int:
    return int(os.environ.get('LIREC_GEMM_MODE', DEFAULT_GEMM_MODE))


_calls = [0]          # library calls checked so far (lirec_amd.graph uses it to tell an empty capture segment)


def check(code: int, what: str = ''):
    _calls[0] += 1
    if code != 0:
        msg = lib().lirec_error_string(code)
        raise LirecError('%s failed: %s (code %d)' % (what or 'lirec call', msg.decode() if msg else '?', code))
