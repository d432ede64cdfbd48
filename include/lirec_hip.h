/*
 * lirec_hip.h -- C ABI of the MI355X (gfx950) hot-path library for LIReC.
 *
 * The reference (Annusha/LIReC) has no FFI layer: its hot path is the Python
 * object protocol between mlp/train.py / mlp/test.py and mlp/model.py, executed
 * by ATen.  Each entry point below replaces the ATen op sequence of one region
 * of mlp/model.py (cited per function; paths relative to the reference).  The
 * Python host (lirec_amd/) binds these with ctypes and keeps the reference's
 * create_model / model(batch) / loss(out, batch) protocol on top.
 *
 * Conventions
 *   - extern "C"; plain pointers and sizes; no torch types.
 *   - every function returns 0 on success or a hipError_t / LIREC_E* code; never throws.
 *   - all pointers are DEVICE pointers unless stated; the caller owns every buffer;
 *     nothing is allocated inside (scratch comes in through `workspace`, sized by
 *     lirec_workspace_bytes); every call is enqueued on `stream` and returns
 *     without synchronising.
 *   - matrices are row-major fp32; `ld*` are row strides in elements.
 *   - Linear weights are [out, in] row-major with a bias of [out], as
 *     torch.nn.Linear stores them (state_dict layout).
 *   - gradient outputs ACCUMULATE (+=) into the caller's gradient buffers, like
 *     autograd's .grad accumulation; zero them with hipMemsetAsync between steps.
 *   - dropout masks come from a counter-based generator (Philox4x32-10): element
 *     (row, col) of dropout site s is kept iff word[row & 3] of
 *     philox(counter = (col, row >> 2, s, 0), key = seed) >= floor(p * 2^32); kept values
 *     are scaled by 1/(1-p) (torch.nn.Dropout train-mode semantics, mlp/model.py:52).
 *     p == 0 (eval mode) disables it.
 */
#ifndef LIREC_HIP_H
#define LIREC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lirec_stream_t;            /* hipStream_t */
typedef void* lirec_ctx_t;               /* library context (lirec_ctx_create); NULL = the default context */

#define LIREC_VERSION 124                /* 0.1.9 */
#define LIREC_MAX_SEG 4

enum {
  LIREC_OK = 0,
  LIREC_EINVAL = 10001,                  /* bad argument (null pointer, size <= 0, unsupported combination) */
  LIREC_EWORKSPACE = 10002               /* workspace too small */
};

/* dropout sites (one counter stream each) */
enum { LIREC_SITE_H1_INTS = 0, LIREC_SITE_H1_CTX = 1, LIREC_SITE_E_INTS = 2,
       LIREC_SITE_E_CTX = 3, LIREC_SITE_GATE = 4,
       LIREC_SITE_TRACK_SAMPLE = 5,      /* the uniform draw of the positive-track sampler (lirec_margin_loss, sample) */
       LIREC_SITE_CONTEXT_DRAW = 6 };    /* the per-epoch draw from over-long context lists (lirec_draw_context) */

/* Row selection inside the feature block.  Logical row n of an operand maps to
 * physical row (n / group) * group_stride + (n % group) + group_off of the
 * (B*T, R+1, D) feature tensor: the interaction head reads row 0 of every
 * candidate (group=1, stride=R+1, off=0; mlp/model.py:279), the context head rows
 * 1..R (group=R, stride=R+1, off=1; mlp/model.py:305).  group == 0 means identity. */
typedef struct {
  int32_t group, group_stride, group_off;
} lirec_rowsel;

typedef struct {
  uint64_t seed;                          /* Philox key */
  float p;                                /* drop probability; 0 disables */
  int32_t site;                           /* LIREC_SITE_* of the first-layer activation */
  int32_t site2;                          /* site of the embedding dropout (embed epilogue 1 / pool) */
  const uint64_t* seed_dev;               /* optional device counter: the key is seed + *seed_dev, read by the kernels.
                                           * Lets a recorded train step (command list) draw new masks on every replay
                                           * (lirec_counter_add inside the graph); NULL = seed alone */
} lirec_dropout;

/* ---- embedding MLPs -----------------------------------------------------
 * Replaces, for one head h in {ints, ctx}, the four two-layer branches
 *   Lin -> dropout -> relu -> Lin      (mlp/model.py:279-294 / :305-322,
 *                                       :152-167 / :177-194, :59-76)
 * on `rows` logical rows of X selected by `sel`.
 * Segment s reads X[:, in_off[s] : in_off[s]+in_dim[s]], first layer W1[s]
 * [J, in_dim[s]], second layer W2[s] [out_dim[s], J].
 *   H1 [rows, nseg*J]   = relu(dropout(X_s W1_s^T + b1_s))    (saved for backward)
 *   Z2 [rows, sum out_dim] at (Z2, ldz2):
 *       epilogue 0: Z2 = H1_s W2_s^T + b2_s
 *       epilogue 1: Tn = tanh(Z2) -> Tn_out; Z2 := dropout(Tn)  (cat -> tanh -> dropout, mlp/model.py:296-297,
 *                                                                :326-327; dropout site = drop.site2)
 *
 * Pooled form (context head, mask != NULL): rows = n*R.  The masked mean over the R context
 * clips of a candidate (mlp/model.py:309,315,323-324) is linear and sits directly behind the
 * second Linear, so it is moved in front of it -- exact algebra, 1/R of the layer-2 work:
 *   Hbar[c,:] = sum_r mask[c,r] H1[c,r,:] / div[c]     (the pooling pass, now over H1)
 *   f[c]      = (sum_r mask[c,r]) / div[c]              (1, or 0 for an all-masked candidate with
 *                                                        clamp_zero; NaN without it, as the reference)
 *   Z2[c,:]   = Hbar[c,:] W2^T + f[c] b2                (n rows), then the epilogue as above
 *   with div = sum_r mask (clamp_zero: 0 -> 1, mlp/model.py:303; MidFusionMultiClip has none, :175).
 */
struct lirec_pieces_s;                    /* piece tables + index (defined with lirec_embed_l1_indexed below) */
typedef struct {
  const float* X; int64_t ldx;
  const float* W1[LIREC_MAX_SEG]; const float* b1[LIREC_MAX_SEG];
  const float* W2[LIREC_MAX_SEG]; const float* b2[LIREC_MAX_SEG];
  float* H1;                              /* [rows, nseg*J], ld = nseg*J */
  float* Z2; int64_t ldz2;
  float* Tn; int64_t ldtn;                /* epilogue 1 only */
  const float* mask;                      /* pooled form: fp32 [n, R]; NULL = plain form */
  float* Hbar;                            /* pooled form: [n, nseg*J] out (saved for backward) */
  float* fscale;                          /* pooled form: [n] out (saved for backward) */
  /* compact pooled form (all three from lirec_compact_rows, or all NULL): only the context rows with
   * a non-zero mask are run through layer 1; H1 then holds one row per VALID context row, in rowmap
   * order (allocate it for n*R rows; the tail is left untouched). */
  const int32_t* rowmap; const int32_t* cstart; const int32_t* count;
  const float* wts;                       /* compact form, optional: the mask value of each compact row (lirec_compact_rows2);
                                           * when given, `mask` may be NULL */
  int32_t in_off[LIREC_MAX_SEG], in_dim[LIREC_MAX_SEG], out_dim[LIREC_MAX_SEG];
  int32_t rows, nseg, J, epilogue;
  int32_t R, clamp_zero;                  /* pooled form */
  lirec_rowsel sel;
  lirec_dropout drop;
  /* 1: X is stored as bf16 (ldx in elements; BASELINE config 5 "bf16 storage"): half the feature bytes, and the
   * split-precision core runs two MFMAs per product instead of three (X has no low part).  Default core only.
   * With `planes` (lirec_planes_bytes(.., x_mode = 1); ABI 119) the staging launch copies the valid rows into q16b there and the
   * one-plane persistent kernels read them: bit-identical to the block stored as q16b (x_q32 = 2). */
  int32_t x_bf16;
  int32_t parts;                          /* 0: the whole call; 1: layer 1 (+ the pooling pass of the pooled form) only; 2: layer 2 only; 3: the pooling
                                           * pass + layer 2 (layer 1 done elsewhere: lirec_embed_l1_indexed); 4: stage the ROWS into `planes` and nothing
                                           * else (see rows_staged); lirec_embed_fwd2 wants the same value in both */
  /* Optional workspace (lirec_planes_bytes) for the PRE-SPLIT bf16 operand planes of layer 1.  When given (default GEMM
   * core, segments adjacent in the feature row, in_dim % 32 == 0, J % 128 == 0, aligned X; pooled form: R <= 64) the forward first writes the
   * selected feature rows as dense hi / lo bf16 planes -- compacted, when the compact form is used -- and the first-layer
   * weights likewise, and layer 1 runs on those planes with LDS-DMA staging (no conversion in the k-loop; same three
   * MFMAs per product, bit-identical results).  The backward call must be handed the same buffer: the weight gradient
   * reads the feature planes again.  NULL: operands are split on the fly per k-tile. */
  void* planes; int64_t planes_bytes;
  /* Optional, with `planes` only (ABI 115): the feature rows come as PIECE TABLES + INDEX (the inputs of lirec_gather_features:
   * text | clip-visual | track-1 | track-2, nseg = 4, in_off[0] = 0) instead of X -- the staging pass writes the q32b rows of
   * layer 1 straight from the tables, the (B, T, R+1, D) block is never built and X may be NULL.  The row selector then
   * addresses index rows.  The backward call gets the same `planes` buffer and needs neither X nor the pieces.  When the
   * q32b form does not apply the call fails with LIREC_EINVAL (use lirec_embed_l1_indexed). */
  const struct lirec_pieces_s* pieces;
  /* Optional, pooled form only (ABI 118): lirec_hbits_bytes(rows, nseg * J) bytes.  The pooling pass, which reads every valid row
   * of H1 anyway, also leaves one bit per element, [H1 > 0] -- all that backward needs of H1 (the relu / dropout derivative in the
   * un-pooling pass: relu(dropout(z)) > 0 <=> kept and z > 0).  Hand the same buffer to lirec_embed_bwd and H1 need not be kept
   * from forward to backward (151 MB at the bench shape) nor be read again (58 MB).  Needs R <= 64, (nseg * J) % 4 == 0 and
   * 16-byte aligned H1 / Hbar (LIREC_EINVAL otherwise); bit-identical results. */
  void* hbits;
  /* 1 (ABI 118, with `planes`): X is not an fp32 block but the SAME block stored as q32b (lirec_to_q32b: blocked bf16 hi / lo,
   * the fp32 footprint; ldx = its columns, rows padded to 32) -- the storage layer 1 reads.  Nothing is staged: layer 1 and its
   * weight gradient gather their rows from X through a row list the staging launch writes (which then only stages W1 and the
   * dropout keep bytes).  Bit-identical to the staged path.
   * 2 (ABI 119): X is the block stored as q16b (lirec_to_q16b: its values rounded to bf16, blocked, HALF the fp32 footprint --
   * "bf16 feature storage", BASELINE config 5): gathered the same way by the ONE-PLANE forms of the two kernels (the stored value
   * is the hi half of the product's split, there is no lo half: two MFMAs per product instead of three).  Block form only.
   * 3 (ABI 122): X is the block stored as q16c (lirec_to_q16c: the same bf16 values in 32 x 64 blocks of 4 KiB, 128-byte rows) --
   * the storage of the SINGLE-PASS mode (lirec_set_gemm_mode(3)) and of that mode only: its forward kernel takes 64 of k per step,
   * whole 128-byte lines of both operands (rows as q16c, first-layer weights staged -- or kept by the caller, W1q -- as q16c), one
   * MFMA per product.  Mode 3 refuses q16b / q32b rows (LIREC_EINVAL), mode 2 refuses q16c; a row-major bf16 block (x_bf16) is
   * staged in the form of the mode in force.  Block form only; ldx % 64 == 0, segments start at multiples of 64 columns. */
  int32_t x_q32;
  /* 1 (ABI 118): the feature rows, the dropout keep bytes and the partition bound are ALREADY in `planes` -- an earlier call with
   * parts = 4 (same arguments, same `planes`, drop.seed = the key THIS call draws its masks from) put them there, on a stream this
   * one is ordered behind.  The call then stages the first-layer weights only.  That is how a training loop stages the rows of
   * batch t + 1 beside the MFMA-bound backward of batch t (an input pipeline: the rows do not depend on the weights).
   * q32b path only: LIREC_EINVAL where the call would have fallen back to the on-the-fly kernels. */
  int32_t rows_staged;
  /* Optional (ABI 119, with `planes`): W1q[i] = the first-layer weights of segment i ALREADY in the q32b form ([J][in_dim[i]],
   * lirec_to_q32b's layout, 256-byte aligned) -- kept current by the caller: by lirec_to_q32b once, then by the fused update of
   * lirec_embed_bwd_args::adam (lirec_fused_adam::wq).  The staging launch then leaves the weights alone (with rows_staged there is
   * no staging launch at all); all segments or none.  Bit-identical.  (ABI 122) In the single-pass mode the form is q16c
   * (lirec_to_q16c; at the same addresses, the first half of each matrix's bytes) -- made and read under that mode only. */
  const void* W1q[LIREC_MAX_SEG];
} lirec_embed_fwd_args;
int64_t lirec_hbits_bytes(int32_t rows, int32_t W);
int lirec_embed_fwd(const lirec_embed_fwd_args* a, lirec_stream_t stream);
/* Both heads of one model in one call (same results as two lirec_embed_fwd calls): the second layers of the two
 * heads -- small GEMMs on the candidate rows -- share one grouped launch. */
int lirec_embed_fwd2(const lirec_embed_fwd_args* a, const lirec_embed_fwd_args* b, lirec_stream_t stream);

/* Rows of a RESIDENT BLOCK STORE (added to ABI 124 without a new number: new exports and a new struct, index 21 of
 * lirec_abi_sizeof).  A tiled dataset's feature rows are kept once on the device as ONE q32b matrix -- sample s owns storage rows
 * [s * rows_per_clip, (s + 1) * rows_per_clip) -- and a batch is a list of sample ids.  With the setter armed, the X of the next
 * call (x_q32 = 1) is that whole matrix and the call's block is "these n_clips samples of it": batch-local physical row p -- what
 * the lirec_rowsel arithmetic yields -- names
 *   storage row  (int64) clip_ids[p / rows_per_clip] * rows_per_clip + p % rows_per_clip.
 * The staging launch writes that into the row lists layer 1 and its weight gradient gather through (nothing else changes: the
 * backward reads the lists from `planes` and takes no setter; dropout counters keep the BATCH-LOCAL row id, as they do under row
 * compaction, so a mask does not depend on where a sample is stored).  clip_ids is DEVICE memory, read by the kernel through the
 * pointer each time it runs: a recorded launch sees the ids that are there when it is replayed.  TRUSTED, not checked on the
 * device: every id in [0, store_rows / rows_per_clip); duplicates are fine.
 * READ BY: lirec_embed_fwd and lirec_embed_fwd2, parts 0, 1 and 4 (with rows_staged the lists are in `planes` already: the value
 * is checked and otherwise unused).  CONSUMED by the first such call the thread makes after the setter, whether it succeeds or
 * not -- a forgotten one cannot leak into another model's forward; NULL switches it off.  Per calling thread.
 * While armed the call returns LIREC_EINVAL, before any device call and also under the host-side dry run, when: clip_ids is NULL
 * or misaligned, n_clips or rows_per_clip < 1; a head has x_q32 != 1, x_bf16 or `pieces`; the call would not take the gathered
 * q32b path (shapes, planes, GEMM mode); parts is 2 or 3 or a head is empty; a head's `rows` is not a multiple of its per-sample
 * row count (rows_per_clip without a selector; rows_per_clip / group_stride * group with one, rows_per_clip % group_stride == 0);
 * n_clips * rows_per_clip differs from the physical rows of the call (rows, or rows / group * group_stride);
 * store_rows > LIREC_FEATURE_ROWS_MAX.
 * LIMIT: row lists are int32, so a store holds at most LIREC_FEATURE_ROWS_MAX = 2^31 - 32 rows (59 TB at 27 648 B a row: the
 * card's memory is the bound that bites); every byte offset formed from a list entry is 64-bit (gemm_p2.hpp: p2_row_off and the
 * per-lane / scalar addresses built on it), a store may pass 4 GiB. */
#define LIREC_FEATURE_ROWS_MAX 2147483616LL
typedef struct {
  const int32_t* clip_ids;                /* device, [n_clips] */
  int32_t n_clips, rows_per_clip;
  int64_t store_rows;                     /* rows of the q32b matrix at X (multiple of 32) */
} lirec_feature_rows;
int lirec_set_feature_rows(const lirec_feature_rows* rows);

/* Layer 1 on the UNIQUE feature pieces (second half).  A row of the loader's (B, T, R+1, D) block is
 * [clip piece (text | clip-visual) | track-1 piece | track-2 piece] and every piece is shared by many rows
 * (mixed_utils/classification_dataloader.py:336-349, :477-478, :531-533); the first Linear of a modality branch
 * (mlp/model.py:279-292, :305-320) acts on one piece only.  With the tables and the index of lirec_gather_features the
 * pre-activations are computed once per PIECE and expanded per row with that row's dropout mask: H1 -- and everything
 * after it -- is bit-identical to lirec_embed_fwd on the expanded block, which is never built.
 *   heads[h]: the arguments lirec_embed_fwd would get (X ignored; nseg = 4: text, visual, tracks1, tracks2; J % 256 == 0);
 *   zclip[h] [n_clip, 2J], ztrk[h] [n_track, 2J]: caller-provided scratch (kept for nothing: backward does not need it).
 * Does layer 1 only; the caller continues with parts = 3 (pooling pass + layer 2: lirec_embed_fwd / lirec_embed_fwd2). */
typedef struct lirec_pieces_s {
  const float* clip; int64_t ld_clip; int32_t n_clip;       /* [n_clip, text_dim + visual_dim] fp32 */
  const float* track; int64_t ld_track; int32_t n_track;    /* [n_track, track_dim] fp32 */
  const int32_t* index;                                     /* [physical rows, 3]: clip, track-1, track-2 piece (or < 0) */
  int32_t text_dim, visual_dim, track_dim;
  /* Optional (ABI 118): the same tables stored as q32b (lirec_to_q32b; rows n_clip + 1 / n_track + 1 -- the zero row included --
   * padded to 32).  With them (and `planes`) layer 1 and its weight gradient GATHER their rows from the tables through the index:
   * no staged copy of the rows exists, `clip` / `track` may be NULL.  clip_rows / track_rows (optional): a second level for a
   * store of ALL pieces resident in HBM -- an index value v >= 0 then names table row clip_rows[v] / track_rows[v] (v < 0: the
   * zero row n_clip / n_track), so a batch brings two short lists and the index, and no table is cut. */
  const void* clip_q; const void* track_q;
  const int32_t* clip_rows; const int32_t* track_rows;
} lirec_pieces;
/* fp32 [rows][cols] (cols % 32 == 0, 16-byte aligned) -> q32b with the rows padded to a multiple of 32 by zero rows;
 * lirec_q32b_bytes(rows, cols) bytes at dst (256-byte aligned). */
int64_t lirec_q32b_bytes(int64_t rows, int64_t cols);
int lirec_to_q32b(const float* src, int64_t ld_src, int64_t rows, int64_t cols, void* dst, lirec_stream_t stream);
/* `rows` rows of src -> storage rows [dst_row0, dst_row0 + rows) of an EXISTING q32b matrix of dst_rows (a multiple of 32, at most
 * LIREC_FEATURE_ROWS_MAX) x cols at dst: how a resident block store is filled in chunks and updated in place.  The same hi / lo
 * halves lirec_to_q32b writes for those values, at any row offset (a row's 128-byte lines are independent: no read-modify-write,
 * no other row is touched -- the caller zeroes a store's tail rows once).  src_f64 = 0: fp32 source; 1: float64, every value
 * converted through fp32 exactly as lirec_cast_f64_f32 + lirec_to_q32b would.  ld_src in elements.  LIREC_EINVAL for NULL or
 * misaligned pointers (dst 256 bytes, src its element size), cols % 32 != 0, ld_src < cols, a row range outside the matrix. */
int lirec_q32b_write_rows(const void* src, int32_t src_f64, int64_t ld_src, int64_t rows, int64_t cols, void* dst, int64_t dst_row0,
                          int64_t dst_rows, lirec_stream_t stream);
/* The same to q16b (ABI 119): every value rounded to bf16 (nearest even), 32 x 32 blocks of 2 KiB, row r of a block = 64 B;
 * lirec_q16b_bytes(rows, cols) bytes at dst (256-byte aligned).  What lirec_embed_fwd_args::x_q32 = 2 reads. */
int64_t lirec_q16b_bytes(int64_t rows, int64_t cols);
int lirec_to_q16b(const float* src, int64_t ld_src, int64_t rows, int64_t cols, void* dst, lirec_stream_t stream);
/* The same to q16c (ABI 122): the bf16 values in 32 x 64 blocks of 4 KiB, row r of a block = 128 B (cols % 64 == 0; the same
 * lirec_q16b_bytes).  What x_q32 = 3 reads, and the form of W1q in the single-pass mode. */
int lirec_to_q16c(const float* src, int64_t ld_src, int64_t rows, int64_t cols, void* dst, lirec_stream_t stream);
int lirec_embed_l1_indexed(const lirec_embed_fwd_args* const* heads, int32_t nh, const lirec_pieces* pieces,
                           float* const* zclip, float* const* ztrk, lirec_stream_t stream);

/* Row compaction for the pooled form.  A context row whose mask is 0 cannot influence any output
 * (the masked mean multiplies it by 0 and its gradient is 0; mlp/model.py:309-324), so it need not
 * be computed at all.  From mask [n, R] this writes rowmap[j] = c*R + r of the j-th row with a
 * non-zero mask (ascending; size n*R), cstart[c] = first compact row of candidate c (size n+1) and
 * count[0] = number of valid rows.  The count stays on the device: the GEMMs read it there and size
 * their work at run time, so nothing synchronises with the host.  Dropout counters keep the
 * original row ids, so every value equals the uncompacted computation. */
int lirec_compact_rows(const float* mask, int32_t n, int32_t R, int32_t* rowmap, int32_t* cstart, int32_t* count,
                       lirec_stream_t stream);
/* The same reading the mask in the dtype the DataLoader delivers it (mask_dtype: 0 fp32, 1 int64 -- rels_mask, SURVEY
 * appendix B --, 2 float64; no cast kernel) and also writing wts[j] = (float)mask[rowmap[j]] (size n*R, optional): the
 * pooling passes then read each candidate's weights as one contiguous run. */
int lirec_compact_rows2(const void* mask, int32_t mask_dtype, int32_t n, int32_t R, int32_t* rowmap, int32_t* cstart,
                        int32_t* count, float* wts, lirec_stream_t stream);
/* cstart of lirec_compact_rows2 must have room for 2 n + 1 ints: the entries behind n + 1 are scratch while the call runs
 * (one wave per candidate, two launches; lirec_compact_rows keeps n + 1 and a single-workgroup kernel). */

/* Backward of lirec_embed_fwd (replaces autograd through the same lines):
 *   given dZ2 [rows, sum out_dim] (ld lddz2) -- already multiplied by the
 *   tanh/dropout derivative when epilogue was 1 -- accumulates
 *   dW2_s += dZ2_s^T H1_s, db2_s += colsum dZ2_s,
 *   dZ1 = (dZ2_s W2_s) * [H1 > 0] / (1-p)   (into workspace, rows*nseg*J floats)
 *   dW1_s += dZ1_s^T X_s,  db1_s += colsum dZ1_s.
 * dX is not formed here: a caller whose features require grad asks lirec_embed_dx for it once this call has run (ABI 123).
 * Pooled form (mask != NULL; rows = n*R, dZ2 is [n, sum out_dim]):
 *   dW2_s += dZ2_s^T Hbar_s, db2_s += sum_c f[c] dZ2_s[c,:], dHbar = dZ2_s W2_s  (n rows),
 *   dZ1[c,r,:] = dHbar[c,:] * mask[c,r]/div[c] * [H1[c,r,:] > 0] / (1-p), then dW1/db1 as above.
 * Workspace layout of the pooled form, with rows32 = rows rounded up to 32 and W = nseg*J: dZ1 [rows, W] fp32 at float 0 (compact
 * form: one row per valid context row, in rowmap order) -- or, on the `planes` path, its bf16 hi plane [rows32, W] at byte 0 and
 * the lo plane right behind it; dHbar [n, W] fp32 at float rows32 * W, behind either (parts 3 writes it, parts 4 / 5 read it). */
typedef struct {
  const float* X; int64_t ldx;
  const float* W2[LIREC_MAX_SEG];
  const float* H1;
  const float* dZ2; int64_t lddz2;
  float* dW1[LIREC_MAX_SEG]; float* db1[LIREC_MAX_SEG];
  float* dW2[LIREC_MAX_SEG]; float* db2[LIREC_MAX_SEG];
  void* workspace; int64_t workspace_bytes;
  const float* mask; const float* Hbar; const float* fscale;   /* pooled form (as saved by lirec_embed_fwd) */
  const int32_t* rowmap; const int32_t* cstart; const int32_t* count;   /* compact pooled form, as in forward */
  const float* wts;                                                      /* as in forward */
  int32_t in_off[LIREC_MAX_SEG], in_dim[LIREC_MAX_SEG], out_dim[LIREC_MAX_SEG];
  /* parts: 0 the whole backward; 1 only the second-layer weight gradient (dW2, db2); 2 everything else = 3 then 4;
   * 3 only the hidden-layer gradient (dZ1, or dHbar in the pooled form); 4 only what follows it (un-pooling, dW1 / db1).
   * 1 is independent of 2 given dZ2, and the 4 of one head is independent of the 4 of another: a caller may enqueue
   * them on two streams (each stream with its own library context: both may split K into their context's scratch).
   * lirec_embed_bwd only: 5 = the un-pooling pass of 4 alone (then lirec_embed_dw1_indexed). */
  int32_t rows, nseg, J, parts;
  int32_t R, clamp_zero;
  lirec_rowsel sel;
  lirec_dropout drop;
  int32_t x_bf16, reserved2_;             /* as in lirec_embed_fwd_args */
  void* planes; int64_t planes_bytes;     /* the buffer the forward call filled (or NULL), see lirec_embed_fwd_args */
  const void* hbits;                      /* pooled form: the sign bits the forward call left (see lirec_embed_fwd_args); H1 may then be NULL */
  const struct lirec_pieces_s* pieces;    /* as in the forward call when its rows were gathered from q32b piece tables (else NULL) */
  int32_t x_q32, reserved3_;              /* as in the forward call */
  /* Optional (ABI 119; parts 0, 2 or 4 on the q32b path, single GPU): fold the Adam update of the first-layer parameters into the
   * kernel that finishes their gradients -- see lirec_fused_adam.  Taken from the first head of the call; LIREC_EINVAL where the
   * weight gradient would not run on the gemm_p2 kernels or the problems of the call do not cover `n_params`. */
  const struct lirec_fused_adam_s* adam;
} lirec_embed_bwd_args;
/* An Adam update folded into the launch that FINISHES the gradients it consumes (lirec_embed_bwd_args::adam: W1, b1 of every
 * segment of every head of the call, in the launch that sums the stream-K partial tiles of dW1 -- 10 M of the 34 M parameters at
 * the bench shape):
 * the thread that owns four gradient elements applies Adam to the parameters and moments at the same offsets of their flat
 * buffers (lirec_adam_step's arithmetic and op order: bit-identical), still stores the gradient, and -- `wq` -- writes the new
 * weights' q32b form into a shadow buffer (what lirec_embed_fwd_args::W1q points into): the weights at element offset o of the
 * flat buffers go to byte 4 * (o - wq_first) of `wq`, which must come out 256-byte aligned for every W1 (single-pass mode, ABI 122:
 * the q16c form at the same byte, half as long).  Saves the
 * gradient's round trip (written by the reduce, read back by lirec_adam_step), one launch, and the next forward's W1 staging.
 * p, g, m, v: buffers with ONE layout; every dW1[i] / db1[i] of the call must point into [g, g + n).  `n_params` = the number of
 * parameter elements the caller expects the call to update (sum of J * in_dim + J over the segments): checked, so that a
 * parameter the call does not reach cannot silently miss its update.  step / step_dev as in lirec_adam_step. */
typedef struct lirec_fused_adam_s {
  float* p; const float* g; float* m; float* v;
  void* wq; int64_t wq_first;
  int64_t n, n_params;
  int32_t step; float lr, beta1, beta2, eps, weight_decay, grad_scale;
  const int64_t* step_dev;
} lirec_fused_adam;
int lirec_embed_bwd(const lirec_embed_bwd_args* a, lirec_stream_t stream);
/* Both heads in one call: dW2 of both heads in one grouped launch, likewise the hidden-layer gradients; the two
 * first-layer weight gradients stay separate launches (a's first). */
int lirec_embed_bwd2(const lirec_embed_bwd_args* a, const lirec_embed_bwd_args* b, lirec_stream_t stream);
/* Input-feature gradient (ABI 123): dX = d loss / d X of the (n, rp1, D) block the forward read, from the hidden-layer gradients
 * the backward left in the heads' workspaces.  For head h and segment i, row L of the head (physical row (L / group) * group_stride
 * + group_off + L % group; the compact rows of the context head through its row map):
 *   dX[row(L), in_off[i] .. + in_dim[i]) = dZ1_i[L, :] W1[h][i]        (K = J; one grouped launch over head x segment)
 * and every element that no problem writes -- rows of a head that is absent, context rows whose mask is 0 (not computed under
 * compaction), columns of unused segments -- is set to 0 (a second launch).  No accumulation: the block is overwritten.
 * heads: the argument structs of the lirec_embed_bwd2 (nh = 2, in its order) or lirec_embed_bwd (nh = 1) call that ran the
 * whole backward (parts 0, or 2 after 1) -- the same workspaces, planes and GEMM core; nothing may have written the workspaces
 * since.  W1[h][i]: the first-layer weights [J][in_dim] of that head's segment i as the forward read them (issue the call before
 * any update of the weights).  group_stride must be rp1, the heads' row ranges disjoint, segments in column order, J and in_dim multiples of 4.
 * GEMM core: modes 0 and 1 the exact f32-input MFMA; modes 2 and 3 bf16x3 (three passes on both operands; in mode 3 the context
 * head's dZ1 exists only as its bf16 hi plane, so those rows multiply dZ1 rounded to bf16).
 * out_bf16: the block is bf16 (round to nearest even), else fp32.  ldx (elements, multiple of 4) >= D; dX 16-byte aligned. */
typedef struct {
  const lirec_embed_bwd_args* heads[2];
  int32_t nh, out_bf16;
  const float* W1[2][LIREC_MAX_SEG];
  void* dX; int64_t ldx;
  int32_t n, rp1, D, reserved_;
} lirec_embed_dx_args;
int lirec_embed_dx(const lirec_embed_dx_args* a, lirec_stream_t stream);
/* First-layer weight gradients from the unique pieces (the backward of lirec_embed_l1_indexed):
 *   dW1_seg += sum over pieces u of ( sum of the dZ1 rows whose index names u ) (x) piece_u ,  db1_seg += sum of the dZ1 rows.
 * The inner sums are  S = P^T dZ1  with P the 0/1 incidence matrix of the index (written by the call), an ordinary weight-
 * gradient GEMM: no sort, no atomics, fixed summation order.  heads[h]: the arguments of lirec_embed_bwd after its parts 3
 * (and 5, the un-pooling pass alone, for the pooled form) have run -- dZ1 sits in the workspace; X is not used.
 * The piece tables must carry ONE EXTRA ZERO ROW behind their n_clip / n_track rows (the piece of a negative index).
 * Scratch: P[h] rows_h x round4((n_clip + 1) + 2 (n_track + 1)) floats, S[h] ((n_clip + 1) + (n_track + 1)) x 2J floats. */
int lirec_embed_dw1_indexed(const lirec_embed_bwd_args* const* heads, int32_t nh, const lirec_pieces* pieces,
                            float* const* P, float* const* S, lirec_stream_t stream);
/* Gradient of the piece tables (ABI 124): d loss / d clip and d loss / d track of the de-duplicated tables the batch was given
 * as, from the per-piece sums S that lirec_embed_dw1_indexed left (S_h[u] = sum of head h's dZ1 rows whose index names piece u;
 * layer 1 is linear in the pieces).  With v' = n_clip + 1 + v, the row of track piece v in S:
 *   dClip[u, 0 .. text_dim)                 = sum_h S_h[u, 0 .. J)   W1[h][0]                      (K = nh J)
 *   dClip[u, text_dim .. + visual_dim)      = sum_h S_h[u, J .. 2J)  W1[h][1]
 *   dTrack[v, 0 .. track_dim)               = sum_h S_h[v', 0 .. J) W1[h][2] + S_h[v', J .. 2J) W1[h][3]   (K = 2 nh J)
 * (a track piece may be track-1 of some rows and track-2 of others).  The trailing zero rows dClip[n_clip] and dTrack[n_track]
 * are set to 0; pieces no row reads -- or only masked context rows -- come out 0 as well.  ONE launch, one writer per element
 * (the k-loop runs over the (S, W1) chunks in order): deterministic, no accumulation -- both outputs are overwritten.
 * Run it after lirec_embed_dw1_indexed on the same stream with the same heads, pieces and S; nothing may write S in between.
 * W1[h][i]: the first-layer weights [J][in_dim] of head h's segment i (text, visual, tracks1, tracks2) as the forward read them.
 * GEMM core: modes 0 and 1 the exact f32-input MFMA; modes 2 and 3 bf16x3 (S is fp32 in every mode).  Outputs fp32, 16-byte
 * aligned, ld_clip >= text_dim + visual_dim and ld_track >= track_dim (multiples of 4).  LIREC_EINVAL, before any device call,
 * for NULL pointers, nh not 1 or 2, nseg != 4, J or the dims not multiples of 4 (or J differing between the heads), segment
 * dims that disagree with `pieces`, misaligned outputs or strides. */
typedef struct {
  const lirec_embed_bwd_args* heads[2];
  int32_t nh, reserved_;
  const float* S[2];
  const float* W1[2][LIREC_MAX_SEG];
  const lirec_pieces* pieces;
  float* dClip; int64_t ld_clip;
  float* dTrack; int64_t ld_track;
} lirec_embed_dx_indexed_args;
int lirec_embed_dx_indexed(const lirec_embed_dx_indexed_args* a, lirec_stream_t stream);
/* scratch lirec_embed_bwd needs: `rows` = the logical row count, plus n for the pooled form
 * (pass rows = n*R + n).  (Twice the fp32 gradient of the hidden layer, rows rounded up to 32: the plain form keeps
 * the fp32 gradient and its bf16 planes side by side when layer 1 runs on planes.) */
int64_t lirec_workspace_bytes(int32_t rows, int32_t nseg, int32_t J);
/* bytes of the `planes` workspace of one head: feature planes for `rows` rows (rounded up to 32) of `dsum` = sum of
 * in_dim columns (hi + lo; hi only when x_bf16) + weight planes for J x dsum (hi + lo); 256-byte aligned parts */
int64_t lirec_planes_bytes(int32_t rows, int32_t dsum, int32_t J, int32_t x_mode);
/* (x_mode: 0 = fp32 rows, staged into the workspace; 2 = rows gathered from q32b storage -- x_q32 or q32b piece tables --, for
 *  which the workspace holds no row copy; 1 = a row-major bf16 block (x_bf16): its rows are staged as ONE plane, q16b) */

/* ---- masked mean over context clips ("pairwise" pooling pass) ------------
 * Replaces (z.view(n, R, W) * mask).sum(1) / divider followed by tanh and
 * dropout (mlp/model.py:301-327; :174-199 without the divider clamp):
 *   P[c,:] = sum_r mask[c,r] Z2[c,r,:] / div[c],  div = sum_r mask (clamp_zero: 0 -> 1)
 *   Tn = tanh(P);  E = dropout(Tn)   (site = drop.site2, row = c)
 * Z2 is [n*R, W] with row stride ldz; mask is fp32 [n, R]. */
int lirec_pool_fwd(const float* Z2, int64_t ldz, const float* mask, int32_t n, int32_t R, int32_t W,
                   int32_t clamp_zero, float* Tn, int64_t ldtn, float* E, int64_t lde,
                   const lirec_dropout* drop, lirec_stream_t stream);
/* dZ2[c,r,:] = dP[c,:] * mask[c,r] / div[c]   (dP already carries the tanh/dropout derivative) */
int lirec_pool_bwd(const float* dP, int64_t lddp, const float* mask, int32_t n, int32_t R, int32_t W,
                   int32_t clamp_zero, float* dZ2, int64_t lddz, lirec_stream_t stream);

/* ---- gating unit ----------------------------------------------------------
 * Replaces GatingUnit.forward (mlp/model.py:349-354):
 *   G = dropout(relu(EE Wg^T + bg)),  EE = [E_ctx | E_ints]  [n, K]  (ctx first, :352) */
int lirec_gate_fwd(const float* EE, int64_t ldee, const float* Wg, const float* bg, int32_t n, int32_t K,
                   int32_t N, float* G, int64_t ldg, const lirec_dropout* drop, lirec_stream_t stream);
/* Backward: dZg = dG * [G > 0] / (1-p) must already be in dZg (lirec_heads_bwd writes it);
 *   dWg += dZg^T EE, dbg += colsum dZg, and
 *   dEE[:, j] (op)= (dZg Wg)[:, j] * tanh'/dropout factor of column j, where
 *   columns [0, split) use (Tn_ctx, site_ctx) and [split, K) use (Tn_ints, site_ints);
 *   acc_first != 0 adds the existing contents of dEE[:, :split) (the relationship-head
 *   gradient) before applying the factor. */
int lirec_gate_bwd(const float* dZg, int64_t lddzg, const float* EE, int64_t ldee, const float* Wg,
                   int32_t n, int32_t K, int32_t N, int32_t split,
                   const float* Tn, int64_t ldtn, float* dWg, float* dbg, float* dEE, int64_t lddee,
                   int32_t acc_first, const lirec_dropout* drop, int32_t site_ctx, int32_t site_ints,
                   lirec_stream_t stream);
/* The same with `parts`: 0 both; 1 only dWg / dbg; 2 only dEE (independent given dZg: two streams, two contexts). */
int lirec_gate_bwd_parts(const float* dZg, int64_t lddzg, const float* EE, int64_t ldee, const float* Wg,
                         int32_t n, int32_t K, int32_t N, int32_t split,
                         const float* Tn, int64_t ldtn, float* dWg, float* dbg, float* dEE, int64_t lddee,
                         int32_t acc_first, const lirec_dropout* drop, int32_t site_ctx, int32_t site_ints,
                         int32_t parts, lirec_stream_t stream);

/* The gate's three GEMMs on STAGED q32b operands (ABI 118; ABI 120: one kernel form for all three).  `ws` =
 * lirec_gate_ws_bytes(n, K, N) bytes, 256-byte aligned, kept by the caller from the forward call to the backward call: the forward
 * stages Wg and EE there (blocked bf16 hi / lo, the fp32 footprint) AND their transposes (one read, two forms), the backward stages dZg
 * and its transpose -- so that forward (EE . Wg^T), data gradient (dZg . Wg, through the rows of Wg^T) and weight gradient (dZg^T . EE,
 * through the rows of dZg^T and EE^T) all read k-contiguous rows (the weights must not change between the two calls).  Kernel:
 * gemm_p3.hpp (wave-specialised workgroups, 128 x 96 or 128 x 128 tiles, persistent over tiles) when n % 128 == 0, N % 128 == 0,
 * N % 96 == 0, K % 96 == 0, split % 96 == 0 and K / 96 >= 8; else gemm_p2.hpp's forward / data-gradient kernels (n % 32 == 0, K and N
 * % 256, split % 256) with the plain weight-gradient kernel; else -- or with ws NULL -- the calls ARE the plain ones.  Same arithmetic
 * as lirec_gate_fwd / lirec_gate_bwd_parts (three bf16 products per element pair, fp32 accumulate, same dropout counters), another
 * summation order.  2 * split == K and contiguous EE / dZg are required throughout.  parts as in lirec_gate_bwd_parts. */
int64_t lirec_gate_ws_bytes(int32_t n, int32_t K, int32_t N);
int lirec_gate_fwd_ws(const float* EE, int64_t ldee, const float* Wg, const float* bg, int32_t n, int32_t K,
                      int32_t N, float* G, int64_t ldg, const lirec_dropout* drop, void* ws, int64_t ws_bytes,
                      int32_t weights_staged, lirec_stream_t stream);
/* Stages Wg (and Wg^T) into `ws` on its own (37.7 MB read, 75 MB written for the 3072 x 3072 gate: 25-45 us of HBM traffic that depends
 * on nothing else in the step).  A caller puts it on another stream beside the MFMA-bound layer-1 launch and then passes weights_staged = 1 to
 * lirec_gate_fwd_ws, which in that case stages the rows only and fails with LIREC_EINVAL where it would have fallen back.
 * LIREC_EINVAL when the shapes do not qualify (same rule as lirec_gate_fwd_ws: ask before relying on it). */
int lirec_gate_stage_weights(const float* Wg, int32_t n, int32_t K, int32_t N, void* ws, int64_t ws_bytes, lirec_stream_t stream);
int lirec_gate_bwd_ws(const float* dZg, int64_t lddzg, const float* EE, int64_t ldee, const float* Wg,
                      int32_t n, int32_t K, int32_t N, int32_t split,
                      const float* Tn, int64_t ldtn, float* dWg, float* dbg, float* dEE, int64_t lddee,
                      int32_t acc_first, const lirec_dropout* drop, int32_t site_ctx, int32_t site_ints,
                      int32_t parts, void* ws, int64_t ws_bytes, int32_t rows_staged, lirec_stream_t stream);
/* (parts 4 = stage the rows of dZg into `ws` and nothing else; a later call with rows_staged = 1 -- on any stream ordered behind
 *  it -- then skips that pass: this is how the weight gradient (part 1) runs on another stream beside the data gradient (part 2),
 *  both reading ONE staged copy.  Where the shapes do not qualify part 4 does nothing and the other parts are the plain kernels.) */

/* ---- output heads ----------------------------------------------------------
 * Replaces out_ints / out_ctx (mlp/model.py:332-336, :205-209, :90): Y = A W^T + b. */
int lirec_linear_fwd(const float* A, int64_t lda, const float* W, const float* b, int32_t n, int32_t K,
                     int32_t N, float* Y, int64_t ldy, lirec_stream_t stream);
/* Backward of one head: dW += dY^T A, db += colsum dY, and (if dA != NULL)
 *   dA (op)= dY W  with epilogue `mode`:
 *     0 store            1 relu-dropout backward: * [act > 0] / (1-p)   (act = G)
 *     2 tanh-dropout backward: * keep/(1-p) * (1 - act^2)               (act = Tn; site from drop->site2)
 *   accumulate != 0 adds the previous contents of dA before the factor is applied. */
int lirec_linear_bwd(const float* dY, int64_t lddy, const float* A, int64_t lda, const float* W,
                     int32_t n, int32_t K, int32_t N, float* dW, float* db,
                     float* dA, int64_t ldda, int32_t mode, const float* act, int64_t ldact,
                     int32_t accumulate, const lirec_dropout* drop, lirec_stream_t stream);

/* The same for several heads at once (out_ints and out_ctx are independent given their inputs): one grouped
 * launch per GEMM kind instead of one per head.  Field meaning as in lirec_linear_fwd / lirec_linear_bwd. */
typedef struct {
  const float* A; int64_t lda; const float* W; const float* b; float* Y; int64_t ldy;
  int32_t n, K, N, reserved_;
} lirec_linear_fwd_args;
int lirec_linear_fwd_group(const lirec_linear_fwd_args* v, int32_t count, lirec_stream_t stream);
typedef struct {
  const float* dY; int64_t lddy; const float* A; int64_t lda; const float* W;
  float* dW; float* db; float* dA; int64_t ldda; const float* act; int64_t ldact;
  int32_t n, K, N, mode, accumulate;
  int32_t parts;                          /* 0 both; 1 only dW / db; 2 only dA (independent of each other: two streams) */
  lirec_dropout drop;
} lirec_linear_bwd_args;
int lirec_linear_bwd_group(const lirec_linear_bwd_args* v, int32_t count, lirec_stream_t stream);

/* ---- losses ---------------------------------------------------------------
 * One fused forward+backward per loss: writes the scalar loss and d(loss)/d(logits).
 *
 * lirec_margin_loss covers the four max-margin losses of mlp/model.py:
 *   MaxMarginCrossEntropyLoss :427-441   (T=1, rels=NULL, lymbda=1, margin=opt.margin)
 *   MultiTaskMaxMargin        :387-419   (T=1, rels_mean_valid=1, margin=opt.margin)
 *   MarginLoss                :450-494   (rels=NULL, lymbda=1, margin=opt.tr_margin)
 *   MarginTrackRelsLoss       :503-575   (margin=opt.tr_margin)
 * Per clip b: padded tracks (mem==0) get logit -inf (written back into `ints` when
 * mask_inplace, as the reference's in-place masking does, :460,:512); S=sigmoid;
 * positive track k:
 *   sel[b] when sel != NULL and sel[b] >= 0 (a draw injected by the caller), else
 *   0 when tr_correct (:476,:550), else
 *   sample != 0 (opt.tr_cat_distr, :468-471,:538-543): drawn in the kernel from the categorical distribution
 *       p_t = softmax_t(ints[t,y])                                   (MarginLoss; logits with -inf on padded tracks)
 *       p_t = (softmax_t(ints[t,y]) + nan->0(softmax_t(rels'[t,r0]))) / 2      (MarginTrackRelsLoss; rels' = rels with
 *             the None column appended and -inf wherever the track is padded or its label is None, :516-524, :542)
 *     one wave per clip: lane t holds track t, max / sum by wave shuffles, u = (word 0 of
 *     philox(counter = (b, 0, LIREC_SITE_TRACK_SAMPLE, 0), key = sample_seed [+ *sample_seed_dev]) >> 8) * 2^-24,
 *     k = the first t with cumsum(p)_t > u * sum(p) (torch.multinomial normalises the same way; its own draw comes
 *     from torch's global generator, which nothing else can reproduce: the caller may inject one through `sel`);
 *     probs_out[b,t] (optional) receives p_t, the tensor the reference hands to torch.multinomial;
 *   otherwise argmax_t (S[t,y] + Q[t,r0]) * mem[t]  (:479,:552-553);
 * negatives = every (t,c) not masked by mem, multilab
 * weights or the target-column rules (:462-467,:526-537);
 *   sum variant: sum relu(m - pos + S) over negatives          (:488-492,:563-573)
 *   max variant: sum_t relu(m - pos + max_c S*mask)            (:483-486,:557-562)
 * loss = lymbda * mean_b(ints part) + mean(rels part), the latter over B clips or,
 * with rels_mean_valid, over the clips whose label != NR (:407-418).
 * Size limit: one workgroup per clip keeps the clip's sigmoid tables in LDS, 4 * (T*C + T*(NR+1) + 2*T + C + 20) bytes (the NR term
 * only with rels), which must not exceed 160 KiB -- LIREC_EINVAL before any device call otherwise (C = 101, NR = 15: T <= 343).
 * Any T within it is supported: the track softmax / sampler / argmax walk the tracks in steps of 64 lanes.
 */
typedef struct {
  float* ints; int64_t ld_ints;           /* [B*T, C] logits (modified in place when mask_inplace) */
  const float* rels; int64_t ld_rels;     /* [B*T, NR] or NULL */
  const float* mem;                       /* [B, T] fp32 0/1, or NULL = all ones */
  const float* w;                         /* [B, C] multilab weights fp32 0/1, or NULL = all ones */
  const int32_t* y;                       /* [B] interaction labels */
  const int32_t* r;                       /* [B, T] relationship labels (NR = None), or NULL */
  const int32_t* g;                       /* [B, 2] gt_tracks, or NULL = (0,0) */
  const int32_t* sel;                     /* [B] forced positive track, <0 = argmax; or NULL = argmax */
  float* d_ints; int64_t ld_dints;        /* [B*T, C] out */
  float* d_rels; int64_t ld_drels;        /* [B*T, NR] out (when rels) */
  float* loss;                            /* [1] out */
  float* partial;                         /* [2*B + 2] scratch */
  int32_t* sel_out;                       /* [B] chosen track (out, optional) */
  int32_t B, T, C, NR;
  float margin, lymbda;
  int32_t max_neg, tr_correct, mask_inplace, rels_mean_valid;
  /* 1: mem and w point to float64, y / r / g to int64 -- the dtypes the reference's DataLoader delivers
   *  -- and are read in place: no cast kernels between the loader batch and the loss. */
  int32_t loader_types;
  /* 0 argmax / forced; 1 draw the positive track in the kernel (tr_cat_distr); 2 as 1, but only probs_out and sel_out
   * are written (no loss, no gradients): for a caller that wants to draw from the probabilities itself */
  int32_t sample;
  uint64_t sample_seed;                   /* Philox key of the draw */
  const uint64_t* sample_seed_dev;        /* optional device counter added to the key (graph replay), as lirec_dropout */
  float* probs_out;                       /* [B, T] out, optional */
  /* Optional arrival counter (device int32, ZERO on entry, left zero on exit): when given, the clip whose workgroup
   * arrives last sums the per-clip partials in a fixed order and writes `loss` -- one launch instead of two. */
  int32_t* arrive;
  /* Data-parallel form of the batch means (the reference is single-device, mlp/train.py:42).  A rank that holds B
   * of the B_global clips of a global batch, and whose gradients are then AVERAGED over `world` ranks, passes the denominators
   * of the GLOBAL means divided by world:
   *   batch_divisor = B_global / world                                        (0: B, the local clip count)
   *   rels_divisor  = (clips of the global batch whose label != NR) / world   (0: the local count; rels_mean_valid only, :407-418)
   * The average over the ranks of the per-rank losses / gradients then IS the single-process loss / gradient of the global
   * batch, whatever the ranks' own counts.  divisors_dev: optional device float[2] = {batch_divisor, rels_divisor} read by the
   * kernel instead of the two values (the result of an all-reduce that never visits the host); entries <= 0: the defaults. */
  float batch_divisor, rels_divisor;
  const float* divisors_dev;
  /* stride of `y` in elements (0 = 1): the clip's label read IN PLACE out of the loader's [B, R+1, 1] labels tensor of the
   * multi-clip recipe (mlp/model.py:393: labels[:, 0]) -- no gathered copy, so a recorded step sees a refilled batch's labels */
  int32_t y_stride, reserved_;
} lirec_margin_loss_args;
int lirec_margin_loss(const lirec_margin_loss_args* a, lirec_stream_t stream);

/* Per-clip weights and per-clip loss values of the fused losses (added to ABI 124 without a new number: three new exports and a
 * new struct, index 19 of lirec_abi_sizeof; 18 stays unassigned).  With li_b / lr_b the interaction and relationship terms of
 * clip b as the kernels compute them before the batch means' coefficients, and weights w_b >= 0, finite:
 *     loss = lymbda * sum_b w_b li_b / D_i  +  sum_b w_b lr_b / D_r
 * and the gradients are exactly its derivative (the coefficients become per-clip, the positive element's term included).
 *   norm 0 ('sum'):   a weighted mean, the convention of F.cross_entropy(weight=): D_i = sum_b w_b; D_r = the sum of w_b over the
 *                     clips whose label != NR for the two multitask clip losses (rels_mean_valid; the CE loss's relationship
 *                     half), sum_b w_b otherwise.  In lirec_ce_loss the clip weight multiplies the class weight:
 *                     scale_b = w_b cw[y_b] / sum_b w_b cw[y_b].
 *   norm 1 ('count'): the denominators stay the counts (B, the labelled clips); the weights are plain multipliers.
 * A denominator of 0 (every weight 0; no labelled clip) gives loss 0 and all-zero gradients for that half, never NaN.  Weights
 * all 1.0 give, under either norm, the bits of the unweighted call.  Every workgroup forms the sums itself in one fixed order:
 * no extra launch, deterministic.  The weights are read as given: a negative or non-finite weight is the caller's to refuse.
 * The data-parallel denominators (batch_divisor / rels_divisor / divisors_dev; den_ints / den_rels / dens_dev) keep their
 * meaning, "the global denominators over world": with norm 0 those are the global weight sums.
 * A NULL struct, or one whose `w` is NULL, issues the launches and gives the bits of the unweighted call; with only `clip_loss`
 * set it is the unweighted loss that also reports the per-clip values.  LIREC_EINVAL before any device call: `w` and `clip_loss`
 * both NULL; norm outside {0, 1}; `w` not aligned to its type (8 / 4 bytes); `clip_loss` not aligned to 4 bytes; sample == 2
 * (probabilities only) with a struct.  The LDS need is that of the unweighted call. */
typedef struct {
  const void* w;        /* [B] clip weights, or NULL = all ones */
  int32_t w_f64;        /* 1: w is float64 (the loader's dtype), 0: float32 */
  int32_t norm;         /* 0 'sum', 1 'count' */
  float* clip_loss;     /* [B, 2] out, optional: (lymbda * li_b, lr_b) UNWEIGHTED and UNDIVIDED, so that
                           sum_b w_b (clip_loss[b,0] / D_i + clip_loss[b,1] / D_r) = loss; column 1 is 0 where the clip has no
                           relationship term.  lirec_ce_loss: (cw[y_b] * CE_b of the interaction row, CE_b of the relationship row) */
} lirec_clip_weights;
/* lirec_margin_loss with clip weights; lirec_margin_loss(a, s) is lirec_margin_loss_weighted(a, NULL, s) */
int lirec_margin_loss_weighted(const lirec_margin_loss_args* a, const lirec_clip_weights* cw, lirec_stream_t stream);

/* SURVEY 8(b)'s K5 boundary call: the output heads, the loss and the heads' data gradient as ONE library call --
 *   out_ints / out_ctx (mlp/model.py:332-336, :205-209)   heads[0..n_heads): Y = A W^T + b          (one grouped launch)
 *   the max-margin loss on those logits (:381-575)         loss: fused forward + d(loss)/d(logits)   (one launch)
 *   dA = dlogits W of every head                           back[0..n_heads), issued with parts = 2   (one grouped launch)
 * i.e. what a host that drives forward, loss and backward together (an inference-free training loop, the recorded step) issues
 * between the gate product and the gate's data gradient.  `loss->ints` / `loss->rels` must be the heads' Y, `back[h].dY` the
 * loss's d_ints / d_rels.  The heads' WEIGHT gradients are not part of it (independent of the chain: lirec_linear_bwd_group
 * with parts = 1, on a second stream).  Three launches, not one: a single-launch form -- one workgroup per clip pulling the
 * 1.2 MB of out_ints.weight through its CU twice -- is slower than these on this machine.  NULL `loss` (evaluation):
 * the heads only. */
int lirec_heads_loss_fwd_bwd(const lirec_linear_fwd_args* heads, const lirec_linear_bwd_args* back, int32_t n_heads,
                             const lirec_margin_loss_args* loss, lirec_stream_t stream);
/* The same boundary call with clip weights on its loss (lirec_clip_weights; NULL: the call above).  NULL `loss` with a struct:
 * LIREC_EINVAL. */
int lirec_heads_loss_fwd_bwd_weighted(const lirec_linear_fwd_args* heads, const lirec_linear_bwd_args* back, int32_t n_heads,
                                      const lirec_margin_loss_args* loss, const lirec_clip_weights* cw, lirec_stream_t stream);

/* MultiTaskCrossEntropyLoss.forward (mlp/model.py:367-378): mean CE over `ints` rows plus
 * mean CE over the `rels` rows whose label != NR.  class_w ([C]) may be NULL.
 * den_ints / den_rels / dens_dev: the data-parallel form, as lirec_margin_loss_args::batch_divisor -- the denominators of the
 * two means given by the caller (the global batch's sum of target class weights / its count of labelled rows, each divided by
 * world); 0 / NULL: this batch's own (the reference's single-device form).  dens_dev: device float[2] read instead. */
int lirec_ce_loss(const float* ints, int64_t ld_ints, const float* rels, int64_t ld_rels,
                  const int32_t* y, const int32_t* r, const float* class_w,
                  int32_t B, int32_t C, int32_t NR, float* d_ints, int64_t ld_dints,
                  float* d_rels, int64_t ld_drels, float* loss, float* partial,
                  float den_ints, float den_rels, const float* dens_dev, lirec_stream_t stream);
/* The same with clip weights (lirec_clip_weights; NULL: the call above).  Norm 0: the interaction denominator is
 * sum_b w_b cw[y_b], the relationship denominator the sum of w_b over the labelled rows; den_ints / den_rels / dens_dev, when
 * given, are those sums of the global batch over world. */
int lirec_ce_loss_weighted(const float* ints, int64_t ld_ints, const float* rels, int64_t ld_rels,
                           const int32_t* y, const int32_t* r, const float* class_w,
                           int32_t B, int32_t C, int32_t NR, float* d_ints, int64_t ld_dints,
                           float* d_rels, int64_t ld_drels, float* loss, float* partial,
                           float den_ints, float den_rels, const float* dens_dev, const lirec_clip_weights* cw,
                           lirec_stream_t stream);

/* ---- optimiser --------------------------------------------------------------
 * torch.optim.Adam(lr, weight_decay) as configured at mlp/model.py:599-601, fused over
 * one flat fp32 buffer: g += wd*p; m = lerp(m, g, 1-b1); v = b2*v + (1-b2) g^2;
 * p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).  grad_scale multiplies g first
 * (1/world_size after a summing all-reduce). `step` is 1-based.
 * p, g, m, v must be 16-byte aligned (the kernel moves them four floats at a time; `n` may be any count): LIREC_EINVAL
 * otherwise, from lirec_adam_step and lirec_adam_step_counted alike, before any device call. */
int lirec_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int32_t step,
                    float lr, float beta1, float beta2, float eps, float weight_decay,
                    float grad_scale, const int64_t* step_dev, lirec_stream_t stream);
/* The same update with the step taken from a device counter of COMPLETED steps that the launch itself maintains: step =
 * *count_dev + 1, and -- advance != 0 -- the workgroup that finishes last stores it back (`ticket`: a device int32, zero on entry,
 * left zero).  For a stream that counts its own steps: a replayed train step leaves its weight-gradient side stream running into
 * the next step, whose first launch advances the shared step counter (lirec_amd/graph.py) -- the side stream's share of the update
 * reads its own.  An update cut into several calls passes advance on the last one only. */
int lirec_adam_step_counted(float* p, const float* g, float* m, float* v, int64_t n,
                            float lr, float beta1, float beta2, float eps, float weight_decay,
                            float grad_scale, int64_t* count_dev, int32_t* ticket, int32_t advance, lirec_stream_t stream);
/* The same update over a scattered set of ranges of the flat buffers, one launch: what a partly frozen model needs (parameters
 * with requires_grad = False keep their values AND their moments; lirec_amd/optim.py).  `ranges` (HOST memory, copied into the
 * launch by value): `count` <= LIREC_ADAM_MAX_RANGES entries, ascending and disjoint; element offsets from p / g / m / v that
 * are multiples of 4 (every parameter of the flat layout starts on one), any length >= 0.  Range r is updated with step
 * t - lag[r] -- the number of updates ITS parameters have received, torch.optim.Adam's per-parameter `step` -- where t is
 *   `step` by value (step_dev and count_dev NULL; step - lag >= 1 for every range),
 *   *step_dev, or
 *   *count_dev + 1, with ticket / advance exactly as in lirec_adam_step_counted
 * (a device step below 1 after the lag counts as 1).  Element for element the arithmetic -- and the bits -- of lirec_adam_step
 * on that range with that step; nothing outside the ranges is read or written.  count == 0, or all lengths 0: no launch (and no
 * advance).  LIREC_EINVAL before any device call for: count outside 0..64, a negative length, offset or lag, an offset that is not
 * a multiple of 4, p / g / m / v not 16-byte aligned, ranges overlapping or out of order, a by-value step with step - lag < 1,
 * step_dev together with count_dev, count_dev without ticket. */
#define LIREC_ADAM_MAX_RANGES 64
typedef struct {
  int64_t offset, length;                /* elements */
  int32_t lag, reserved_;
} lirec_adam_range;
int lirec_adam_step_ranges(float* p, const float* g, float* m, float* v, const lirec_adam_range* ranges, int32_t count,
                           int32_t step, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                           const int64_t* step_dev, int64_t* count_dev, int32_t* ticket, int32_t advance, lirec_stream_t stream);
/* ---- gradient clipping by global norm, on the device ------------------------------
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm type 2) for callers that cannot visit the host between backward and
 * update (a recorded step, a sharded data-parallel update): a reduction leaves the clip coefficient in device memory, and the Adam
 * launches multiply it into the scale they already apply to every gradient -- no pass that scales the gradients, which therefore
 * stay UNCLIPPED in their buffer (clip_grad_norm_ scales them in place; the update is the same to one fp32 rounding of the scalar:
 * g * (grad_scale * coef) here, (g * coef) * grad_scale there).  (Added to ABI 124 without a new number: exports only.)
 *
 * lirec_grad_sq_partials: partials[w], w < LIREC_CLIP_PARTIALS (device doubles, all of them written), = the sums of squares that
 * workgroup w of a FIXED grid finds in the ranges of g (`ranges`: host memory, offset / length as in lirec_adam_step_ranges, `lag`
 * ignored; ranges may come in any order and are not checked against each other).  Accumulated in double in a fixed order: the
 * partials -- and their sum -- are a pure function of the values, the ranges and LIREC_CLIP_PARTIALS, bit for bit the same on every
 * device, stream and launch form (eager, recorded).  LIREC_EINVAL before any device call for: a NULL pointer, n_ranges outside
 * 1..64, a negative length or offset, an offset that is not a multiple of 4, g not 16-byte or partials not 8-byte aligned.
 *
 * lirec_clip_finalize (one workgroup): S = the sum of the partials in a fixed tree;
 *   mode 0  *sq_dev = S          mode 1  *sq_dev += S (a second table of ranges, further buckets)
 *   mode 2  partials not read (may be NULL), *sq_dev as it stands (after an all-reduce of it)
 * then, in double, norm = sqrt(*sq_dev) * grad_scale, x = max_norm / (norm + 1e-6) (torch's formula), and
 *   out[0] = coef = x < 1 ? x : (x is NaN ? x : 1)      out[1] = norm                      (device floats)
 * A NaN norm gives a NaN coefficient -- and NaN parameters, as clip_grad_norm_ without error_if_nonfinite does --, an infinite
 * norm the coefficient 0.  LIREC_EINVAL for: sq_dev / out NULL, partials NULL with mode 0 or 1, a mode outside 0..2, max_norm NaN
 * or <= 0, partials / sq_dev not 8-byte or out not 4-byte aligned.
 *
 * lirec_set_adam_clip(coef_dev): while coef_dev is not NULL, every lirec_adam_step, lirec_adam_step_counted and
 * lirec_adam_step_ranges launch issued BY THE CALLING HOST THREAD uses grad_scale * *coef_dev (one fp32 product) where it used
 * grad_scale; the kernel reads the word once per launch -- a uniform load of what an earlier launch on the stream wrote.  The
 * pointer is taken when the launch is issued: a recorded launch keeps it by value, and every replay reads the coefficient anew.
 * The setting follows the HOST THREAD (like lirec_set_grad_overwrite and the recorder), not the context: launches the thread issues
 * on a side stream under a context of its own are clipped too.  NULL (the default): the launches are exactly the unclipped ones,
 * kernels and arguments.  A folded update (lirec_embed_bwd_args::adam) is REFUSED (LIREC_EINVAL) while a coefficient is set: the
 * norm needs the finished gradient that launch itself produces.  LIREC_EINVAL for a pointer that is not 4-byte aligned. */
#define LIREC_CLIP_PARTIALS 1024
int lirec_grad_sq_partials(const float* g, const lirec_adam_range* ranges, int32_t n_ranges, double* partials,
                           lirec_stream_t stream);
int lirec_clip_finalize(const double* partials, double* sq_dev, int32_t mode, float grad_scale, float max_norm, float* out,
                        lirec_stream_t stream);
int lirec_set_adam_clip(const float* coef_dev);
/* ---- skipping non-finite steps, on the device ---------------------------------------
 * The device-side "found inf -> no-op" of a fused optimiser (apex's noop_flag, torch's _fused_adam(found_inf=)) for callers that
 * cannot visit the host between backward and update: a step whose gradients hold a NaN or an Inf leaves p, m and v untouched and
 * does not count as an update for the bias corrections.  Built on the norm above: the double sum of squares of
 * lirec_grad_sq_partials is non-finite exactly when an element of its ranges is (squares cannot cancel, and the squares of finite
 * fp32 values cannot overflow a double).  (Added to ABI 124 without a new number: exports only.)
 *
 * lirec_clip_finalize_guard (one workgroup): lirec_clip_finalize -- modes, tree and arithmetic, bit for bit -- with
 *   max_norm == 0   allowed: no clipping, out[0] = 1
 *   out[2] = skip   1.0f when *sq_dev (the double itself, not norm * grad_scale) is NaN or infinite, 0 otherwise
 *   count != 0      *skipped_dev += skip (a device int64: the steps skipped so far)
 * `out`: three device floats (four reserved).  `count` goes on exactly ONE finalize of a step -- the last, behind the all-reduce
 * under data parallelism.  LIREC_EINVAL before any device call for: sq_dev / out NULL, partials NULL with mode 0 or 1, a mode
 * outside 0..2, max_norm NaN or negative, count != 0 with skipped_dev NULL, partials / sq_dev / skipped_dev not 8-byte or out not
 * 4-byte aligned.
 *
 * lirec_set_adam_guard(out_dev, skipped_dev): while set, every lirec_adam_step, lirec_adam_step_counted, lirec_adam_step_ranges and
 * lirec_adam_step_groups launch issued BY THE CALLING HOST THREAD is the guarded kernel: one uniform load of out_dev[2]; set, no
 * element of p, g, m, v is read or written (the count_dev / ticket / advance epilogue still runs: a counting stream stays in
 * step); otherwise the update uses the scale grad_scale * out_dev[0] and the step t - *skipped_dev (then - lag per range), clamped
 * at 1, with the bias corrections ALWAYS computed by the kernel, in double (a by-value step behaves as step_dev holding it): the
 * bits of the clipped launch with that coefficient and step_dev holding t - *skipped_dev.  Both pointers are taken when the launch
 * is issued: a recorded launch keeps them, every replay reads them anew.  Host-thread state like lirec_set_adam_clip, over which
 * it takes precedence.  NULL, NULL (the default): exactly what is launched without this call.  A folded update
 * (lirec_embed_bwd_args::adam) is REFUSED (LIREC_EINVAL) while a guard is set.  LIREC_EINVAL for: one pointer without the other,
 * out_dev not 4-byte or skipped_dev not 8-byte aligned. */
int lirec_clip_finalize_guard(const double* partials, double* sq_dev, int32_t mode, float grad_scale, float max_norm, float* out,
                              int64_t* skipped_dev, int32_t count, lirec_stream_t stream);
int lirec_set_adam_guard(const float* out_dev, const int64_t* skipped_dev);
/* ---- gradient accumulation: one update per k micro-batches, decided on the device ---------
 * For callers that re-issue the same launches every micro-step (a recorded step) and therefore cannot decide on the host whether a
 * micro-step only accumulates ("hold") or closes its window and updates ("apply").  (Added to ABI 124 without a new number: exports
 * only.)
 *
 * The WINDOW BLOCK: four int64 in device memory, 16-byte aligned -- [0] phase = the micro-batches already in the open window,
 * 0 .. k-1, set by the caller before the first call; [1] hold, written by lirec_accum_begin; [2] a ticket, zero on entry and
 * left zero; [3] reserved.
 *
 * lirec_accum_begin: the head launch of a micro-step, in the place of lirec_zero_count.  Zeroes the `bytes` at p (lirec_zero_count's
 * rules: 16-byte aligned, any byte count) ONLY when the micro-step opens a window (phase 0); adds every_host[i] to ctr[i], i < n <= 4,
 * on every call and apply_host[i] besides on the call that closes the window (phase + 1 >= k); leaves hold = 1 (a hold) or 0 (an
 * apply) for the launches behind it on the stream, and the phase advanced (0 after an apply).  Every workgroup decides from the
 * phase as it was on entry; the words are advanced by the workgroup that finishes last.  Nothing of an earlier step may still
 * read the hold word when this launch runs: a caller joins its side streams before the next micro-step.  LIREC_EINVAL before any
 * device call for: bytes < 0, p NULL with bytes > 0 or not 16-byte aligned, n outside 0..4, n > 0 with ctr, every_host or
 * apply_host NULL, ctr not 8-byte aligned, win NULL or not 16-byte aligned, k < 1.
 *
 * lirec_set_adam_hold(hold_dev, k): while set, every lirec_adam_step, lirec_adam_step_counted, lirec_adam_step_ranges and
 * lirec_adam_step_groups launch issued BY THE CALLING HOST THREAD does one uniform load of *hold_dev (word 1 of a window block) in
 * front of everything else; non-zero: no element of p, g, m, v is read or written and -- unlike a guarded skip -- the
 * count_dev / ticket / advance epilogue does NOT run (a hold is no update for a counting stream either).  Zero: the launch is the
 * one issued without this call with the scale (float)((double)grad_scale / k) in the place of grad_scale, bit for bit.
 * lirec_ema_step launches of the thread take the same gate.  With a guard or a clip coefficient also set the scale is multiplied
 * on as ever, and a launch is a no-op when either flag says so.  The pointer is taken when the launch is issued: a recorded launch
 * keeps it, every replay reads the word anew.  Host-thread state like lirec_set_adam_guard.  NULL, 0 (the default): exactly what
 * is launched without this call.  A folded update (lirec_embed_bwd_args::adam) is REFUSED (LIREC_EINVAL) while a hold is set.
 * LIREC_EINVAL for: hold_dev without k >= 1, k != 0 without hold_dev, hold_dev not 8-byte aligned. */
int lirec_accum_begin(void* p, int64_t bytes, int64_t* ctr, const int64_t* every_host, const int64_t* apply_host, int32_t n,
                      int64_t* win, int32_t k, lirec_stream_t stream);
int lirec_set_adam_hold(const int64_t* hold_dev, int32_t k);
/* ---- exponential moving average of the weights --------------------------------------
 * torch.optim.swa_utils.get_ema_multi_avg_fn(decay) / timm's ModelEmaV2 as a launch that rides behind an Adam launch on that
 * launch's stream: ema[i] <- fmaf(weight, p[i] - ema[i], ema[i]) for i < n, the difference rounded to fp32 first -- torch's
 * lerp(ema, p, weight) for weight < 0.5, bit for bit.  weight = (float)(1.0 - decay), rounded by the caller.  An element with
 * ema[i] == p[i] keeps its bits (but for ema[i] = -0, which becomes +0 as in torch: the difference of equal values is +0).  One memory-bound launch (12 bytes per element: f32x4 body, 256-thread workgroups, at most
 * LIREC_EMA_MAX_BLOCKS of them, grid-strided), with a scalar head until the pointers reach 16-byte alignment and a scalar tail:
 * ema and p may start at ANY element of their buffers (a data-parallel slice), as long as both sit at the same offset modulo 16
 * bytes.  guard_dev, when not NULL, is the `out` block of lirec_clip_finalize_guard: one uniform load of word 2; non-zero, no
 * element is read or written (a skipped step is no update of the average either).  The pointer is taken when the launch is
 * issued: a recorded launch keeps it, every replay reads the word anew.  n == 0: no launch.  LIREC_EINVAL before any device call
 * for: ema or p NULL, n < 0, a pointer (guard_dev included) not 4-byte aligned, ema and p differing modulo 16 bytes, weight not in
 * (0, 0.5) (NaN included).  (Added to ABI 124 without a new number: an export only.) */
#define LIREC_EMA_MAX_BLOCKS 2048
int lirec_ema_step(float* ema, const float* p, int64_t n, float weight, const float* guard_dev, lirec_stream_t stream);
/* ---- per-range gradient, weight and update statistics ---------------------------------
 * What a training dashboard asks of every layer -- gradient norm, weight norm, the size of the Adam step against the weight, and
 * WHERE a NaN sits -- as one deterministic pass over the flat buffers instead of six torch ops per parameter.  On demand: no other
 * call issues it.  (Added to ABI 124 without a new number: two new exports and a new struct, index 43 of lirec_abi_sizeof; 42
 * stays unassigned.)
 *
 * `entries` (HOST memory, copied into the launch by value): n_ranges in 1..LIREC_PARAM_STATS_MAX_RANGES ranges
 * [offset, offset + length) of p / g / m / v -- the four buffers are addressed with the SAME element offsets; ANY offset, any
 * length >= 0, in any order, overlapping or not.  `flags` says which groups of columns the entry asks for: bit 0 the gradient
 * (needs g), bit 1 the parameter (needs p), bit 2 the update (needs m and v); a buffer no entry needs may be NULL.  Row r of `out`
 * (device double[n_ranges][LIREC_PARAM_STATS_COLS]) is
 *   cols 0-2  over x = g[i]:   the sum of x^2 over the finite x, the largest |x| over the finite x, the count of non-finite x
 *   cols 3-5  over x = p[i]:   the same three
 *   cols 6-8  over x = u_i = ((double)m[i] * inv_bc1) / (sqrt((double)v[i]) * inv_sqrt_bc2 + eps), every operation in double and
 *             rounded on its own: the same three.  An element whose u_i is not finite -- a NaN or infinite m, a NaN or negative v,
 *             0 / 0 -- is counted and left out.  (v = +Inf with a finite m gives u_i = 0, a finite value.)  With inv_bc1 =
 *             1 / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t), lr * sqrt(col 6) is the norm of Adam's step t.
 * A group that is not asked for, and every column of an empty range, is 0.  A NaN is counted, never propagated into a sum or a
 * maximum; -0 and denormals are ordinary finite values; FLT_MAX squared is finite in double and is summed.
 * DETERMINISM: a row is a pure function of the values in its range and of its own entry -- the same bits on every launch, stream,
 * device and launch form (eager, recorded), wherever the buffers lie and whatever else the table holds.  The grid is a constant; a range is dealt in blocks of
 * 1024 elements counted from the multiple of 4 at or below its offset, four consecutive elements a thread; every thread
 * accumulates in double in element order (the square of an fp32 value is exact there); fixed shuffle / LDS trees, then a second
 * launch, one workgroup per range, that takes the workgroups' partials in the order of the range's own blocks.  No floating-point atomics.
 * ALIGNMENT: with every buffer in use on a 16-byte boundary a thread's four elements are one 16-byte load per buffer wherever
 * they lie inside the range -- the whole of a range whose offset is a multiple of 4 but its last length % 4 elements; up to three
 * head and three tail elements of another are loaded one by one.  If ANY buffer in use is off a 16-byte boundary (all of them by
 * the same amount or not) the call falls back to scalar loads of the same elements in the same order: the same bits, more load
 * instructions.  A pointer that is not 4-byte aligned is refused.
 * `workspace`: caller-owned device memory of at least lirec_param_stats_ws_bytes(n_ranges) bytes (-1 for n_ranges outside
 * 1..64), 8-byte aligned, not zeroed by anybody; free again when the call's launches have run.  Two launches (one when every
 * length is 0) on `stream`, recorded into a command list like any other; profile site "param_stats".
 * LIREC_EINVAL before any device call (also under the host-side dry run) for: entries NULL; n_ranges outside 1..64; a negative
 * offset or length, or an end that would wrap; flags outside 0..7; a flag whose buffers are NULL; eps NaN, infinite or negative;
 * inv_bc1 or inv_sqrt_bc2 NaN or infinite; out or workspace NULL or not 8-byte aligned; workspace_bytes below the query's answer;
 * p, g, m or v not 4-byte aligned.  TRUSTED: every range lies inside the buffers it asks for. */
#define LIREC_PARAM_STATS_MAX_RANGES 64
#define LIREC_PARAM_STATS_COLS 9
typedef struct {
  int64_t offset, length;                /* elements */
  int32_t flags;                         /* bit 0 gradient, bit 1 parameter, bit 2 update */
  float inv_bc1, inv_sqrt_bc2, eps;      /* of the update columns; ignored without bit 2 (but checked) */
} lirec_param_stat_entry;
int64_t lirec_param_stats_ws_bytes(int32_t n_ranges);
int lirec_param_stats(const float* p, const float* g, const float* m, const float* v, const lirec_param_stat_entry* entries,
                      int32_t n_ranges, double* out, void* workspace, int64_t workspace_bytes, lirec_stream_t stream);
/* ---- parameter groups: hyper-parameters in device memory ---------------------------
 * torch.optim.Adam's param_groups, and hyper-parameters that change between the replays of a recorded step (a learning-rate
 * schedule): lr, betas, eps and weight_decay live in a small TABLE in device memory, one 32-byte row per group, that the Adam
 * launches read instead of taking the five values as arguments.  A recorded launch then holds the table's address, and a changed
 * value is one tiny launch in front of the replay.  (Added to ABI 124 without a new number: exports only.)
 *
 * A table: n_groups <= LIREC_ADAM_MAX_GROUPS rows of lirec_adam_hyper in device memory, 16-byte aligned.
 *
 * lirec_adam_hyper_write: one tiny launch that stores `rows_host` (HOST memory, n_groups rows, copied into the launch by value;
 * `decoupled` as 1.0f / 0, the reserved words as zeros) into the table -- an ordinary kernel on `stream`: stream order is all that protects the
 * launches that read the table, so a table belongs to ONE stream and is written on the stream that reads it.  LIREC_EINVAL before
 * any device call for: a NULL or not 16-byte aligned table, rows_host NULL, n_groups outside 1..8.  The VALUES are not checked.
 *
 * lirec_adam_step_groups: lirec_adam_step_ranges with a group per range: lr, beta1, beta2, eps and weight_decay of range r are
 * those of row ranges[r].group of the table as the launch finds it.  Ranges, lags, step / step_dev / count_dev + ticket + advance
 * and the clip coefficient of lirec_set_adam_clip exactly as there.  The bias corrections are ALWAYS computed by the kernel, in
 * double, from the row's values: a by-value `step` t behaves as step_dev holding t, and the bits on a range are those of
 * lirec_adam_step with step_dev on that range with the row's values.  count == 0, or all lengths 0: no launch (and no advance).
 * LIREC_EINVAL before any device call for: everything lirec_adam_step_ranges refuses, a group outside 0..n_groups-1, n_groups
 * outside 1..8, a NULL or not 16-byte aligned table.
 *
 * lirec_set_adam_hyper_row(row_dev): while row_dev is not NULL, a folded update (lirec_embed_bwd_args::adam) issued BY THE CALLING
 * HOST THREAD reads its five values from that device row -- the by-value ones in lirec_fused_adam are ignored -- and computes its
 * bias corrections itself (the bits of lirec_adam_step with step_dev and the row's values).  The pointer is taken when the launch
 * is issued: a recorded launch keeps it, every replay reads the values anew.  NULL (the default): exactly the kernel and the
 * arguments as without this call.  LIREC_EINVAL for a pointer that is not 16-byte aligned.
 *
 * DECOUPLED WEIGHT DECAY (AdamW; added to ABI 124 without a new number: word 5 of a row was reserved and written as zero, which
 * reads as "coupled").  A row whose `decoupled` is not 0 is updated, on the ranges of lirec_adam_step_groups that name it and in a
 * folded update that reads it, by
 *     d  = (float)(1.0 - (double)lr * (double)weight_decay)          once per range / launch
 *     g' = g * gscale                                                (no decay term; gscale includes the clip coefficient)
 *     m' = m + (1 - beta1) * (g' - m);   v' = v * beta2 + ((1 - beta2) * g') * g'
 *     p' = p * d - step_size * (m' / (sqrtf(v') / bc2_sqrt + eps))
 * in fp32 in this order, no contraction: torch.optim.AdamW's single-tensor order.  d is exactly 1 when lr weight_decay < 2^-25
 * (3e-5 x 1e-5, the defaults, is such a case): the decay is then invisible in fp32, as in torch's fp32 mul_.  A launch may mix
 * coupled and decoupled rows; a row with 0 gives the bits it always gave.  lirec_adam_hyper_write stores the word as 1.0f for any
 * non-zero host value and as 0 otherwise, the two reserved words as zeros.  THE BY-VALUE LAUNCHES (lirec_adam_step,
 * lirec_adam_step_counted, lirec_adam_step_ranges, the by-value fields of lirec_fused_adam) KNOW THE COUPLED FORM ONLY: a caller
 * who wants AdamW uses lirec_adam_step_groups with a table of one row.
 *
 * lirec_set_adam_hyper_map(table_dev, ranges, count): ONE ROW PER PARAMETER in a folded update.  While count > 0, a folded update
 * issued by the calling host thread looks up, per workgroup, the entry of `ranges` that holds its problem's weight and the one
 * that holds its bias (offsets in elements from lirec_fused_adam::g, i.e. ranges of the flat layout; `group` = the row of
 * table_dev), and updates each with its own row -- a first layer whose weights and biases are in different groups keeps the
 * fold.  `ranges` is HOST memory, copied by the call; at most LIREC_ADAM_MAP_MAX entries (two heads x four segments x weight and
 * bias); every lag must be 0 (the fold updates with the one global step).  It takes precedence over lirec_set_adam_hyper_row;
 * count == 0 or table_dev NULL switches it off, and the library then launches what it launched before.  LIREC_EINVAL before any
 * device call for: a table that is not 16-byte aligned, count outside 0..16, count > 0 with ranges or table NULL, ranges that
 * overlap or do not ascend, a length < 1, offset + length beyond INT64_MAX, a lag != 0, a group outside 0..7; and from the
 * folded update itself when a weight or a bias of the call lies in no entry. */
#define LIREC_ADAM_MAX_GROUPS 8
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
  float decoupled;                       /* != 0: AdamW, the decay multiplies p by 1 - lr weight_decay; 0: coupled (L2) */
  float reserved_[2];
} lirec_adam_hyper;
typedef struct {
  int64_t offset, length;                /* elements */
  int32_t lag, group;
} lirec_adam_group_range;
int lirec_adam_hyper_write(lirec_adam_hyper* table_dev, const lirec_adam_hyper* rows_host, int32_t n_groups, lirec_stream_t stream);
int lirec_adam_step_groups(float* p, const float* g, float* m, float* v, const lirec_adam_group_range* ranges, int32_t count,
                           const lirec_adam_hyper* table_dev, int32_t n_groups, int32_t step, float grad_scale,
                           const int64_t* step_dev, int64_t* count_dev, int32_t* ticket, int32_t advance, lirec_stream_t stream);
int lirec_set_adam_hyper_row(const lirec_adam_hyper* row_dev);
#define LIREC_ADAM_MAP_MAX 16
int lirec_set_adam_hyper_map(const lirec_adam_hyper* table_dev, const lirec_adam_group_range* ranges, int32_t count);
/* `step_dev` (optional, device): when not NULL the 1-based step is read from it by the kernel instead of `step`
 * (bias corrections computed on the device), so that a captured graph advances through the steps.
 * lirec_counter_add: ctr[i] += inc[i] for i < n (n <= 4), one tiny kernel -- the "next step" node of such a graph. */
int lirec_counter_add(int64_t* ctr, const int64_t* inc_host, int32_t n, lirec_stream_t stream);

/* ---- evaluation counters on the device -------------------------
 * Precision.update_probs_max_tracks (utils/evaluation.py:114-176) and, with `rels`,
 * update_probs_max_tracks_rels (:179-271): per clip, padded tracks -> -inf, S = sigmoid; predicted track
 * = argmax_t S[t,y] (+ Q[t,r0] with the "None" column appended as 0, :220-222); joint prediction = first
 * flat argmax over (t,c) of S, or over (t,c,r) of S[t,c]+Q[t,r] (:229-235); then the two-pass bookkeeping over
 * the two ground-truth tracks (:150-175, :239-270).  The reference copies the logits to the host every batch
 * (mlp/test.py:50-67) and tiles a (B*T, C, NR) tensor in numpy; here one workgroup per clip adds into
 *   counters[0..6] = total, total_cl, total_rels, top1, trks_top1, cls_top1, rels_top1   (int64, device)
 * which the eval loop reads once at the end.  mem, y, r, g: as for the margin loss; with loader_types f64 /
 * i64 are read in place.  just_zeros: [B] bytes, NULL = none.
 * Size limit: 4 * (2*T*C + T*(2*NR+1) + 512) bytes of LDS per clip (the NR term only with rels) must not exceed 160 KiB --
 * LIREC_EINVAL otherwise (C = 101, NR = 15: T <= 173 with rels). */
typedef struct {
  const float* ints; int64_t ld_ints;     /* [B*T, C] logits */
  const float* rels; int64_t ld_rels;     /* [B*T, NR] or NULL */
  const float* mem;                       /* [B, T] 0/1 or NULL */
  const int32_t* y;                       /* [B] */
  const int32_t* r;                       /* [B, T] (NR = None); required with rels */
  const int32_t* g;                       /* [B, 2] gt_tracks */
  const uint8_t* just_zeros;              /* [B] or NULL */
  int64_t* counters;                      /* [8] in/out (accumulated) */
  int32_t B, T, C, NR;
  int32_t loader_types, reserved_;
} lirec_eval_args;
int lirec_eval_max_tracks(const lirec_eval_args* a, lirec_stream_t stream);

/* Precision.update_probs (utils/evaluation.py:68-107), the clip-level counters of the recipes WITHOUT a maximum over tracks:
 * top-1 / 3 / 5 of the clip's label, the two soft-label counters and the confusion matrix, accumulated on the device.
 * The reference sorts every row (np.argsort(-x)); here the order is stated without a sort.  Class j comes BEFORE class c of a
 * row x when x[j] > x[c], or when x[j] == x[c] and j < c (comparison by value: +0 and -0 tie); a NaN comes after every number,
 * and among NaNs the lower index first.  This is np.argsort(-x, kind='stable'), and what the reference's default argsort gives
 * on any row without ties.  rank(c) = the number of classes before c.  Per clip b, with x = logits + b*ld_logits (C values)
 * and y = the clip's label:
 *     total += 1;   top1 / top3 / top5 += rank(y) < 1 / 3 / 5;   conf[y, the class of rank 0] += 1
 *     with soft: r* = the minimum of rank(s) over the entries s of the clip's soft row that are whole numbers in [0, C)
 *                (rows are padded with -1; duplicates are harmless); top1_sf += (r* == 0), top5_sf += (r* < 5) -- the reference's
 *                "first of the top five that is a soft label".  A row without a valid entry counts in neither.
 *   counters[0..5] = total, top1, top3, top5, top1_sf, top5_sf   (int64, device; [6], [7] are not touched)
 * A LABEL OUTSIDE [0, C) COUNTS IN total ONLY: no hit and no conf entry.  The labels are device memory, which the host cannot
 * inspect without a visit, so the call cannot refuse them (the host restatement would raise an IndexError there).
 * One workgroup per clip: the row goes into LDS once, every thread ranks the classes it owns with C comparisons each, and the
 * workgroup adds its sums with one integer atomic per non-zero counter and one for conf (total: one atomic per launch).
 * INTEGER ATOMICS ONLY: the result does not depend on the order in which the workgroups arrive, run to run and bit for bit.
 *   logits: fp32, row b at logits + b*ld_logits; ld_logits may exceed C (int_rels evaluates row 0 of each clip's group of rows,
 *           inters.reshape(bs, -1, C)[:, 0], in place).
 *   y:      the label of clip b is y[b * y_stride] (elements; 0 means 1): int32, with loader_types the loader's int64.
 *   soft:   [B, n_soft], row stride ld_soft (elements): fp32, with loader_types the loader's float64.  NULL: the two soft
 *           counters are not touched.
 *   conf:   int64 [C, C] row-major, or NULL.
 * Size limit: C <= LIREC_EVAL_TOPK_MAX_C (8 bytes of LDS per class -- its key and its rank -- 32 KiB at the limit; the ranking
 * is C*C comparisons per clip, and C is 11 to 324 here).
 * LIREC_EINVAL before any device call for: a NULL struct, logits, y or counters; B < 0, C < 1, C over the limit,
 * ld_logits < C, y_stride < 0; soft with n_soft < 1 or ld_soft < n_soft; logits not 4-byte, counters / conf not 8-byte, y /
 * soft not 4-byte (loader_types: 8-byte) aligned.  B == 0: no launch, LIREC_OK.  Recorded into a command list like every other
 * launch (added to ABI 124 without a new number: a new export and a new struct, index 13 of lirec_abi_sizeof). */
#define LIREC_EVAL_TOPK_MAX_C 4096
typedef struct {
  const float* logits; int64_t ld_logits; /* [B, C] */
  const void* y; int64_t y_stride;        /* int32 (loader_types: int64) */
  const void* soft; int64_t ld_soft;      /* [B, n_soft] fp32 (loader_types: float64) or NULL */
  int64_t* counters;                      /* [8] in/out (accumulated) */
  int64_t* conf;                          /* [C, C] in/out (accumulated) or NULL */
  int32_t B, C, n_soft, loader_types;
} lirec_eval_topk_args;
int lirec_eval_clip_topk(const lirec_eval_topk_args* a, lirec_stream_t stream);

/* ---- predictions on the device ---------------------------------------------------
 * What the two evaluation calls decide per clip, WITHOUT labels: the answer for a clip instead of a counter.  One workgroup per
 * clip; every output element has one writer, no atomics: two launches on the same inputs give the same bytes.
 * Per clip b (lirec_eval_max_tracks stays the statement of record for these rules):
 *   a padded track (mem[b, t] == 0) has logits of -inf;  S = sigmoid(ints), Q = sigmoid(rels), in float;
 *   with rels a "None" column Q[t, NR] = 0 is appended;
 *   joint score: S[t, c] (float) without rels, (double)S[t, c] + (double)Q[t, r] with rels;
 *   (trk, cls[, rel]) = the FIRST flat index of its maximum in (t, c[, r]) order -- np.argmax over the reference's tiled tensor
 *   (utils/evaluation.py:144-147, :229-235), pairs that round to the same double included.
 * T = 1 with mem = NULL is the clip-level form (the recipes without a maximum over tracks).
 * Outputs (device; every pointer except `trk` may be NULL = not wanted):
 *   trk, cls, rel   int32 [B]     the joint prediction; rel in [0, NR] (NR = None), -1 without rels
 *   score           double [B]    the joint maximum
 *   trk_score       double [B, T] per track, max_c S (+ max_r Q over the NR + 1 columns, in double)
 *   top_cls         int32 [B, K]  the first min(K, C) classes of the PREDICTED track, ordered by that track's masked logits under
 *                                 the order of lirec_eval_clip_topk (value descending, the lower index first on ties, +0 == -0, NaN
 *                                 last); the remaining entries are -1
 *   top_cls_p       float [B, K]  the sigmoids of those classes; the remaining entries are 0
 *   top_rel, top_rel_p            the same over the NR real relationship logits of the predicted track; written only with rels
 *   flags           int32 [B]     bit 0: a NaN among the clip's unmasked logits; bit 1: no valid track (every mem entry is 0)
 * Two corners:
 *   top_cls[b, 0] is ordered by LOGIT, cls[b] by PROBABILITY: they can differ only where two different logits give the same float
 *   probability (a saturated sigmoid) -- top_cls then names the larger logit, cls the lower index.
 *   A clip with flag bit 1 has trk = cls = 0 (rel = 0 with rels) and scores of 0.  For a clip with flag bit 0 the joint fields
 *   (trk, cls, rel, score, trk_score) are whatever the shared argmax gives on NaN -- valid indices, otherwise not pinned; the top
 *   lists still put every NaN last.
 * mem: fp32, with loader_types the loader's float64, read in place.
 * Size limit: 4 * (T*C + T*(NR+1) + C + NR) + 8*T + 144 bytes of LDS per clip (the NR terms only with rels; probabilities, the two
 * rows of keys, the per-track maxima and the reduction slots) must not exceed 160 KiB (C = 101, NR = 15: T <= 342 with rels).
 * LIREC_EINVAL before any device call for: a NULL struct, ints or trk; B < 0, T < 1, C < 1, K outside 1..LIREC_PREDICT_MAX_K,
 * ld_ints < C; rels with NR < 1 or ld_rels < NR; a pointer that is not 4-byte aligned (8-byte: score, trk_score, and mem with
 * loader_types); a clip over the LDS limit.  B == 0: no launch, LIREC_OK.  Recorded into a command list like every other launch
 * (added to ABI 124 without a new number: a new export and a new struct, index 15 of lirec_abi_sizeof). */
#define LIREC_PREDICT_MAX_K 16
typedef struct {
  const float* ints; int64_t ld_ints;     /* [B*T, C] logits */
  const float* rels; int64_t ld_rels;     /* [B*T, NR] or NULL */
  const void* mem;                        /* [B, T] 0/1 fp32 (loader_types: float64) or NULL */
  int32_t* trk; int32_t* cls; int32_t* rel;          /* [B] */
  double* score;                          /* [B] */
  double* trk_score;                      /* [B, T] */
  int32_t* top_cls; float* top_cls_p;     /* [B, K] */
  int32_t* top_rel; float* top_rel_p;     /* [B, K] */
  int32_t* flags;                         /* [B] */
  int32_t B, T, C, NR, K, loader_types;
} lirec_predict_args;
int lirec_predict_clips(const lirec_predict_args* a, lirec_stream_t stream);
/* lirec_predict_clips with every non-NULL output pointer the base of a DATASET-SIZED array: clip b writes row cursor[0] + b of each
 * (trk_score: T doubles a row, the top lists: K entries a row).  cursor: an int64 device word the kernel reads when it runs (once
 * per workgroup), so the launch, recorded into a command list, writes where the cursor points at replay time.  The launch does not
 * move the cursor: lirec_counter_add(cursor, {B}, 1, stream) behind it does.  The same kernel body -- one workgroup per clip, one
 * writer per element, the same LDS limit -- and the same LIREC_EINVAL cases as lirec_predict_clips, plus a NULL or misaligned
 * (8 bytes) cursor; all before any device call, also under the dry run.  TRUSTED, as lirec_collate_fields_at trusts its cursor:
 * 0 <= cursor[0] and cursor[0] + B <= the arrays' rows.  (Added to ABI 124 without a new number: one new export, no struct changes.) */
int lirec_predict_clips_at(const lirec_predict_args* a, const int64_t* cursor, lirec_stream_t stream);
/* dst row cursor[0] + r = src row r for r < rows: fp32, `cols` values a row (any cols >= 1: no multiple of 4 asked), row strides
 * ld_src / ld_dst in elements (src may be a strided view: row 0 of each clip's group of rows).  What a forward-only command list
 * keeps a batch's rows with in a dataset-sized buffer (the deferred relationship logits of the clip-level evaluation).  cursor as
 * above: read by the kernel when it runs, not moved, trusted.  One launch, one writer per element.  LIREC_EINVAL before any device
 * call (also under the dry run) for a NULL src, dst or cursor; rows < 0, cols < 1, ld_src or ld_dst < cols; src / dst not 4-byte,
 * cursor not 8-byte aligned.  rows == 0: no launch, LIREC_OK.  (ABI 124: one new export.) */
int lirec_rows_copy_at(const float* src, int64_t ld_src, int32_t rows, int32_t cols, float* dst, int64_t ld_dst, const int64_t* cursor,
                       lirec_stream_t stream);
/* acc[0] += v[0] on the device, in the accumulator's own type: fp32 (acc_f64 == 0) or float64 -- the fp32 addend converted first, one
 * rounding: bit for bit what torch's `acc += v` gives on the same device tensors.  One thread, a plain load and store: launches on
 * one stream are ordered, and nothing else may write acc meanwhile.  LIREC_EINVAL (also under the dry run) for a NULL acc or v, acc
 * not 4-byte (float64: 8-byte) aligned, v not 4-byte aligned.  (ABI 124: one new export.) */
int lirec_scalar_accumulate(void* acc, int32_t acc_f64, const float* v, lirec_stream_t stream);

/* ---- collate on the device (resident piece store) ----------------------------------
 * The loader's per-batch work for a dataset whose pieces AND whose stacked sample tables are resident: what
 * lirec_amd.features.collate(store=, static_layout=True) + batch_to_device leave in the batch buffer, written by the device from
 * B sample ids.  Everything is exact (integer gathers and one prefix sum), on the given stream, without a read-back or an
 * allocation; every output element has one writer, so two calls on the same inputs give the same bytes.
 *   ids          int32 [B]          sample ids (rows of index_rows and of every field's source)
 *   index_rows   int32 [N, E, 3]    per sample E = T_max * (R + 1) entries: column 0 a clip-piece row, columns 1 and 2 track-piece
 *                                   rows, -1 = zeros
 *   n_clip_all, n_track_all         the piece stores' row counts; row n_all of a store is its zero row
 *   fields[nf]   {src, row_bytes, dst}: field f of sample s is the row_bytes bytes at src + s * row_bytes
 * Outputs (device):
 *   feature_index int32 [B, E, 3]   column 0: the position of the entry's clip row in clip_rows; columns 1, 2: of its track row in
 *                                   track_rows; a negative entry stays -1
 *   clip_rows    int32 [n_clip_list]   the distinct non-negative values of column 0 over the batch, ascending (u of them), then
 *                                   n_clip_all (the zero row) to the end of the list
 *   track_rows   int32 [n_track_list]  the same over columns 1 and 2 together, padded with n_track_all
 *   counts       int32 [2]          the used lengths with the zero-row entry: max(u, 1) + 1 per list
 *   fields[f].dst                   [B, row_bytes] bytes: dst row b = src row ids[b], byte for byte (16-, 8- or 4-byte moves where
 *                                   src, dst and row_bytes allow, else bytes)
 * workspace: lirec_collate_workspace_bytes(n_clip_all, n_track_all) bytes, 16-byte aligned: a byte map and a rank table per store.
 * The library owns its contents -- it is cleared inside every call, the caller promises nothing about it -- but two calls that
 * share a workspace must be ordered (the same stream).  Four commands per call: the clear, the marks (plain byte stores of 1: every
 * writer of a byte stores the same value), one workgroup per store that scans its map in chunks of 16384 rows with a carry and
 * writes the row list, its padding and the count, and the grid that writes feature_index and copies the field rows.
 * TRUSTED, not checked on the device: every id is in [0, N), every entry of index_rows in [-1, n_all) of its store, and the row
 * lists are long enough for the batch (n_list >= min(B * E [* 2 for tracks], n_all) + 1, collate's static layout).  The host
 * validates the tables once when it uploads them and the ids once per epoch.  (An entry outside its store is skipped by the
 * kernels -- no store goes out of bounds -- and its feature_index is then not meaningful.)
 * LIREC_EINVAL before any device call (also under the host-side dry run) for: a NULL struct; B, E, nf, n_*_all or workspace_bytes
 * negative; nf over LIREC_COLLATE_MAX_FIELDS; a row_bytes < 1; n_clip_list or n_track_list < 2; a workspace smaller than
 * lirec_collate_workspace_bytes or not 16-byte aligned; with B > 0: a NULL ids, index_rows, feature_index, clip_rows, track_rows,
 * counts or workspace, E < 1, a field with a NULL src or dst; an int32 pointer that is not 4-byte aligned.  B == 0: no launch,
 * LIREC_OK (the checks come first).  Recorded into a command list like every other launch (added to ABI 124 without a new number:
 * two new exports and a new struct, index 17 of lirec_abi_sizeof). */
#define LIREC_COLLATE_MAX_FIELDS 16
typedef struct {
  const void* src; int64_t row_bytes; void* dst;
} lirec_collate_field;
typedef struct {
  const int32_t* ids;                     /* [B] */
  const int32_t* index_rows;              /* [N, E, 3] */
  int32_t* feature_index;                 /* [B, E, 3] */
  int32_t* clip_rows; int32_t* track_rows;           /* [n_clip_list], [n_track_list] */
  int32_t* counts;                        /* [2] */
  void* workspace; int64_t workspace_bytes;
  int64_t n_clip_all, n_track_all, n_clip_list, n_track_list;
  int32_t B, E, nf, reserved_;
  lirec_collate_field fields[LIREC_COLLATE_MAX_FIELDS];
} lirec_collate_args;
/* (pure host arithmetic; -1 for a negative count) */
int64_t lirec_collate_workspace_bytes(int64_t n_clip_all, int64_t n_track_all);
int lirec_collate_resident(const lirec_collate_args* a, lirec_stream_t stream);
/* The field-row copy of lirec_collate_resident on its own (resident block store; index 23 of lirec_abi_sizeof = the field struct):
 * for every field f < nf, dst row b = src row ids[b], b < B, byte for byte with the same 16 / 8 / 4 / 1-byte moves.  ONE launch.
 * The batch's own id list is one more field (src = the table 0, 1, 2, ... as int32, row_bytes 4): it then sits at a fixed address
 * of the batch buffer, where lirec_feature_rows::clip_ids of a recorded step reads it.  ids are trusted as above.  LIREC_EINVAL
 * (also under the dry run) for B or nf negative, nf over LIREC_COLLATE_MAX_FIELDS, NULL fields with nf > 0, a row_bytes < 1, a
 * misaligned ids; with B > 0: NULL ids, a field with a NULL src or dst.  B == 0 (or nf == 0): no launch, LIREC_OK. */
int lirec_collate_fields(const int32_t* ids, int32_t B, const lirec_collate_field* fields, int32_t nf, lirec_stream_t stream);
/* lirec_collate_fields with the batch's ids read THROUGH A DEVICE WORD: ids = ids_base + *cursor, the cursor read by the kernel (once
 * per workgroup) when it runs -- so the launch, recorded into a command list, draws another batch at every replay: the batch the
 * cursor names then.  ids_base: the epoch's sample ids (int32, a stable address); cursor: an int64 device word, an offset in ids.
 * The same one launch, moves and blockIdx.y = field; no id outside [*cursor, *cursor + B) is read.  The launch does NOT move the
 * cursor: lirec_counter_add(cursor, {B}, 1, stream) directly behind it does (a launch of its own: every workgroup of this one
 * reads the word).  TRUSTED: 0 <= *cursor, *cursor + B <= the ids behind ids_base, every id a row of every field's source (the host
 * sets the cursor and validated the ids).  LIREC_EINVAL (also under the dry run) for a NULL or misaligned ids_base (4 bytes) or
 * cursor (8 bytes), B < 1, nf negative or over LIREC_COLLATE_MAX_FIELDS, NULL fields with nf > 0, a row_bytes < 1, a field with a
 * NULL src or dst.  nf == 0: no launch, LIREC_OK.  (Added to ABI 124 without a new number: one new export, no struct changes.) */
int lirec_collate_fields_at(const int32_t* ids_base, const int64_t* cursor, int32_t B, const lirec_collate_field* fields, int32_t nf,
                            lirec_stream_t stream);

/* ---- train-mode context sampling (resident piece store) ----------------------------
 * The reference's training loader draws np.random.choice(L, R, replace=False) from a context list of L > R clips on every
 * __getitem__ (mixed_utils/classification_dataloader.py:387, :405, :488).  Here the draw is made ONCE PER EPOCH for the whole
 * dataset, in place in the resident index_rows table that lirec_collate_resident reads; it is a function of (seed, epoch, sample,
 * candidate) alone -- lirec_amd.features.draw_context is the same rule in numpy.  A slot is a (sample s, candidate c) with an
 * over-long list; its id is s * T_max + c, i.e. its row of index_rows seen as [N * T_max, R + 1, 3].
 *   slot_dst    int32 [S]       slot ids (read as uint32)
 *   slot_off    int32 [S + 1]   ascending; the list of slot i is pool_rows[slot_off[i] .. slot_off[i + 1])
 *   pool_rows   int32 [P, 3]    (clip-piece row, track-1 row, track-2 row) of every list entry
 *   index_rows  int32 [N, E, 3] E = T_max * (R + 1); written in place
 *   seed, epoch                 by value
 * Entry j < L of slot i gets the key
 *   (uint64(word 0 of philox4x32_10(counter = (j, slot, LIREC_SITE_CONTEXT_DRAW, epoch), key = (seed lo, seed hi))) << 32) | j
 * and index_rows[slot, 1 + p, 0..2] = pool_rows[slot_off[i] + j_p] for p < R, j_p the entry with the p-th smallest key.  The keys of
 * a slot are distinct, so nothing depends on an order of execution: two calls give the same bytes.  Row 0 of the slot and every
 * other element of the table are not touched; every written element has one writer.  ONE launch, one workgroup per slot, a
 * slot's keys in LDS (8 bytes each: 32 KiB at LIREC_CONTEXT_LIST_MAX entries); exact integer work, plain vector stores.
 * TRUSTED, not checked on the device: every slot id below N * T_max, slot_off ascending from 0 to P with R < L <=
 * LIREC_CONTEXT_LIST_MAX per slot, every entry of pool_rows in [-1, n_all) of its store.  The host validates the tables once when
 * it uploads them.  (A list outside (0, LIREC_CONTEXT_LIST_MAX] is skipped by the kernel.)  The collate calls that read the table
 * must be ordered around the call: the same stream.
 * LIREC_EINVAL before any device call (also under the host-side dry run) for: a NULL struct; S negative; R < 1; E < R + 1; with
 * S > 0: a NULL slot_dst, slot_off, pool_rows or index_rows; a pointer that is not 4-byte aligned.  S == 0: no launch, LIREC_OK
 * (the checks come first).  Recorded into a command list like every other launch (added to ABI 124 without a new number: one new
 * export and a new struct, index 41 of lirec_abi_sizeof; 24 .. 40 stay unassigned). */
#define LIREC_CONTEXT_LIST_MAX 4096
typedef struct {
  const int32_t* slot_dst;                /* [S] */
  const int32_t* slot_off;                /* [S + 1] */
  const int32_t* pool_rows;               /* [P, 3] */
  int32_t* index_rows;                    /* [N, E, 3] */
  uint64_t seed;
  uint32_t epoch;
  int32_t S, R, E;
} lirec_draw_context_args;
int lirec_draw_context(const lirec_draw_context_args* a, lirec_stream_t stream);

/* ---- feature assembly ---------------------------------------------
 * The reference's loader tiles every row of the (B, T, R+1, D) feature block on the host as
 *   [ clip piece (text | clip-visual) | track-1 piece | track-2 piece ]
 * (mixed_utils/classification_dataloader.py:336-349, :419, :477-478, :496-497, :531-533, :558-565;
 * mixed_utils/mixed_features.py:115-125) and the block crosses PCIe every step (mlp/model.py:279-280).  Here only the
 * de-duplicated piece tables and an index cross it:
 *   out[row, :] = [ clip[index[row,0], :clip_dim] | track[index[row,1], :track_dim] | track[index[row,2], :track_dim] ]
 * with zeros for a negative index.  clip / track: fp32 (table_f64 = 0) or float64 tables (row strides ld_* in
 * elements); out: fp32 [rows, clip_dim + 2 track_dim] (ld_out in elements); clip_dim and track_dim multiples of 4,
 * tables / out 16-byte (float64: 16-byte) aligned. */
int lirec_gather_features(const void* clip, int64_t ld_clip, const void* track, int64_t ld_track, int32_t table_f64,
                          const int32_t* index, int64_t rows, int32_t clip_dim, int32_t track_dim,
                          float* out, int64_t ld_out, lirec_stream_t stream);
/* The same block written as bf16 (round to nearest even; `out`: [rows, clip_dim + 2 track_dim] bf16, ld_out in elements):
 * "bf16 feature storage" (x_bf16 of lirec_embed_fwd_args) fed straight from the piece tables. */
int lirec_gather_features_bf16(const void* clip, int64_t ld_clip, const void* track, int64_t ld_track, int32_t table_f64,
                               const int32_t* index, int64_t rows, int32_t clip_dim, int32_t track_dim,
                               void* out, int64_t ld_out, lirec_stream_t stream);

/* ---- raw feature pooling ------------------------------------------
 * What the reference's feature classes compute with numpy for a clip or a track that is not in their cache:
 * lirec_grid_pool: out[o, c] = max over the elements e in [estart[o], estart[o+1]) of the MEAN of
 *   grid[frame_e, c, y0_e:y1_e, x0_e:x1_e]   (boxes[e] = {frame, y0, y1, x0, x1}, half-open ranges)
 * = the clip-visual feature with one full-grid box per frame of the clip's frame range (visual_utils/
 * visual_features.py:60-103 spatial mean, mixed_utils/mixed_features.py:54 temporal max), and the track feature with the
 * person box of every track element (visual_features.py:105-134, mixed_features.py:104-105).  grid: fp32 [F, C, H, W];
 * a frame outside [0, F) contributes a zero row (:129), an empty box NaN, no element zeros.  The mean follows numpy's
 * float32 pairwise summation order: results equal np.mean bit for bit.
 * lirec_rows_max: out[o, :] = max over the rows idx[e], e in [estart[o], estart[o+1]), of src [*, ld] (the text feature
 * of a clip: tokens in its time range, text_utils/text_features.py:140-165, then np.max, mixed_features.py:61). */
int lirec_grid_pool(const float* grid, int32_t F, int32_t C, int32_t H, int32_t W, const int32_t* boxes,
                    const int32_t* estart, int32_t n_out, float* out, int64_t ld_out, lirec_stream_t stream);
int lirec_rows_max(const float* src, int64_t ld, const int32_t* idx, const int32_t* estart, int32_t n_out, int32_t dim,
                   float* out, int64_t ld_out, lirec_stream_t stream);

/* ---- utilities ---------------------------------------------------------------- */
/* float64 -> float32 (the DataLoader delivers float64, mlp/model.py:279 `.float()`) */
int lirec_cast_f64_f32(const double* src, float* dst, int64_t n, lirec_stream_t stream);
/* keep[row, col] (uint8) of one dropout site, for tests */
int lirec_dropout_mask(uint8_t* keep, int32_t rows, int32_t cols, const lirec_dropout* drop,
                       int32_t site, lirec_stream_t stream);
int lirec_version(void);
/* sizeof() of ABI struct `which` (5 = eval; 0 embed_fwd, 1 embed_bwd, 2 margin_loss, 3 dropout,
 * 4 rowsel, 6 linear_fwd, 7 linear_bwd, 8 embed_dx, 9 embed_dx_indexed, 10 adam_range, 11 adam_hyper, 12 adam_group_range,
 * 13 eval_topk, 15 predict, 17 collate, 19 clip_weights, 21 feature_rows, 23 collate_field, 41 draw_context, 43 param_stat_entry; 14, 16, 18, 20, 22, 24 .. 40 and 42 are not assigned) so a binding can verify its mirror;
 * -1 if unknown */
int lirec_abi_sizeof(int which);
/* GEMM core: 0 exact f32-input MFMA   1 one-thread-per-output HIP GEMM (bring-up cross-check)
 *            2 split-precision bf16x3 MFMA (fp32 in/out, ~2^-16 per product, up to 5.3x the f32 core)
 *            3 the bf16 core with ONE pass on the large GEMMs -- layer 1 and its weight gradient, the gate's forward / data /
 *              weight gradients: operands rounded to bf16 once, fp32 accumulate (~2^-9 per operand); every other GEMM as in 2.
 *              BASELINE config 5's arithmetic ("bf16, 32 tracks/clip stress"); outside the 1e-4 parity contract by design,
 *              never the headline (tests/test_gpu_onepass.py states and checks its tolerance) */
int lirec_set_gemm_mode(int mode);
int lirec_get_gemm_mode(void);
/* on != 0: every weight / bias gradient launched from now on OVERWRITES its buffer (dW = ..., db = ...) instead of accumulating
 * (+=).  For a caller that issues zero_grad + forward + backward + step as one unit (the recorded train step): the zeroing pass
 * over the gradient buffer (76 MB per step here) is then not needed.  Every parameter must receive exactly one gradient launch
 * per step (true for the models of this library; lirec_amd.graph checks it once per recording).  PER CALLING THREAD (like
 * lirec_grad_overwrite_conflicts): a backward that runs on another host thread -- an autograd engine thread, a loader thread -- is not
 * switched and accumulates; the Python side only enters the mode where loss.backward() takes the direct path on the calling thread
 * (lirec_amd.graph refuses to record anything else).  Default off. */
int lirec_set_grad_overwrite(int on);
/* The number of gradient buffers that were the target of MORE than one weight- / bias-gradient launch since the mode was last
 * switched on (calling thread): non-zero means overwriting would lose contributions -- keep the zeroing pass. */
int lirec_grad_overwrite_conflicts(void);
const char* lirec_error_string(int code);
/* Optional device scratch for split-K: the GEMMs whose output is small but whose reduction is deep
 * (weight gradients dW = dY^T X over all rows, the skinny head GEMMs) cut K into chunks so that
 * they fill the chip; partial tiles go to this buffer and a fixed-order reduce kernel sums them
 * (bitwise reproducible, no atomics).  Without scratch (NULL / 0) nothing is split.  The buffer is
 * used by the next GEMM launch, so all launches must be on one stream while it is registered.
 * 128 MiB covers the full-size model. */
int lirec_set_scratch(void* ptr, int64_t bytes);

/* Contexts.  The GEMM core (lirec_set_gemm_mode), the split-K scratch (lirec_set_scratch) and the diagnostic switches
 * (lirec_debug_set) are state of a context, and every thread has a current one -- the default context until
 * lirec_ctx_set_current(ctx) is called on that thread (NULL switches back).  All launches that use one context's scratch
 * must be on one stream; a host with two concurrent streams (training + evaluation) gives each its own context.
 * A new context starts with the default context's GEMM core and no scratch. */
int lirec_ctx_create(lirec_ctx_t* out);
int lirec_ctx_destroy(lirec_ctx_t ctx);
int lirec_ctx_set_current(lirec_ctx_t ctx);
lirec_ctx_t lirec_ctx_get_current(void);
/* Command lists: a recorded step re-issued from C.  Between lirec_record_begin() and lirec_record_end() every kernel launch,
 * memset and lirec_stream_wait made by the calling thread through this library is executed as usual AND appended -- kernel,
 * grid, arguments by value, stream -- to a list; lirec_cmdlist_replay(list, from, to) re-issues commands [from, to) (to < 0:
 * to the end) as plain launches on the streams they were recorded on.  The caller keeps every buffer the recorded calls
 * were given alive and at its address, and passes per-step scalars through device memory (lirec_dropout.seed_dev,
 * lirec_adam_step's step_dev, lirec_counter_add).  lirec_record_mark() = number of commands recorded so far: the host notes
 * it where it has work of its own to do between commands at replay time (the gradient all-reduces of a data-parallel step).
 * Replaces nothing in the reference (a plain eager loop, mlp/train.py:57-63); host time per step 0.9 ms -> ~0.1 ms with the
 * eager loop's kernel timeline (lirec_amd/graph.py, RecordedTrainStep). */
typedef struct lirec_cmdlist* lirec_cmdlist_t;
int lirec_record_begin(void);
int32_t lirec_record_mark(void);
int lirec_record_end(lirec_cmdlist_t* out);
int32_t lirec_cmdlist_size(lirec_cmdlist_t list);
int lirec_cmdlist_replay(lirec_cmdlist_t list, int32_t from, int32_t to);
/* Diagnostics: the same replay with the stream of command `lag_at` held back by `ticks` of the 100 MHz clock in front of that
 * command (tests: a recorded step's cross-stream dependencies must be events, not timing); lirec_cmdlist_command: the stream
 * command i is issued on (a stream wait: the signalling stream) and its kind (0 launch / memset, 1 stream wait, 2 profiling bracket). */
int lirec_cmdlist_replay_lagged(lirec_cmdlist_t list, int32_t from, int32_t to, int32_t lag_at, int64_t ticks);
int lirec_cmdlist_command(lirec_cmdlist_t list, int32_t i, lirec_stream_t* stream, int32_t* kind);
int lirec_cmdlist_destroy(lirec_cmdlist_t list);
/* `waiter` waits for everything enqueued on `signaller` so far (event record + stream wait; recorded like a launch). */
int lirec_stream_wait(lirec_stream_t waiter, lirec_stream_t signaller);
/* The same for n <= 4 waiters behind ONE event record on `signaller` (a record costs the signalling stream a ~6 us bubble on
 * this runtime; a fork that orders two side streams behind the same point pays it once). */
int lirec_stream_wait_many(const lirec_stream_t* waiters, int32_t n, lirec_stream_t signaller);
/* hipMemsetAsync(p, 0, bytes) on `stream`, recorded like a launch (optimizer.zero_grad inside a recorded step). */
int lirec_memset_zero(void* p, int64_t bytes, lirec_stream_t stream);
/* One kernel: zero `bytes` bytes at `p` (16-byte aligned) and ctr[i] += inc[i] for i < n <= 4 (n = 0: no counters).  The
 * first launch of a replayed step: optimizer.zero_grad() and lirec_counter_add() without a second launch between them. */
int lirec_zero_count(void* p, int64_t bytes, int64_t* ctr, const int64_t* inc, int32_t n, lirec_stream_t stream);
/* Device snapshot (the cut of an asynchronous checkpoint: lirec_amd.util.AsyncCheckpointer).  ONE kernel launch copies n <= 8
 * ranges, src[i] -> dst[i], bytes[i] bytes each, bit for bit, and in the same pass leaves in digests[i] the sum of range i's
 * 32-bit words modulo 2^64 -- an integer sum: the same bits in whatever order the workgroups add.  The three arrays are HOST
 * arrays, copied into the launch; digests: n 64-bit words in device memory, zeroed by the call itself (a memset on `stream` in
 * front of the launch; both are recorded when a recording is open).  LIREC_EINVAL before any device call for: n outside 1..8, a
 * null array or pointer, a src / dst pointer off a 16-byte boundary (digests: 8), bytes[i] negative or no multiple of 4, a dst
 * range that shares a byte with any src range, another dst range or the digest words.  bytes[i] = 0 is an empty range: digest 0. */
int lirec_snapshot(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n, uint64_t* digests,
                   lirec_stream_t stream);

/* Diagnostics (current context): `ablate` = k-loop ablation mask (4: no k-loop; planes kernels 16: no LDS-DMA, 32: no LDS
 * reads / MFMAs; 8: planes path off) -- results are garbage, only the timing is meaningful; 64: run-time split-K rule for the
 * row-compacted dW1, 128: split-K for GEMMs with an epilogue (both correct, both measured null / negative); 256 / 512: the
 * pre-round-2 tile orders of grouped NT / TN launches (correct; more L2 misses: see DESIGN 4.4); 4096: the split-K reduce kernel that
 * walks the problems inside every thread (same results, slower); 131072: lirec_linear_bwd_group puts a ~2 ms idle kernel in front of
 * its weight-gradient launches, 262144: the same in front of a row staging pass run ahead of its step (lirec_embed_fwd parts = 4) -- streams
 * made to lag on purpose: tests/test_gpu_recorded_bench_shape.py; `force_cfg` >= 0 forces one
 * tile configuration of the on-the-fly cores, -1 = automatic.  Never set by the product path. */
int lirec_debug_set(int ablate, int force_cfg);

/* Per-call-site timing with HIP events recorded on the launch stream (off by default).
 * enable(1) clears the accumulators; read() waits for the recorded events and returns, for
 * `site` in [0, lirec_profile_sites()): device milliseconds, launches, algorithmic FLOPs
 * (GEMM sites) and algorithmic bytes (HBM-bound sites) accumulated since enable(1). */
int lirec_profile_enable(int on);
int lirec_profile_sites(void);
const char* lirec_profile_site_name(int site);
int lirec_profile_read(int site, double* ms, int64_t* launches, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* LIREC_HIP_H */
