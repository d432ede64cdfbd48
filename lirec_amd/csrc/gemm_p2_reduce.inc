// The body of gemm_p2_tn_reduce_kernel, included three times by gemm_p2.hpp (P2_RED_ROW 0, 1, 2) -- not a header of its own.
//   P2_RED_ROW 0: template <bool ADAM> gemm_p2_tn_reduce_kernel, text and code as they always were.
//   P2_RED_ROW 1: gemm_p2_tn_reduce_row_kernel -- the folded update under device-resident hyper-parameters
//                 (lirec_set_adam_hyper_row): lr, betas, eps and weight decay come from `row` in device memory, one uniform load
//                 per workgroup, and the bias corrections are computed here from the row's values, also for the by-value `step`
//                 (the host cannot pre-compute them from values it does not know).  A row whose `decoupled` word is not 0
//                 gets the AdamW form of adam4 / adam1 (one workgroup-uniform branch).
//   P2_RED_ROW 2: gemm_p2_tn_reduce_map_kernel -- the same with ONE ROW PER PARAMETER (lirec_set_adam_hyper_map): the workgroup
//                 looks the group of its problem's C and the group of its bias up in `map` (ranges of the flat layout, by their
//                 offsets from ad.g: uniform values), loads those rows of `table` and computes the bias corrections per row.
// Two kernels from one text, not one device function inlined into both: the launches without the feature keep their symbols,
// their arguments AND their instructions (an inlined body moved the register allocation of the <true> instantiation).
#if !P2_RED_ROW
template <bool ADAM>
static __global__ __launch_bounds__(256) void gemm_p2_tn_reduce_kernel(const GemmGroup g, const int nrep, const int Gr_, const AdamFuse ad) {
#elif P2_RED_ROW == 1
static __global__ __launch_bounds__(256) void gemm_p2_tn_reduce_row_kernel(const GemmGroup g, const int nrep, const int Gr_, const AdamFuse ad_in,
                                                                           const AdamHyperRow* __restrict__ row, const int step) {
  constexpr bool ADAM = true;
  AdamFuse ad = ad_in;
  bool decoupled;
  float decay;
  {
    const AdamHyperRow h = *row;
    ad.lr = h.lr; ad.beta1 = h.beta1; ad.beta2 = h.beta2; ad.eps = h.eps; ad.wd = h.wd;
    decoupled = h.decoupled != 0.f;
    decay = adam_decay(h);
  }
#else
static __global__ __launch_bounds__(256) void gemm_p2_tn_reduce_map_kernel(const GemmGroup g, const int nrep, const int Gr_, const AdamFuse ad_in,
                                                                           const AdamHyperRow* __restrict__ table, const AdamHyperMap map,
                                                                           const int step) {
  constexpr bool ADAM = true;
  AdamFuse ad = ad_in, adb = ad_in;        // (the weights' values, the bias's)
  bool decoupled = false, decoupled_b = false;
  float decay = 1.f, decay_b = 1.f;
#endif
  const long Gr = Gr_;
  int tile = blockIdx.x / P2_RED_PARTS;
  const int part = blockIdx.x - tile * P2_RED_PARTS;
  // tile -> (problem, nt, rep)
  int pi = 0;
  long P = 0;
  for (; pi < g.nprob; ++pi) {
    const int nt_all = (g.p[pi].N >> 8) * nrep;
    if (tile < nt_all) break;
    tile -= nt_all;
    P += p2_tn_len(g.p[pi]) * (g.p[pi].N >> 8);
  }
  if (pi >= g.nprob) return;
  const GemmProblem& p = g.p[pi];
  const int nt = tile / nrep, rep = tile - nt * nrep;
  const int tid = threadIdx.x;
  const long ks = p2_tn_ks(p), len = p2_tn_len(p), T = p2_tn_total(g);
  const bool do_db = p.dbias != nullptr && nt == 0 && part == 0;
  float step_size = ad.step_size, bc2_sqrt = ad.bc2_sqrt;
#if P2_RED_ROW == 2
  float step_size_b = ad.step_size, bc2_sqrt_b = ad.bc2_sqrt;
  {
    // the rows of this problem's weight and of its bias: map entries hold whole parameters, so the first element decides; the
    // host has checked that both lie in an entry (entry 0 otherwise: a row of the table in any case)
    const long oc = p.C - ad.g, ob = do_db ? p.dbias - ad.g : -1;
    int gc = map.group[0], gb = map.group[0];
    for (int i = 0; i < map.count; ++i) {
      if (oc >= map.off[i] && oc < map.end[i]) gc = map.group[i];
      if (ob >= map.off[i] && ob < map.end[i]) gb = map.group[i];
    }
    const double t = ad.step_dev ? (double)*ad.step_dev : (double)step;
    const AdamHyperRow h = table[gc];
    ad.lr = h.lr; ad.beta1 = h.beta1; ad.beta2 = h.beta2; ad.eps = h.eps; ad.wd = h.wd;
    decoupled = h.decoupled != 0.f;
    decay = adam_decay(h);
    step_size = (float)((double)h.lr / (1.0 - pow((double)h.beta1, t)));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)h.beta2, t));
    if (do_db) {
      const AdamHyperRow hb = table[gb];
      adb.lr = hb.lr; adb.beta1 = hb.beta1; adb.beta2 = hb.beta2; adb.eps = hb.eps; adb.wd = hb.wd;
      decoupled_b = hb.decoupled != 0.f;
      decay_b = adam_decay(hb);
      step_size_b = (float)((double)hb.lr / (1.0 - pow((double)hb.beta1, t)));
      bc2_sqrt_b = (float)sqrt(1.0 - pow((double)hb.beta2, t));
    }
  }
#else
  if constexpr (ADAM) {
#if P2_RED_ROW
    {                       // always here, in double, from the row's values: a by-value step t behaves as step_dev holding t
      const double t = ad.step_dev ? (double)*ad.step_dev : (double)step;
#else
    if (ad.step_dev) {      // step kept on the device (replays): the same double-precision bias corrections as adam_kernel
      const double t = (double)*ad.step_dev;
#endif
      step_size = (float)((double)ad.lr / (1.0 - pow((double)ad.beta1, t)));
      bc2_sqrt = (float)sqrt(1.0 - pow((double)ad.beta2, t));
    }
  }
#endif
  // what happens to the final gradient of this thread's float4 q at C + e: stored (unless C holds it already), and, ADAM, applied
  auto finish = [&](f32x4* cp, const f32x4 o, bool store) {
    if (store) *cp = o;
    if constexpr (ADAM) {
      const long off = reinterpret_cast<const float*>(cp) - ad.g;
#if P2_RED_ROW
      const f32x4 pn = decoupled ? adam4<true>(ad, step_size, bc2_sqrt, off, o, decay) : adam4(ad, step_size, bc2_sqrt, off, o);
#else
      const f32x4 pn = adam4(ad, step_size, bc2_sqrt, off, o);
#endif
      if (p.aux_out) {      // the new weights as q32b [M][N] (rows of C): 8 bytes of hi halves, 8 of lo
        const long row = (reinterpret_cast<const float*>(cp) - p.C) / p.ldc, col = (reinterpret_cast<const float*>(cp) - p.C) - row * p.ldc;
        if (ad.wq16c) {     // (single-pass mode: bf16 values, 64-column blocks)
          *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(p.aux_out) + (((row >> 5) * (p.ldc >> 6) + (col >> 6)) * 32 + (row & 31)) * 128 + (col & 63) * 2) = hi4(pn);
        } else {
          uint2 h2, l2;
          split4(pn, h2, l2);
          unsigned char* q = reinterpret_cast<unsigned char*>(p.aux_out) + (((row >> 5) * (p.ldc >> 5) + (col >> 5)) * 32 + (row & 31)) * 128 + (col & 31) * 2;
          *reinterpret_cast<uint2*>(q) = h2;
          *reinterpret_cast<uint2*>(q + 64) = l2;
        }
      }
    }
  };
  auto finish_db = [&](float db, bool store) {
    float* bp = p.dbias + 256 * rep + tid;
    if (store) *bp = db;
#if P2_RED_ROW == 2
    if (decoupled_b) (void)adam1<true>(adb, step_size_b, bc2_sqrt_b, bp - ad.g, db, decay_b);
    else (void)adam1(adb, step_size_b, bc2_sqrt_b, bp - ad.g, db);
#elif P2_RED_ROW
    if (decoupled) (void)adam1<true>(ad, step_size, bc2_sqrt, bp - ad.g, db, decay);
    else (void)adam1(ad, step_size, bc2_sqrt, bp - ad.g, db);
#else
    if constexpr (ADAM) (void)adam1(ad, step_size, bc2_sqrt, bp - ad.g, db);
#endif
  };
  long e[P2_RED_Q];
#pragma unroll
  for (int q = 0; q < P2_RED_Q; ++q) e[q] = ((long)(part * P2_RED_Q + q) * 256 + tid) * 4;
  auto cptr = [&](int q) { return reinterpret_cast<f32x4*>(p.C + (long)(256 * rep + (int)(e[q] >> 8)) * p.ldc + 256 * nt + (int)(e[q] & 255)); };
  if (ks <= 0 || T <= 0) {
    // No row to reduce over (the device-side count of the compact context rows is 0): the GEMM launch skipped this problem.
    // Accumulating gradients (beta = 1) are then right as they stand; OVERWRITTEN ones (beta = 0: the recorded step, which has
    // no zeroing pass) must be stored as zeros, or the previous step's values would reach the optimiser.
#pragma unroll
    for (int q = 0; q < P2_RED_Q; ++q) {
      f32x4* cp = cptr(q);
      if (p.beta == 0.f) finish(cp, f32x4{0.f, 0.f, 0.f, 0.f}, true);
      else if (ADAM) finish(cp, *cp, false);
    }
    if (do_db) {
      if (p.dbias_set) finish_db(0.f, true);
      else if (ADAM) finish_db(p.dbias[256 * rep + tid], false);
    }
    return;
  }
  const long S = P + (long)nt * len;
  long r = (long)((unsigned)S * (unsigned)Gr / (unsigned)T);
  if (r > Gr - 1) r = Gr - 1;
  while (r + 1 < Gr && p2_cut(r + 1, T, Gr) <= S) ++r;
  while (r > 0 && p2_cut(r, T, Gr) > S) --r;
  // this thread's float4 q: row = (part * P2_RED_Q + q) * 4 + tid / 64, col = 4 (tid % 64)
  f32x4 v[P2_RED_Q];
#pragma unroll
  for (int q = 0; q < P2_RED_Q; ++q) v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db = 0.f;
  bool any = false, whole = false;
  for (; r < Gr; ++r) {
    const long ar = p2_cut(r, T, Gr), br = p2_cut(r + 1, T, Gr);
    if (ar >= S + len) break;
    int k0, k1;
    p2_tn_ksteps(ar, br, S, len, k0, k1);
    if (k1 <= k0) continue;
    if (k0 == 0 && k1 == ks) { whole = true; break; }      // a whole tile: its workgroup has added it to C already
    const long sid = (r * 2 + (ar >= S ? 0 : 1)) * nrep + rep;
    const float* sl = g.p[0].slab + sid * P2::SLAB;
    f32x4 s[P2_RED_Q];
#pragma unroll
    for (int q = 0; q < P2_RED_Q; ++q) s[q] = *reinterpret_cast<const f32x4*>(sl + e[q]);
#pragma unroll
    for (int q = 0; q < P2_RED_Q; ++q) { v[q][0] += s[q][0]; v[q][1] += s[q][1]; v[q][2] += s[q][2]; v[q][3] += s[q][3]; }
    if (do_db) db += g.p[0].dbias_slab[sid * 256 + tid];
    any = true;
  }
  if (whole || !any) {
    if constexpr (ADAM) {
#pragma unroll
      for (int q = 0; q < P2_RED_Q; ++q) { f32x4* cp = cptr(q); finish(cp, *cp, false); }
      if (do_db) finish_db(p.dbias[256 * rep + tid], false);
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < P2_RED_Q; ++q) {
    f32x4* cp = cptr(q);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (p.beta != 0.f) o = *cp;
    o[0] += v[q][0]; o[1] += v[q][1]; o[2] += v[q][2]; o[3] += v[q][3];
    finish(cp, o, true);
  }
  if (do_db) finish_db(p.dbias_set ? db : p.dbias[256 * rep + tid] + db, true);
}
