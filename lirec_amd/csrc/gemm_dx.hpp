// Input-feature gradient of the first layers (lirec_embed_dx):  dX[row(m), in_off_s + n] = sum_k dZ1_s[m, k] W1_s[k, n]
// for every (head, segment) problem of the call, in ONE grouped launch, plus the zero pass over what no problem writes.
//
// Shapes: M = the head's rows (the compact row list of the context head), K = J (512 at the bench shape: 16 k-steps of 32),
// N = in_dim of the segment (768 / 2048).  A short k-loop under a wide, write-heavy output: the tile is 128 x 128 with a
// one-barrier-pair k-loop and the next k-tile's global loads in flight during the MFMA block; nothing persistent, no split-K
// (each output element has exactly one writer, so the result is written once, straight into the caller's block).
//
// Operands:
//   A = dZ1 as the backward left it: fp32 rows (A), or bf16 hi / lo planes (A_hi, A_lo; A_lo NULL = the hi plane only --
//       the single-pass mode keeps no lo plane), row-major [rows32][lda].  Staged to LDS as fp32 (hi + lo is exact in fp32).
//   B = W1_s [K][N] fp32 row-major (the nn.Linear weight: out = J rows, in_dim columns), staged to LDS transposed ([n][k]).
// Cores: CORE 0 = v_mfma_f32_32x32x2_f32 (exact fp32 products, GEMM modes 0 and 1); CORE 1 = bf16x3 on
// v_mfma_f32_32x32x16_bf16 (a = a_hi + a_lo, b = b_hi + b_lo, the lo * lo term dropped; GEMM modes 2 and 3), both operands
// split on the fragment read.
// Output: row m of a problem is logical row L = rowmap ? rowmap[m] : m, physical row (L / gs) * gstride + goff + L % gs of the
// caller's (n, R+1, D) block (ld = ldc elements); fp32, or bf16 (round to nearest even) for a bf16 leaf.  Vector stores only.
//
// The same tiles serve the gradient of de-duplicated piece tables (lirec_embed_dx_indexed, dxi_gemm_kernel): a problem is one
// table segment, its A operand the per-piece sums S of the hidden-layer gradient that lirec_embed_dw1_indexed left (fp32), and
// its k-loop runs over a list of up to four (S, W1) chunks of K = J each -- one per (head, segment) that reads the table
// segment -- so each output element still has one writer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lirec {

enum { DX_MAX_PROB = 8 };

struct DxProblem {
  const float* A; const unsigned short* A_hi; const unsigned short* A_lo; long lda;
  const float* B; long ldb;
  int M, N, K;
  const int* dyn;                 // device row count bounding M (compact context rows), or NULL
  const int* rowmap;              // compact row -> logical row, or NULL
  int gs, gstride, goff;
  long c_off;                     // column of the segment in the output rows (in_off)
  int tiles_n, tile_start;
};

struct DxGroup {
  DxProblem p[DX_MAX_PROB];
  int nprob;
  void* C; long ldc; int out_bf16;
};

// Zero pass: every element of the (n, rp1, D) block that no problem writes.  Row r of candidate c belongs to head h when
// r in [goff_h, goff_h + gs_h); it is written in that head's segment columns when the head computes it (every row, or -- with
// a row map -- the rows listed for candidate c in rowmap[cstart[c] .. cstart[c + 1])).
struct DxZeroHead {
  int gs, goff, nseg;
  int in_off[4], in_dim[4];
  const int* rowmap; const int* cstart;
  int computed;                   // 0: the head does not exist (its rows are all zero)
};
struct DxZero {
  DxZeroHead h[2];
  int nh, rp1, D;
  void* C; long ldc; int out_bf16;
};

// lirec_embed_dx_indexed: C[m, c_off + n] = sum over the chunks c of A_c[m, :] B_c[:, n]  (K = J per chunk), rows m < Ma read,
// rows [Ma, M) written as 0 (the table's trailing zero row); fp32 output, plain row addressing.
enum { DXI_MAX_PROB = 3, DXI_MAX_CHUNK = 4 };

struct DxiProblem {
  const float* A[DXI_MAX_CHUNK]; const float* B[DXI_MAX_CHUNK];
  long lda, ldb;                  // (the same for every chunk: 2J for S, in_dim for W1)
  int nchunk, M, Ma, N, K;
  float* C; long ldc; long c_off;
  int tiles_n, tile_start;
};

struct DxiGroup {
  DxiProblem p[DXI_MAX_PROB];
  int nprob;
};

typedef float dx_f32x16 __attribute__((ext_vector_type(16)));
typedef float dx_f32x4 __attribute__((ext_vector_type(4)));
typedef float dx_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 dx_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dx_bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned dx_u32x4 __attribute__((ext_vector_type(4)));

// a = hi + lo with hi = bf16_rne(a), lo = bf16_rne(a - hi) (the split of gemm_bf16x3.hpp), two elements per call
__device__ __forceinline__ void dx_split2(float x0, float x1, unsigned& hi, unsigned& lo) {
  const dx_f32x2 v = {x0, x1};
  const dx_bf16x2 h = __builtin_convertvector(v, dx_bf16x2);
  const unsigned w = __builtin_bit_cast(unsigned, h);
  const dx_f32x2 f = {__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
  const dx_f32x2 r = v - f;
  hi = w;
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, dx_bf16x2));
}

// eight consecutive fp32 values of an LDS row -> their hi and lo bf16 halves (one MFMA fragment each)
__device__ __forceinline__ void dx_frag(const float* s, dx_bf16x8& hi, dx_bf16x8& lo) {
  const dx_f32x4 x = *reinterpret_cast<const dx_f32x4*>(s), y = *reinterpret_cast<const dx_f32x4*>(s + 4);
  unsigned h0, h1, h2, h3, l0, l1, l2, l3;
  dx_split2(x[0], x[1], h0, l0); dx_split2(x[2], x[3], h1, l1);
  dx_split2(y[0], y[1], h2, l2); dx_split2(y[2], y[3], h3, l3);
  const dx_u32x4 h = {h0, h1, h2, h3}, l = {l0, l1, l2, l3};
  hi = __builtin_bit_cast(dx_bf16x8, h);
  lo = __builtin_bit_cast(dx_bf16x8, l);
}

__device__ __forceinline__ unsigned short dx_bf16_rne(float x) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  if ((u & 0x7f800000u) == 0x7f800000u) return (unsigned short)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));   // inf / NaN
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float dx_bf(unsigned short h) { return __builtin_bit_cast(float, (unsigned)h << 16); }

// One k-tile (BK = 32) of the 128 x 128 tile from the LDS operands (rows of P = 36 floats, B transposed): each wave adds its
// 64 x 64 quarter, 2 x 2 blocks of 32 x 32.
template <int CORE>
__device__ __forceinline__ void dx_mma_ktile(const float* As, const float* Bs, dx_f32x16 (&acc)[2][2], int wm0, int wn0,
                                             int l31, int lh) {
  constexpr int BK = 32, P = BK + 4;
  if constexpr (CORE == 0) {
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = As[(wm0 + 32 * i + l31) * P + kk + lh];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = Bs[(wn0 + 32 * j + l31) * P + kk + lh];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < BK; kk += 16) {
      dx_bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) dx_frag(As + (wm0 + 32 * i + l31) * P + kk + 8 * lh, ah[i], al[i]);
#pragma unroll
      for (int j = 0; j < 2; ++j) dx_frag(Bs + (wn0 + 32 * j + l31) * P + kk + 8 * lh, bh[j], bl[j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // (the small terms first, as gemm_bf16x3.hpp)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
  }
}

template <int CORE>
__global__ void __launch_bounds__(256) dx_gemm_kernel(const DxGroup g) {
  constexpr int BM = 128, BN = 128, BK = 32, P = BK + 4;     // LDS rows of 36 floats: 16-byte aligned, rows spread over banks
  __shared__ float As[BM * P];
  __shared__ float Bs[BN * P];
  int pi = 0;
  while (pi + 1 < g.nprob && (int)blockIdx.x >= g.p[pi + 1].tile_start) ++pi;
  const DxProblem& p = g.p[pi];
  const int t = (int)blockIdx.x - p.tile_start;
  const int tm = t / p.tiles_n, tn = t - tm * p.tiles_n;
  int M = p.M;
  if (p.dyn) { const int d = *p.dyn; M = d < M ? d : M; }
  const int m0 = tm * BM, n0 = tn * BN;
  if (m0 >= M) return;                                       // (grid sized for the full row count: surplus tiles leave)
  const int N = p.N, K = p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;

  // global -> registers: A rows (tid >> 3) + 32 i, columns 4 (tid & 7) .. +3; B rows k 4 (tid >> 5) .. +3, columns 4 (tid & 31) .. +3
  dx_f32x4 ra[4], rb[4];
  auto load = [&](int k0) {
    const int ka = k0 + 4 * (tid & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + (tid >> 3) + 32 * i;
      dx_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < M && ka < K) {
        if (p.A) {
          v = *reinterpret_cast<const dx_f32x4*>(p.A + (long)m * p.lda + ka);
        } else {
          const ushort4 h = *reinterpret_cast<const ushort4*>(p.A_hi + (long)m * p.lda + ka);
          v[0] = dx_bf(h.x); v[1] = dx_bf(h.y); v[2] = dx_bf(h.z); v[3] = dx_bf(h.w);
          if (p.A_lo) {
            const ushort4 l = *reinterpret_cast<const ushort4*>(p.A_lo + (long)m * p.lda + ka);
            v[0] += dx_bf(l.x); v[1] += dx_bf(l.y); v[2] += dx_bf(l.z); v[3] += dx_bf(l.w);
          }
        }
      }
      ra[i] = v;
    }
    const int n = n0 + 4 * (tid & 31), kb = k0 + 4 * (tid >> 5);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dx_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < N && kb + j < K) v = *reinterpret_cast<const dx_f32x4*>(p.B + (long)(kb + j) * p.ldb + n);
      rb[j] = v;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<dx_f32x4*>(As + ((tid >> 3) + 32 * i) * P + 4 * (tid & 7)) = ra[i];
    const int nl = 4 * (tid & 31), kl = 4 * (tid >> 5);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const dx_f32x4 v = {rb[0][c], rb[1][c], rb[2][c], rb[3][c]};
      *reinterpret_cast<dx_f32x4*>(Bs + (nl + c) * P + kl) = v;
    }
  };

  dx_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = (K + BK - 1) / BK;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    store();
    __syncthreads();
    if (kt + 1 < nk) load((kt + 1) * BK);                    // in flight during the MFMA block
    dx_mma_ktile<CORE>(As, Bs, acc, wm0, wn0, l31, lh);
    __syncthreads();
  }

  // epilogue: lane holds rows (r & 3) + 8 (r >> 2) + 4 lh of each 32 x 32 block, column l31 -- a half-wave stores 32
  // consecutive elements of one row
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (m >= M) continue;
      const int L = p.rowmap ? p.rowmap[m] : m;
      const long row = (long)(L / p.gs) * p.gstride + p.goff + L % p.gs;
      const long base = row * g.ldc + p.c_off;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn0 + 32 * j + l31;
        if (n >= N) continue;
        if (g.out_bf16) reinterpret_cast<unsigned short*>(g.C)[base + n] = dx_bf16_rne(acc[i][j][r]);
        else reinterpret_cast<float*>(g.C)[base + n] = acc[i][j][r];
      }
    }
  }
}

// One workgroup per candidate.  A row no problem writes is zeroed whole (16-byte / 8-byte stores, D / 4 per row spread over the
// workgroup); a row a head writes only outside that head's segments -- nothing at all when they cover [0, D), the usual case.
__device__ __forceinline__ void dx_zero_span(const DxZero& z, long row, int c0, int c1, int tid) {
  const long at0 = row * z.ldc;
  int a = c0;
  while (a < c1 && (a & 3)) { if (a - c0 == tid) { if (z.out_bf16) reinterpret_cast<unsigned short*>(z.C)[at0 + a] = 0; else reinterpret_cast<float*>(z.C)[at0 + a] = 0.f; } ++a; }
  const int q0 = a / 4, q1 = c1 / 4;
  for (int q = q0 + tid; q < q1; q += 256) {
    if (z.out_bf16) *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(z.C) + at0 + 4 * q) = make_uint2(0u, 0u);
    else *reinterpret_cast<float4*>(reinterpret_cast<float*>(z.C) + at0 + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int e = (q1 > q0 ? 4 * q1 : a) + tid; e < c1; e += 256) {
    if (z.out_bf16) reinterpret_cast<unsigned short*>(z.C)[at0 + e] = 0; else reinterpret_cast<float*>(z.C)[at0 + e] = 0.f;
  }
}

__global__ void __launch_bounds__(256) dx_zero_kernel(const DxZero z) {
  __shared__ unsigned char written[1024];                    // row r of this candidate computed by its head (rp1 <= 1024)
  __shared__ signed char owner[1024];                        // head of row r, or -1
  const int c = blockIdx.x, tid = threadIdx.x;
  for (int r = tid; r < z.rp1; r += 256) {
    signed char o = -1;
    unsigned char w = 0;
    for (int h = 0; h < z.nh; ++h)
      if (r >= z.h[h].goff && r < z.h[h].goff + z.h[h].gs) { o = (signed char)h; w = (z.h[h].computed && !z.h[h].rowmap) ? 1 : 0; }
    owner[r] = o; written[r] = w;
  }
  __syncthreads();
  for (int h = 0; h < z.nh; ++h) {
    const DxZeroHead& hh = z.h[h];
    if (!hh.computed || !hh.rowmap) continue;
    const int j0 = hh.cstart[c], j1 = hh.cstart[c + 1];
    for (int j = j0 + tid; j < j1; j += 256) written[hh.goff + (hh.rowmap[j] - c * hh.gs)] = 1;
  }
  __syncthreads();
  for (int r = 0; r < z.rp1; ++r) {
    const long row = (long)c * z.rp1 + r;
    const int o = owner[r];
    if (o < 0 || !written[r]) { dx_zero_span(z, row, 0, z.D, tid); continue; }
    // the gaps between the head's segments (sorted by the host), before the first and after the last
    const DxZeroHead& hh = z.h[o];
    int at = 0;
    for (int s = 0; s < hh.nseg; ++s) {
      if (hh.in_off[s] > at) dx_zero_span(z, row, at, hh.in_off[s], tid);
      if (hh.in_off[s] + hh.in_dim[s] > at) at = hh.in_off[s] + hh.in_dim[s];
    }
    if (at < z.D) dx_zero_span(z, row, at, z.D, tid);
  }
}

// The piece-table gradient: dx_gemm_kernel's tile, its k-loop over the problem's chunks in order (nk k-tiles each; the next
// k-tile's loads -- across a chunk boundary too -- in flight during the MFMA block).  Rows [Ma, M) -- the trailing zero row --
// are stored as 0 whatever A and B hold.
template <int CORE>
__global__ void __launch_bounds__(256) dxi_gemm_kernel(const DxiGroup g) {
  constexpr int BM = 128, BN = 128, BK = 32, P = BK + 4;
  __shared__ float As[BM * P];
  __shared__ float Bs[BN * P];
  int pi = 0;
  while (pi + 1 < g.nprob && (int)blockIdx.x >= g.p[pi + 1].tile_start) ++pi;
  const DxiProblem& p = g.p[pi];
  const int t = (int)blockIdx.x - p.tile_start;
  const int tm = t / p.tiles_n, tn = t - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int M = p.M, Ma = p.Ma, N = p.N, K = p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  const int nk = (K + BK - 1) / BK, nt = p.nchunk * nk;

  dx_f32x4 ra[4], rb[4];
  auto load = [&](int it) {
    const int c = it / nk, k0 = (it - c * nk) * BK;
    const float* A = p.A[c];
    const float* B = p.B[c];
    const int ka = k0 + 4 * (tid & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + (tid >> 3) + 32 * i;
      dx_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < Ma && ka < K) v = *reinterpret_cast<const dx_f32x4*>(A + (long)m * p.lda + ka);
      ra[i] = v;
    }
    const int n = n0 + 4 * (tid & 31), kb = k0 + 4 * (tid >> 5);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dx_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < N && kb + j < K) v = *reinterpret_cast<const dx_f32x4*>(B + (long)(kb + j) * p.ldb + n);
      rb[j] = v;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<dx_f32x4*>(As + ((tid >> 3) + 32 * i) * P + 4 * (tid & 7)) = ra[i];
    const int nl = 4 * (tid & 31), kl = 4 * (tid >> 5);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const dx_f32x4 v = {rb[0][c], rb[1][c], rb[2][c], rb[3][c]};
      *reinterpret_cast<dx_f32x4*>(Bs + (nl + c) * P + kl) = v;
    }
  };

  dx_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nt > 0) load(0);
  for (int it = 0; it < nt; ++it) {
    store();
    __syncthreads();
    if (it + 1 < nt) load(it + 1);
    dx_mma_ktile<CORE>(As, Bs, acc, wm0, wn0, l31, lh);
    __syncthreads();
  }

  // epilogue as dx_gemm_kernel's: a half-wave stores 32 consecutive elements of one row
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (m >= M) continue;
      float* row = p.C + (long)m * p.ldc + p.c_off;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn0 + 32 * j + l31;
        if (n < N) row[n] = m < Ma ? acc[i][j][r] : 0.f;
      }
    }
  }
}

}  // namespace lirec
