// Split-K weight gradient of a Linear layer on fp32 operands (gfx950).
//
// wgrad_splitk_f32: gw[M, N] = sum_k g[k, m] * x[k, n] for contiguous fp32
// g [K, M] and x [K, N], fp32 out.  The decomposition is that of
// wgrad_splitk.hip (partial kernel into slab[slice][M][Np], fixed-order finish
// kernel, plain stores, no atomics); the tile and the operand path are fp32's
// own.
//
// MFMA.  v_mfma_f32_32x32x2_f32:
//   A: lane l supplies row l % 32,    k = l / 32
//   B: lane l supplies column l % 32, k = l / 32
//   C: register r of lane l is row 8 * (r / 4) + 4 * (l / 32) + r % 4,
//      column l % 32
// with A = x and B = g, so C[n][m]: registers 4q .. 4q + 3 of a lane are four
// consecutive n of one m and leave as one 16-B store into the slab row m.
//
// LDS images.  Both operands are row-major [BK][W] fp32 copies of the BK x W
// block of g or x, the layout the matrices have in memory.  An operand
// fragment is ONE ds_read_b32 per lane: lanes 0..31 read 32 consecutive floats
// of image row k, lanes 32..63 the same 32 columns of row k + 1.  W is a
// multiple of 64 (the bank count), so unswizzled the two half-waves would
// meet on the same 32 banks.  Odd rows therefore hold their two 32-float
// halves of every 64-float group exchanged (column ^ 32, swz below): lanes
// 32..63 land on the other 32 banks and the 64 lanes of a read touch 64
// distinct banks.  No padding.  The 16-B staging stores keep their chunks
// whole (the swizzle moves bit 5 of the column); 16 consecutive lanes write
// the 16 chunks of one aligned 64-float group, in a permuted order: all 64
// banks once.  The 16-column image of the narrow geometry is not swizzled:
// its rows are 16 banks apart, so the half-waves read banks b .. b + 15 and
// b + 16 .. b + 31 (lanes 16..31 of each half repeat the addresses of lanes
// 0..15, a broadcast), and its 4-B staging stores are consecutive floats.
//
// K loop.  As in wgrad_splitk.hip: the global loads of the NEXT step go into
// registers before the MFMAs of the current one and into the other LDS
// buffer after them, one barrier per step.  Rows past the K-slice and columns
// past the matrix are staged as zeros, so the MFMA loop has no edge case and
// every lane is live in it.
//
// wgrad_gemv_f32: the M = 1 case (the logit layer) with its bias gradient,
// a streaming kernel without MFMA; described where it stands below.

#include <hip/hip_runtime.h>

#include "ops_api.h"

namespace {

constexpr int THREADS = 256;
constexpr int BK_F32 = 32;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// float offset of (row, col) in a [rows][W] image; W >= 64: odd rows hold the
// 32-float halves of each 64-float group exchanged
template <int W>
__device__ __forceinline__ int swz(int row, int col) {
  return row * W + (W >= 64 ? col ^ ((row & 1) << 5) : col);
}

// One operand's BK x W tile on its way global -> registers -> LDS.
// NARROW: rows of any length (no 16-B alignment), element by element.
template <int W, int BK, bool NARROW>
struct Stage {
  static constexpr int E = NARROW ? 1 : 4;  // floats per load
  static constexpr int C = W / E;           // loads per row
  static constexpr int TOTAL = BK * C;
  static constexpr int NL = (TOTAL + THREADS - 1) / THREADS;
  f32x4 v[NARROW ? 1 : NL];
  float s[NARROW ? NL : 1];

  // rows k0.. of src [K][ld], columns col0..; zeros for k >= kend, col >= ld
  __device__ __forceinline__ void load(const float* __restrict__ src,
                                       int64_t k0, int64_t kend, int col0,
                                       int ld) {
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int chunk = it * THREADS + threadIdx.x;
      const int64_t k = k0 + chunk / C;
      const int col = col0 + (chunk % C) * E;
      // ld % 4 == 0 unless NARROW: the whole chunk or none of it
      const bool in = chunk < TOTAL && k < kend && col < ld;
      if constexpr (NARROW) {
        s[it] = in ? src[k * ld + col] : 0.f;
      } else {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        v[it] = z;
        if (in) v[it] = *reinterpret_cast<const f32x4*>(src + k * ld + col);
      }
    }
  }

  __device__ __forceinline__ void store(float* img) const {
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int chunk = it * THREADS + threadIdx.x;
      if (chunk < TOTAL) {
        float* at = &img[swz<W>(chunk / C, (chunk % C) * E)];
        if constexpr (NARROW) {
          *at = s[it];
        } else {
          *reinterpret_cast<f32x4*>(at) = v[it];
        }
      }
    }
  }
};

// Waves as WAVES_M x WAVES_N (= 4), a wave owns WM x WN 32x32 tiles.  XW is
// the width of the x image: BN, or 16 for the narrow geometry, whose one MFMA
// column block reads every x column twice and drops rows n >= 16 of C.
template <int WAVES_M, int WAVES_N, int WM, int WN, int BK, bool NARROW_X>
__global__ __launch_bounds__(THREADS) void wgrad_splitk_f32_partial(
    const float* __restrict__ g, const float* __restrict__ x,
    float* __restrict__ slab, int64_t K, int M, int N, int Np, int64_t kslice,
    int tiles_n) {
  static_assert(WAVES_M * WAVES_N * 64 == THREADS, "4 waves");
  static_assert(BK % 2 == 0, "whole MFMA k-steps");
  static_assert(!NARROW_X || (WAVES_N == 1 && WN == 1), "one 16-column block");
  constexpr int BM = WAVES_M * WM * 32;
  constexpr int BN = WAVES_N * WN * 32;  // MFMA columns of the tile
  constexpr int XW = NARROW_X ? 16 : BN;
  constexpr int BUF = BK * (BM + XW);  // floats of one {g, x} buffer
  constexpr int NQ = NARROW_X ? 2 : 4;  // groups of 8 n of C that are kept
  extern __shared__ float lds_f32[];

  const int lane = threadIdx.x & 63;
  const int half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm0 = (wave / WAVES_N) * WM * 32;
  const int wn0 = (wave % WAVES_N) * WN * 32;
  const int m0 = (blockIdx.x / tiles_n) * BM;
  const int n0 = (blockIdx.x % tiles_n) * XW;
  const int64_t kbeg = (int64_t)blockIdx.y * kslice;
  int64_t kend = kbeg + kslice;
  if (kend > K) kend = K;
  const int nsteps = (int)((kend - kbeg + BK - 1) / BK);

  // the lane's float offset in image rows 0 / 1 (its k of the first MFMA)
  int aoff[WN], boff[WM];
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    aoff[j] = swz<XW>(half, (wn0 + j * 32 + (lane & 31)) & (XW - 1));
  }
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    boff[i] = swz<BM>(half, wm0 + i * 32 + (lane & 31));
  }

  f32x16 acc[WN][WM];
#pragma unroll
  for (int j = 0; j < WN; ++j) {
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;
    }
  }

  Stage<BM, BK, false> sg;
  Stage<XW, BK, NARROW_X> sx;
  sg.load(g, kbeg, kend, m0, M);
  sx.load(x, kbeg, kend, n0, N);
  sg.store(lds_f32);
  sx.store(lds_f32 + BK * BM);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const float* gimg = lds_f32 + (s & 1) * BUF;
    const float* ximg = gimg + BK * BM;
    const bool more = s + 1 < nsteps;  // the same for the whole workgroup
    if (more) {
      sg.load(g, kbeg + (int64_t)(s + 1) * BK, kend, m0, M);
      sx.load(x, kbeg + (int64_t)(s + 1) * BK, kend, n0, N);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[WN], b[WM];
#pragma unroll
      for (int j = 0; j < WN; ++j) a[j] = ximg[kk * XW + aoff[j]];
#pragma unroll
      for (int i = 0; i < WM; ++i) b[i] = gimg[kk * BM + boff[i]];
#pragma unroll
      for (int j = 0; j < WN; ++j) {
#pragma unroll
        for (int i = 0; i < WM; ++i) {
          acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[i],
                                                           acc[j][i], 0, 0, 0);
        }
      }
    }
    if (more) {
      float* nxt = lds_f32 + ((s + 1) & 1) * BUF;
      sg.store(nxt);
      sx.store(nxt + BK * BM);
    }
    __syncthreads();
  }

  // lane: m = tile column lane % 32, n = 8 q + 4 (lane / 32) + 0..3
  float* out = slab + (int64_t)blockIdx.y * M * Np;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int m = m0 + wm0 + i * 32 + (lane & 31);
#pragma unroll
    for (int j = 0; j < WN; ++j) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int n = n0 + wn0 + j * 32 + q * 8 + half * 4;
        // Np % 4 == 0: all four columns or none
        if (m < M && n < Np) {
          const f32x4 o = {acc[j][i][4 * q], acc[j][i][4 * q + 1],
                           acc[j][i][4 * q + 2], acc[j][i][4 * q + 3]};
          *reinterpret_cast<f32x4*>(&out[(int64_t)m * Np + n]) = o;
        }
      }
    }
  }
}

// gw[m][n] = sum_s slab[s][m][n].  Block = 64 groups of 4 columns x 4 slice
// lanes; slice lane l sums slabs l, l+4, ... in order, then
// ((p0 + p1) + p2) + p3.
constexpr int FIN_QUADS = 64;
constexpr int FIN_LANES = 4;

__global__ __launch_bounds__(FIN_QUADS* FIN_LANES) void wgrad_splitk_f32_finish(
    const float* __restrict__ slab, float* __restrict__ gw, int S, int M,
    int N, int Np) {
  __shared__ f32x4 part[FIN_LANES][FIN_QUADS];
  const int q = threadIdx.x % FIN_QUADS;
  const int l = threadIdx.x / FIN_QUADS;
  const int64_t total = (int64_t)M * (Np / 4);
  const int64_t quad = (int64_t)blockIdx.x * FIN_QUADS + q;
  const int64_t stride = (int64_t)M * Np;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (quad < total) {
#pragma unroll 4
    for (int r = l; r < S; r += FIN_LANES) {
      s += *reinterpret_cast<const f32x4*>(&slab[r * stride + quad * 4]);
    }
  }
  part[l][q] = s;
  __syncthreads();
  if (l == 0 && quad < total) {
    f32x4 t = part[0][q];
#pragma unroll
    for (int i = 1; i < FIN_LANES; ++i) t += part[i][q];
    const int64_t m = quad / (Np / 4);
    const int n = (int)(quad % (Np / 4)) * 4;
    float* dst = gw + m * N + n;
    if (N == Np) {
      *reinterpret_cast<f32x4*>(dst) = t;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (n + j < N) dst[j] = t[j];
      }
    }
  }
}

// tile geometries (BM x BN), all with BK = 32 (two double-buffered images of
// 128 x 128: 64 KB, the LDS of the bf16 kernel):
//   0: 128 x 128   a wave owns 64 x 64: 4 MFMAs per 4 LDS reads, 64 accumulators
//   1:  64 x  64   M <= 64 or N <= 64
//   2: 128 x  16   N <= 16 (x rows of any length, staged with 4-B loads)
constexpr int CFG_BM[3] = {128, 64, 128};
constexpr int CFG_BN[3] = {128, 64, 16};

template <int WAVES_M, int WAVES_N, int WM, int WN, bool NARROW_X>
void launch_partial(const void* g, const void* x, float* slab, int64_t K,
                    int M, int N, int Np, int64_t kslice, int splitk,
                    hipStream_t stream) {
  constexpr int BM = WAVES_M * WM * 32;
  constexpr int XW = NARROW_X ? 16 : WAVES_N * WN * 32;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + XW - 1) / XW;
  const size_t lds = (size_t)2 * BK_F32 * (BM + XW) * sizeof(float);
  hipLaunchKernelGGL(
      (wgrad_splitk_f32_partial<WAVES_M, WAVES_N, WM, WN, BK_F32, NARROW_X>),
      dim3(tiles_m * tiles_n, splitk), dim3(THREADS), lds, stream,
      (const float*)g, (const float*)x, slab, K, M, N, Np, kslice, tiles_n);
}

// ---------------------------------------------------------------------------
// wgrad_gemv_f32: the weight and bias gradient of a Linear with ONE output
// feature, gw[n] = sum_k g[k] x[k, n] and gb = sum_k g[k] for fp32 g [K] and
// x [K, N], N % 4 == 0.  The streaming design of wgrad_gemv_partial
// (wgrad_splitk.hip) with 4 fp32 columns per lane: block = GV_COLS x GV_ROWS
// threads, one 16-B load per lane and row, GV_UNROLL loads in flight,
// grid = (column tiles, row chunks).  Every block writes one fp32 row of
// slab [chunks][N + 1] with plain stores (column N: the chunk's sum of g,
// from the blocks of column tile 0); wgrad_gemv_f32_finish sums the rows in a
// fixed order.
// ---------------------------------------------------------------------------
constexpr int GV_COLS = 32;
constexpr int GV_ROWS = 8;
constexpr int GV_TILE_N = GV_COLS * 4;
constexpr int GV_UNROLL = 4;

// scalar fp32 arithmetic in the device pass, as in wgrad_gemv_partial
#if defined(__HIP_DEVICE_COMPILE__)
#define DE_NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define DE_NO_PACKED_FP32
#endif

DE_NO_PACKED_FP32 __global__ __launch_bounds__(GV_COLS* GV_ROWS) void wgrad_gemv_f32_partial(
    const float* __restrict__ g, const float* __restrict__ x,
    float* __restrict__ slab, int64_t K, int N, int64_t rows_per_chunk) {
  __shared__ float part[GV_ROWS][GV_TILE_N + 4];
  __shared__ float gpart[GV_ROWS];
  const int cl = threadIdx.x % GV_COLS;
  const int rl = threadIdx.x / GV_COLS;
  const int col = blockIdx.x * GV_TILE_N + cl * 4;  // N % 4 == 0: all 4 or none
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > K) r1 = K;

  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float gsum = 0.f;

  if (col < N) {
    for (int64_t r = r0 + rl; r < r1; r += GV_ROWS * GV_UNROLL) {
      f32x4 xv[GV_UNROLL];
      float gv[GV_UNROLL];
#pragma unroll
      for (int u = 0; u < GV_UNROLL; ++u) {
        const int64_t ru = r + u * GV_ROWS;
        if (ru < r1) {
          xv[u] = *reinterpret_cast<const f32x4*>(x + ru * N + col);
          gv[u] = g[ru];
        }
      }
#pragma unroll
      for (int u = 0; u < GV_UNROLL; ++u) {
        const int64_t ru = r + u * GV_ROWS;
        if (ru < r1) {
          gsum += gv[u];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] += gv[u] * xv[u][j];
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < 4; ++j) part[rl][cl * 4 + j] = acc[j];
  if (cl == 0) gpart[rl] = gsum;
  __syncthreads();
  float* out = slab + (int64_t)blockIdx.y * (N + 1);
  if (threadIdx.x < GV_TILE_N) {
    const int c = blockIdx.x * GV_TILE_N + threadIdx.x;
    if (c < N) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < GV_ROWS; ++i) s += part[i][threadIdx.x];
      out[c] = s;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < GV_ROWS; ++i) s += gpart[i];
    out[N] = s;
  }
}

// gw[n] = sum_r slab[r][n] for n < N, gb = sum_r slab[r][N].  Block = 32
// columns x 32 row groups; group i sums rows i, i+32, ... in order, then the
// 32 partial sums in order.
constexpr int GVF_COLS = 32;
constexpr int GVF_GROUPS = 32;

__global__ __launch_bounds__(GVF_COLS* GVF_GROUPS) void wgrad_gemv_f32_finish(
    const float* __restrict__ slab, float* __restrict__ gw,
    float* __restrict__ gb, int R, int N) {
  __shared__ float part[GVF_GROUPS][GVF_COLS + 1];
  const int c = threadIdx.x % GVF_COLS;
  const int grp = threadIdx.x / GVF_COLS;
  const int col = blockIdx.x * GVF_COLS + c;
  float s = 0.f;
  if (col <= N) {
#pragma unroll 4
    for (int r = grp; r < R; r += GVF_GROUPS) {
      s += slab[(int64_t)r * (N + 1) + col];
    }
  }
  part[grp][c] = s;
  __syncthreads();
  if (grp == 0 && col <= N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < GVF_GROUPS; ++i) t += part[i][c];
    if (col < N) {
      gw[col] = t;
    } else {
      gb[0] = t;
    }
  }
}

}  // namespace

bool wgrad_gemv_f32_plan(int64_t K, int64_t N, WgradGemvPlan* plan) {
  if (K < 1 || N < 4 || N % 4 != 0 || N >= (1 << 24)) return false;
  // a few thousand blocks at the flagship shape; slab <= 1024 rows
  const int64_t col_tiles = (N + GV_TILE_N - 1) / GV_TILE_N;
  int64_t r = 2048 / col_tiles;
  if (r > 1024) r = 1024;
  if (r < 1) r = 1;
  int64_t rpc = (K + r - 1) / r;
  constexpr int STEP = GV_ROWS * GV_UNROLL;
  rpc = (rpc + STEP - 1) / STEP * STEP;
  plan->rows_per_chunk = rpc;
  plan->num_chunks = (K + rpc - 1) / rpc;
  // Routing: measured ahead of the library's GEMM + column sum at N = 256
  // from K = 8192 to 65536 (17.8 against 164 us there, profiles/mlp_f32.md);
  // smaller batches were not measured and stay on the library.
  plan->use = K >= 8192;
  return true;
}

void launch_wgrad_gemv_f32(const void* g, const void* x, float* slab, void* gw,
                           void* gb, int64_t K, int N,
                           const WgradGemvPlan& plan, hipStream_t stream) {
  const int col_tiles = (N + GV_TILE_N - 1) / GV_TILE_N;
  hipLaunchKernelGGL(wgrad_gemv_f32_partial,
                     dim3(col_tiles, (unsigned)plan.num_chunks),
                     dim3(GV_COLS * GV_ROWS), 0, stream, (const float*)g,
                     (const float*)x, slab, K, N, plan.rows_per_chunk);
  hipLaunchKernelGGL(wgrad_gemv_f32_finish,
                     dim3((N + 1 + GVF_COLS - 1) / GVF_COLS),
                     dim3(GVF_COLS * GVF_GROUPS), 0, stream,
                     (const float*)slab, (float*)gw, (float*)gb,
                     (int)plan.num_chunks, N);
}

bool wgrad_splitk_f32_plan(int64_t K, int64_t M, int64_t N,
                           WgradSplitkPlan* plan) {
  return wgrad_splitk_f32_plan_with(K, M, N, 0, -1, plan);
}

bool wgrad_splitk_f32_plan_with(int64_t K, int64_t M, int64_t N,
                                int64_t splitk, int tile,
                                WgradSplitkPlan* plan) {
  if (K < 1 || M < 4 || M % 4 != 0 || N < 1 || M >= (1 << 24) ||
      N >= (1 << 24) || (N % 4 != 0 && N > 16)) {
    return false;
  }
  int cfg;
  if (N <= 16) {
    cfg = 2;
  } else if (M <= 64 || N <= 64) {
    cfg = 1;
  } else {
    cfg = 0;
  }
  if (tile >= 0) {
    // the 16-column tile for N <= 16 alone, and nothing else for narrow rows
    if (tile > 2 || (tile == 2) != (N <= 16)) return false;
    cfg = tile;
  }
  const int64_t np = (N + 3) / 4 * 4;
  const int64_t tiles = ((M + CFG_BM[cfg] - 1) / CFG_BM[cfg]) *
                        ((N + CFG_BN[cfg] - 1) / CFG_BN[cfg]);
  // two workgroups for each of the 256 CUs ...
  int64_t sk = 512 / tiles;
  const int64_t max_sk = (K + BK_F32 - 1) / BK_F32;
  if (sk > max_sk) sk = max_sk;
  if (sk < 1) sk = 1;
  // ... with the slab, written and read once, no larger than the operands
  // (fp32 operands: twice the bytes of the bf16 plan, so SPLITK is halved
  // one step later)
  const int64_t operand_bytes = K * (M + N) * 4;
  while (sk > 1 && 2 * sk * M * np * 4 > operand_bytes) sk /= 2;
  if (splitk > 0) sk = splitk < max_sk ? splitk : max_sk;
  int64_t kslice = (K + sk - 1) / sk;
  kslice = (kslice + BK_F32 - 1) / BK_F32 * BK_F32;
  sk = (K + kslice - 1) / kslice;  // no empty slice
  if (sk > 65535) return false;
  plan->cfg = cfg;
  plan->splitk = (int)sk;
  plan->kslice = kslice;
  plan->np = (int)np;
  // Routing, from tools/bench_mlp_f32.py (profiles/mlp_f32.md): outputs up to
  // 256 x 512 are 3.4 to 4.4 times ahead of the fp32 GEMM at K = 65536
  // (512 x 13, 128 x 256, 256 x 512); from 512 x 1024 on the library runs at
  // 140 TFLOP/s against 121 here and keeps the shape.  Nothing in between
  // was measured, so nothing in between is routed.
  plan->use = K >= 8192 && M * np <= 256 * 512;
  return true;
}

void launch_wgrad_splitk_f32(const void* g, const void* x, float* slab,
                             void* gw, int64_t K, int M, int N,
                             const WgradSplitkPlan& plan, hipStream_t stream) {
  const int np = plan.np;
  if (plan.cfg == 0) {
    launch_partial<2, 2, 2, 2, false>(g, x, slab, K, M, N, np, plan.kslice,
                                      plan.splitk, stream);
  } else if (plan.cfg == 1) {
    launch_partial<2, 2, 1, 1, false>(g, x, slab, K, M, N, np, plan.kslice,
                                      plan.splitk, stream);
  } else {
    launch_partial<4, 1, 1, 1, true>(g, x, slab, K, M, N, np, plan.kslice,
                                     plan.splitk, stream);
  }
  const int64_t quads = (int64_t)M * (np / 4);
  hipLaunchKernelGGL(wgrad_splitk_f32_finish,
                     dim3((unsigned)((quads + FIN_QUADS - 1) / FIN_QUADS)),
                     dim3(FIN_QUADS * FIN_LANES), 0, stream,
                     (const float*)slab, (float*)gw, plan.splitk, M, N, np);
}
