// Split-K weight gradient of a Linear layer (gfx950).
//
// wgrad_splitk: gw[M, N] = bf16( sum_k g[k, m] * x[k, n] ) for contiguous
// bf16 g [K, M] and x [K, N]: both operands are summed over their slow
// index, the output is small and K is the batch.
//
// Partial kernel.  grid = (output tiles, K-slices), 4 waves per workgroup.  A
// workgroup owns one BM x BN output tile and one K-slice; tiles are the fast
// grid index, so the tiles of one K-slice are dispatched together and the
// re-reads of g (once per column tile) and of x (once per row tile) meet in
// the caches.  Per step of BK rows it
//  - loads g[k0:k0+BK, m-tile] and x[k0:k0+BK, n-tile] of the NEXT step with
//    16-B global loads into registers (rows past the slice, columns past the
//    matrix: zeros),
//  - multiplies the CURRENT step out of LDS: both images are plain row-major
//    [BK][tile width] copies whose 16-B chunks are XORed with a function of
//    the row (swz below, the dot-interaction backward's image), and both
//    MFMA operands are read with ds_read_b64_tr_b16: the 16-lane group h of
//    a wave takes rows 8h..8h+3 and 8h+4..8h+7 of 16 columns, lane 4q+p of
//    the group supplies row q, columns 4p..4p+3.  Every lane is live: no
//    branch around the reads depends on the lane,
//  - writes the registers to the other LDS buffer; one barrier per step.
// The product is formed as (x fragment) x (g fragment), so a lane ends with
// 4 consecutive n of one m per 16x16 tile and the fp32 slab tile leaves as
// 16-B stores.  slab is [SPLITK][M][Np] fp32, Np = N rounded up to 4.
//
// Finish kernel.  Sums the SPLITK slabs in a fixed order (4 interleaved
// partial sums, combined in a fixed order) and rounds once to bf16.  No
// atomics, no hand-off between workgroups: two calls agree bit for bit.
//
// Rows of x that are no multiple of 16 B (the 13 numerical features) are
// staged element by element into a zero-padded 16-column tile (NARROW).

#include <hip/hip_runtime.h>

#include "ops_api.h"

namespace {

constexpr int THREADS = 256;

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef short v4i16_t __attribute__((vector_size(8)));
typedef __attribute__((address_space(3))) v4i16_t lds_v4i16_t;

// round-to-nearest-even, NaN -> 0x7FC0: torch's fp32 -> bf16 conversion
__device__ __forceinline__ unsigned short f32_to_bf16_rne(float f) {
  unsigned int u = __float_as_uint(f);
  if (f != f) return 0x7FC0;
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

// element offset of (row, col) in a [rows][W] image with swizzled chunks
template <int W>
__device__ __forceinline__ int swz(int row, int col) {
  const int sw = (((row & 3) << 2) | ((row >> 2) & 3)) & (W / 8 - 1);
  return row * W + ((((col >> 3) ^ sw) << 3) | (col & 7));
}

// One operand's BK x W tile on its way global -> registers -> LDS.
template <int W, int BK, bool NARROW>
struct Stage {
  static constexpr int C = W / 8;  // 16-B chunks per row
  static constexpr int TOTAL = BK * C;
  static constexpr int NL = (TOTAL + THREADS - 1) / THREADS;
  bf16x8 v[NL];

  // rows k0.. of src [K][ld], columns col0..; zeros for k >= kend, col >= ld
  __device__ __forceinline__ void load(const short* __restrict__ src,
                                       int64_t k0, int64_t kend, int col0,
                                       int ld) {
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int chunk = it * THREADS + threadIdx.x;
      const int64_t k = k0 + chunk / C;
      const int col = col0 + (chunk % C) * 8;
      const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      v[it] = z;
      if (chunk < TOTAL && k < kend) {
        if (!NARROW) {
          // ld % 8 == 0: the whole chunk or none of it
          if (col < ld) {
            v[it] = *reinterpret_cast<const bf16x8*>(src + k * ld + col);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (col + j < ld) v[it][j] = src[k * ld + col + j];
          }
        }
      }
    }
  }

  __device__ __forceinline__ void store(short* img) const {
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int chunk = it * THREADS + threadIdx.x;
      if (chunk < TOTAL) {
        *reinterpret_cast<bf16x8*>(&img[swz<W>(chunk / C, (chunk % C) * 8)]) =
            v[it];
      }
    }
  }
};

// the 16x16x32 operand whose 16 rows/columns are columns c0..c0+15 of the
// image and whose 32 k are image rows r0..r0+31
template <int W>
__device__ __forceinline__ bf16x8 tr_fragment(const short* img, int r0, int c0,
                                              int lane) {
  const int row = r0 + (lane >> 4) * 8 + ((lane & 15) >> 2);
  const int col = c0 + (lane & 3) * 4;
  const v4i16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_v4i16_t*)(img + swz<W>(row, col)));
  const v4i16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_v4i16_t*)(img + swz<W>(row + 4, col)));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// Waves as WAVES_M x WAVES_N (= 4), a wave owns WM x WN 16x16 tiles.
template <int WAVES_M, int WAVES_N, int WM, int WN, int BK, bool NARROW_X>
__global__ __launch_bounds__(THREADS) void wgrad_splitk_partial(
    const short* __restrict__ g, const short* __restrict__ x,
    float* __restrict__ slab, int64_t K, int M, int N, int Np, int64_t kslice,
    int tiles_n) {
  static_assert(WAVES_M * WAVES_N * 64 == THREADS, "4 waves");
  static_assert(BK % 32 == 0, "whole MFMA k-steps");
  constexpr int BM = WAVES_M * WM * 16;
  constexpr int BN = WAVES_N * WN * 16;
  constexpr int BUF = BK * (BM + BN);  // elements of one {g, x} buffer
  extern __shared__ short lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm0 = (wave / WAVES_N) * WM * 16;
  const int wn0 = (wave % WAVES_N) * WN * 16;
  const int m0 = (blockIdx.x / tiles_n) * BM;
  const int n0 = (blockIdx.x % tiles_n) * BN;
  const int64_t kbeg = (int64_t)blockIdx.y * kslice;
  int64_t kend = kbeg + kslice;
  if (kend > K) kend = K;
  const int nsteps = (int)((kend - kbeg + BK - 1) / BK);

  f32x4 acc[WN][WM];
#pragma unroll
  for (int j = 0; j < WN; ++j) {
#pragma unroll
    for (int i = 0; i < WM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  Stage<BM, BK, false> sg;
  Stage<BN, BK, NARROW_X> sx;
  sg.load(g, kbeg, kend, m0, M);
  sx.load(x, kbeg, kend, n0, N);
  sg.store(lds);
  sx.store(lds + BK * BM);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const short* gimg = lds + (s & 1) * BUF;
    const short* ximg = gimg + BK * BM;
    const bool more = s + 1 < nsteps;  // the same for the whole workgroup
    if (more) {
      sg.load(g, kbeg + (int64_t)(s + 1) * BK, kend, m0, M);
      sx.load(x, kbeg + (int64_t)(s + 1) * BK, kend, n0, N);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 32) {
      bf16x8 a[WM], b[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        a[i] = tr_fragment<BM>(gimg, kk, wm0 + i * 16, lane);
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        b[j] = tr_fragment<BN>(ximg, kk, wn0 + j * 16, lane);
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
#pragma unroll
        for (int i = 0; i < WM; ++i) {
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i],
                                                              acc[j][i], 0, 0, 0);
        }
      }
    }
    if (more) {
      short* nxt = lds + ((s + 1) & 1) * BUF;
      sg.store(nxt);
      sx.store(nxt + BK * BM);
    }
    __syncthreads();
  }

  // lane: m = tile row (lane & 15), n = 4 * (lane >> 4) + 0..3
  float* out = slab + (int64_t)blockIdx.y * M * Np;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int m = m0 + wm0 + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = n0 + wn0 + j * 16 + 4 * (lane >> 4);
      // Np % 4 == 0: all four columns or none
      if (m < M && n < Np) {
        *reinterpret_cast<f32x4*>(&out[(int64_t)m * Np + n]) = acc[j][i];
      }
    }
  }
}

// gw[m][n] = bf16(sum_s slab[s][m][n]).  Block = 64 groups of 4 columns x 4
// slice lanes; slice lane l sums slabs l, l+4, ... in order, then
// ((p0 + p1) + p2) + p3.
constexpr int FIN_QUADS = 64;
constexpr int FIN_LANES = 4;

__global__ __launch_bounds__(FIN_QUADS* FIN_LANES) void wgrad_splitk_finish(
    const float* __restrict__ slab, unsigned short* __restrict__ gw, int S,
    int M, int N, int Np) {
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
    unsigned short* dst = gw + m * N + n;
    if (N == Np) {
      typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
      const u16x4 o = {f32_to_bf16_rne(t[0]), f32_to_bf16_rne(t[1]),
                       f32_to_bf16_rne(t[2]), f32_to_bf16_rne(t[3])};
      *reinterpret_cast<u16x4*>(dst) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (n + j < N) dst[j] = f32_to_bf16_rne(t[j]);
      }
    }
  }
}

// tile geometries (BM x BN), all with BK = 64:
//   0: 128 x 128   16 MFMAs per 16 transposed reads and wave
//   1:  64 x  64   M <= 64 or N <= 64
//   2: 128 x  16   N <= 16 (x rows of any length when N % 8 != 0)
constexpr int BK_ALL = 64;
constexpr int CFG_BM[3] = {128, 64, 128};
constexpr int CFG_BN[3] = {128, 64, 16};

template <int WAVES_M, int WAVES_N, int WM, int WN, bool NARROW_X>
void launch_partial(const void* g, const void* x, float* slab, int64_t K,
                    int M, int N, int Np, int64_t kslice, int splitk,
                    hipStream_t stream) {
  constexpr int BM = WAVES_M * WM * 16, BN = WAVES_N * WN * 16;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const size_t lds = (size_t)2 * BK_ALL * (BM + BN) * sizeof(short);
  hipLaunchKernelGGL(
      (wgrad_splitk_partial<WAVES_M, WAVES_N, WM, WN, BK_ALL, NARROW_X>),
      dim3(tiles_m * tiles_n, splitk), dim3(THREADS), lds, stream,
      (const short*)g, (const short*)x, slab, K, M, N, Np, kslice, tiles_n);
}

}  // namespace

bool wgrad_splitk_plan(int64_t K, int64_t M, int64_t N, WgradSplitkPlan* plan) {
  return wgrad_splitk_plan_with(K, M, N, 0, -1, plan);
}

bool wgrad_splitk_plan_with(int64_t K, int64_t M, int64_t N, int64_t splitk,
                            int tile, WgradSplitkPlan* plan) {
  if (K < 1 || M < 8 || M % 8 != 0 || N < 1 || M >= (1 << 24) ||
      N >= (1 << 24) || (N % 8 != 0 && N > 16)) {
    return false;
  }
  int cfg;
  if (N <= 16) {
    cfg = 2;
  } else if (M <= 64 || N <= 64) {
    cfg = 1;
  } else {
    // also for 128 x 256, where it is two tiles: measured ahead of 64 x 64
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
  // two workgroups for each of the 256 CUs (measured: ahead of one at every
  // flagship shape) ...
  int64_t sk = 512 / tiles;
  const int64_t max_sk = (K + BK_ALL - 1) / BK_ALL;
  if (sk > max_sk) sk = max_sk;
  if (sk < 1) sk = 1;
  // ... with the slab, written and read once, no larger than the operands
  const int64_t operand_bytes = K * (M + N) * 2;
  while (sk > 1 && 2 * sk * M * np * 4 > operand_bytes) sk /= 2;
  if (splitk > 0) sk = splitk < max_sk ? splitk : max_sk;
  int64_t kslice = (K + sk - 1) / sk;
  kslice = (kslice + BK_ALL - 1) / BK_ALL * BK_ALL;
  sk = (K + kslice - 1) / kslice;  // no empty slice
  if (sk > 65535) return false;
  plan->cfg = cfg;
  plan->splitk = (int)sk;
  plan->kslice = kslice;
  plan->np = (int)np;
  // Routing: the kind of shape at which the split-K kernels beat the tuned
  // GEMM in tools/bench_wgrad.py (profiles/wgrad_splitk.md: all seven
  // flagship layers, SPLITK 8 to 128 at K = 65536).  A small K, or an output
  // so large that there is little to split, stays on the GEMM library.
  plan->use = K >= 4096 && sk >= 8;
  return true;
}

void launch_wgrad_splitk(const void* g, const void* x, float* slab, void* gw,
                         int64_t K, int M, int N, const WgradSplitkPlan& plan,
                         hipStream_t stream) {
  const int np = plan.np;
  if (plan.cfg == 0) {
    launch_partial<2, 2, 4, 4, false>(g, x, slab, K, M, N, np, plan.kslice,
                                      plan.splitk, stream);
  } else if (plan.cfg == 1) {
    launch_partial<2, 2, 2, 2, false>(g, x, slab, K, M, N, np, plan.kslice,
                                      plan.splitk, stream);
  } else if (N % 8 == 0) {
    launch_partial<4, 1, 2, 1, false>(g, x, slab, K, M, N, np, plan.kslice,
                                      plan.splitk, stream);
  } else {
    launch_partial<4, 1, 2, 1, true>(g, x, slab, K, M, N, np, plan.kslice,
                                     plan.splitk, stream);
  }
  const int64_t quads = (int64_t)M * (np / 4);
  hipLaunchKernelGGL(wgrad_splitk_finish,
                     dim3((unsigned)((quads + FIN_QUADS - 1) / FIN_QUADS)),
                     dim3(FIN_QUADS * FIN_LANES), 0, stream,
                     (const float*)slab, (unsigned short*)gw, plan.splitk, M,
                     N, np);
}
