// Elementwise work around the Linear+ReLU stacks (gfx950).
//
// relu_bwd_bias_grad: grad_in = (y <= 0) ? 0 : grad_out  (torch's
//   threshold_backward, bit for bit) and bias_grad[n] = bf16(sum_b grad_in)
//   from ONE pass over grad_out and y.  Deterministic: every block sums its
//   row chunk in a fixed order and writes one fp32 row of a slab [R, N] with
//   plain stores; a second tiny kernel sums the R rows in a fixed order.
//
// cross_bwd: the elementwise backward of a low-rank cross layer (DCN-v2),
//   gu = G * x0, its column sum (the bias gradient) and acc (+)= G * u from
//   one pass, on the same tiling, slab and finish kernel.

#include <hip/hip_runtime.h>

#include "ops_api.h"

namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short h) {
  return __uint_as_float((unsigned int)h << 16);
}

// round-to-nearest-even, NaN -> 0x7FC0: torch's fp32 -> bf16 conversion
__device__ __forceinline__ unsigned short f32_to_bf16_rne(float f) {
  unsigned int u = __float_as_uint(f);
  if (f != f) return 0x7FC0;
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

// ---------------------------------------------------------------------------
// relu_bwd_bias_grad, pass 1.
// Block = COL_LANES x ROW_LANES threads; a lane owns 8 adjacent columns (one
// 16-byte load/store per row), so a block covers a tile of COL_LANES*8 = 128
// columns and walks its row chunk ROW_LANES rows at a time.
// grid = (column tiles, row chunks).
// ---------------------------------------------------------------------------
constexpr int COL_LANES = 16;
constexpr int ROW_LANES = 16;
constexpr int TILE_N = COL_LANES * 8;
constexpr int ROW_UNROLL = 4;

__global__ __launch_bounds__(COL_LANES* ROW_LANES) void relu_bwd_bias_partial(
    const unsigned short* __restrict__ gout, const unsigned short* __restrict__ y,
    unsigned short* __restrict__ gin, float* __restrict__ slab, int64_t B,
    int N, int64_t rows_per_chunk) {
  __shared__ float part[ROW_LANES][TILE_N + 4];
  const int cl = threadIdx.x % COL_LANES;
  const int rl = threadIdx.x / COL_LANES;
  const int col = blockIdx.x * TILE_N + cl * 8;  // N % 8 == 0: all 8 or none
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > B) r1 = B;

  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;

  if (col < N) {
    for (int64_t r = r0 + rl; r < r1; r += ROW_LANES * ROW_UNROLL) {
      u16x8 g[ROW_UNROLL], a[ROW_UNROLL];
#pragma unroll
      for (int u = 0; u < ROW_UNROLL; ++u) {
        const int64_t ru = r + u * ROW_LANES;
        if (ru < r1) {
          const int64_t off = ru * N + col;
          g[u] = *reinterpret_cast<const u16x8*>(gout + off);
          a[u] = *reinterpret_cast<const u16x8*>(y + off);
        }
      }
#pragma unroll
      for (int u = 0; u < ROW_UNROLL; ++u) {
        const int64_t ru = r + u * ROW_LANES;
        if (ru < r1) {
          u16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            // NaN in y compares false: the gradient passes, as in torch
            const bool blocked = bf16_bits_to_f32(a[u][j]) <= 0.f;
            o[j] = blocked ? (unsigned short)0 : g[u][j];
            acc[j] += bf16_bits_to_f32(o[j]);
          }
          *reinterpret_cast<u16x8*>(gin + ru * N + col) = o;
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < 8; ++j) part[rl][cl * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < TILE_N) {
    const int c = blockIdx.x * TILE_N + threadIdx.x;
    if (c < N) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < ROW_LANES; ++i) s += part[i][threadIdx.x];
      slab[(int64_t)blockIdx.y * N + c] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// cross_bwd, pass 1: the elementwise backward of one low-rank cross layer
// x_{l+1} = x0 * u + x_l.  Same tiling and slab as relu_bwd_bias_partial.
//   gu  = bf16(G * x0)                      (exact fp32 product, one rounding)
//   acc = bf16((INIT ? 0 : acc) + G * u)    (fp32, one rounding; in place)
//   slab[chunk][n] = sum over the chunk's rows of fp32(gu)
// INIT never reads acc, so acc may hold anything (NaN included) beforehand.
// acc is read and written by the same lane at the same address only.
// ---------------------------------------------------------------------------
constexpr int CROSS_UNROLL = 2;

template <bool INIT>
__global__ __launch_bounds__(COL_LANES* ROW_LANES) void cross_bwd_partial(
    const unsigned short* __restrict__ gout, const unsigned short* __restrict__ x0,
    const unsigned short* __restrict__ u, unsigned short* acc,
    unsigned short* __restrict__ gu, float* __restrict__ slab, int64_t B, int N,
    int64_t rows_per_chunk) {
  __shared__ float part[ROW_LANES][TILE_N + 4];
  const int cl = threadIdx.x % COL_LANES;
  const int rl = threadIdx.x / COL_LANES;
  const int col = blockIdx.x * TILE_N + cl * 8;  // N % 8 == 0: all 8 or none
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > B) r1 = B;

  float sum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) sum[j] = 0.f;

  if (col < N) {
    for (int64_t r = r0 + rl; r < r1; r += ROW_LANES * CROSS_UNROLL) {
      u16x8 g[CROSS_UNROLL], x[CROSS_UNROLL], w[CROSS_UNROLL], a[CROSS_UNROLL];
#pragma unroll
      for (int k = 0; k < CROSS_UNROLL; ++k) {
        const int64_t rk = r + k * ROW_LANES;
        if (rk < r1) {
          const int64_t off = rk * N + col;
          g[k] = *reinterpret_cast<const u16x8*>(gout + off);
          x[k] = *reinterpret_cast<const u16x8*>(x0 + off);
          w[k] = *reinterpret_cast<const u16x8*>(u + off);
          if (!INIT) a[k] = *reinterpret_cast<const u16x8*>(acc + off);
        }
      }
#pragma unroll
      for (int k = 0; k < CROSS_UNROLL; ++k) {
        const int64_t rk = r + k * ROW_LANES;
        if (rk < r1) {
          u16x8 o, s;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float gf = bf16_bits_to_f32(g[k][j]);
            o[j] = f32_to_bf16_rne(gf * bf16_bits_to_f32(x[k][j]));
            sum[j] += bf16_bits_to_f32(o[j]);
            // the product is exact in fp32, so a contracted fma changes nothing
            // under INIT and rounds once instead of twice otherwise
            const float gw = gf * bf16_bits_to_f32(w[k][j]);
            s[j] = f32_to_bf16_rne(INIT ? gw : bf16_bits_to_f32(a[k][j]) + gw);
          }
          const int64_t off = rk * N + col;
          *reinterpret_cast<u16x8*>(gu + off) = o;
          *reinterpret_cast<u16x8*>(acc + off) = s;
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < 8; ++j) part[rl][cl * 8 + j] = sum[j];
  __syncthreads();
  if (threadIdx.x < TILE_N) {
    const int c = blockIdx.x * TILE_N + threadIdx.x;
    if (c < N) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < ROW_LANES; ++i) s += part[i][threadIdx.x];
      slab[(int64_t)blockIdx.y * N + c] = s;
    }
  }
}

// pass 2: bias_grad[n] = bf16(sum_r slab[r][n]), fixed order.
// Block = 32 columns x 32 row groups; group g sums rows g, g+32, ...
constexpr int FIN_COLS = 32;
constexpr int FIN_GROUPS = 32;

__global__ __launch_bounds__(FIN_COLS* FIN_GROUPS) void bias_grad_finish(
    const float* __restrict__ slab, unsigned short* __restrict__ bias_grad,
    int R, int N) {
  __shared__ float part[FIN_GROUPS][FIN_COLS + 1];
  const int c = threadIdx.x % FIN_COLS;
  const int g = threadIdx.x / FIN_COLS;
  const int col = blockIdx.x * FIN_COLS + c;
  float s = 0.f;
  if (col < N) {
#pragma unroll 4
    for (int r = g; r < R; r += FIN_GROUPS) s += slab[(int64_t)r * N + col];
  }
  part[g][c] = s;
  __syncthreads();
  if (g == 0 && col < N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < FIN_GROUPS; ++i) t += part[i][c];
    bias_grad[col] = f32_to_bf16_rne(t);
  }
}

}  // namespace

void relu_bwd_bias_grad_plan(int64_t B, int N, int64_t* rows_per_chunk,
                             int64_t* num_chunks) {
  // a few thousand blocks at the flagship shapes; slab <= 1024 rows
  const int64_t col_tiles = (N + TILE_N - 1) / TILE_N;
  int64_t r = 2048 / col_tiles;
  if (r > 1024) r = 1024;
  if (r < 1) r = 1;
  int64_t rpc = (B + r - 1) / r;
  rpc = (rpc + ROW_LANES - 1) / ROW_LANES * ROW_LANES;
  *rows_per_chunk = rpc;
  *num_chunks = (B + rpc - 1) / rpc;
}

void launch_relu_bwd_bias_grad(const void* grad_out, const void* y,
                               void* grad_in, float* slab, void* bias_grad,
                               int64_t B, int N, int64_t rows_per_chunk,
                               int64_t num_chunks, hipStream_t stream) {
  const int col_tiles = (N + TILE_N - 1) / TILE_N;
  dim3 grid(col_tiles, (unsigned)num_chunks);
  hipLaunchKernelGGL(relu_bwd_bias_partial, grid,
                     dim3(COL_LANES * ROW_LANES), 0, stream,
                     (const unsigned short*)grad_out,
                     (const unsigned short*)y, (unsigned short*)grad_in, slab,
                     B, N, rows_per_chunk);
  hipLaunchKernelGGL(bias_grad_finish, dim3((N + FIN_COLS - 1) / FIN_COLS),
                     dim3(FIN_COLS * FIN_GROUPS), 0, stream,
                     (const float*)slab, (unsigned short*)bias_grad,
                     (int)num_chunks, N);
}

void launch_cross_bwd(const void* gout, const void* x0, const void* u,
                      void* acc, bool init, void* gu, float* slab,
                      void* bias_grad, int64_t B, int N,
                      int64_t rows_per_chunk, int64_t num_chunks,
                      hipStream_t stream) {
  const int col_tiles = (N + TILE_N - 1) / TILE_N;
  dim3 grid(col_tiles, (unsigned)num_chunks);
  auto kernel = init ? cross_bwd_partial<true> : cross_bwd_partial<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(COL_LANES * ROW_LANES), 0, stream,
                     (const unsigned short*)gout, (const unsigned short*)x0,
                     (const unsigned short*)u, (unsigned short*)acc,
                     (unsigned short*)gu, slab, B, N, rows_per_chunk);
  hipLaunchKernelGGL(bias_grad_finish, dim3((N + FIN_COLS - 1) / FIN_COLS),
                     dim3(FIN_COLS * FIN_GROUPS), 0, stream,
                     (const float*)slab, (unsigned short*)bias_grad,
                     (int)num_chunks, N);
}
