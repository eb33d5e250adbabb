// Input assembly for the low-rank cross interaction (gfx950).
//
// cross_concat_fwd: x0 [B, (P+1)*D] = [bottom | packed rows in perm order]
//   from bottom [B, D] and the packed embeddings, [P, B, D] feature-major or
//   [B, P, D] sample-major (strides sb, sp as in dot_interact.hip).
// cross_concat_bwd: the reverse split of x0's gradient.
// Both are 16-byte copies: a lane moves 8 adjacent bf16 of one feature.

#include <hip/hip_runtime.h>

#include "ops_api.h"

namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

constexpr int CC_THREADS = 256;
// rows of x0 per block iteration: keeps the index arithmetic in 32 bits
constexpr int CC_ROWS = 16;
constexpr int CC_MAX_BLOCKS = 2048;

// Element offset of the 8 columns that vector v of row b of x0 mirrors in
// bottom (feature 0) or packed; -1 for a perm entry outside [0, P).
__device__ __forceinline__ int64_t concat_src(unsigned v, int64_t b, int D8,
                                              int P, int D, int64_t sb,
                                              int64_t sp,
                                              const int* __restrict__ perm,
                                              bool* is_bottom) {
  const unsigned f = v / (unsigned)D8;
  const unsigned d = (v - f * (unsigned)D8) * 8u;
  *is_bottom = f == 0;
  if (f == 0) return b * D + d;
  const int p = perm[f - 1];
  if ((unsigned)p >= (unsigned)P) return -1;
  return (b * sb + (int64_t)p * sp) * D + d;
}

template <bool FWD>
__global__ __launch_bounds__(CC_THREADS) void cross_concat_kernel(
    unsigned short* __restrict__ bottom, unsigned short* __restrict__ packed,
    const int* __restrict__ perm, unsigned short* __restrict__ x0, int64_t B,
    int P, int D, int64_t sb, int64_t sp) {
  const int D8 = D / 8;
  const unsigned row_vecs = (unsigned)(P + 1) * (unsigned)D8;
  const int64_t tiles = (B + CC_ROWS - 1) / CC_ROWS;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t b0 = t * CC_ROWS;
    const unsigned rows = (unsigned)(B - b0 < CC_ROWS ? B - b0 : CC_ROWS);
    const unsigned n = rows * row_vecs;
    for (unsigned i = threadIdx.x; i < n; i += CC_THREADS) {
      const unsigned r = i / row_vecs;
      const unsigned v = i - r * row_vecs;
      const int64_t b = b0 + r;
      bool is_bottom;
      const int64_t src = concat_src(v, b, D8, P, D, sb, sp, perm, &is_bottom);
      unsigned short* xp = x0 + (b * row_vecs + v) * 8;
      if (FWD) {
        u16x8 val = {0, 0, 0, 0, 0, 0, 0, 0};
        if (src >= 0)
          val = *reinterpret_cast<const u16x8*>((is_bottom ? bottom : packed) + src);
        *reinterpret_cast<u16x8*>(xp) = val;
      } else if (src >= 0) {
        *reinterpret_cast<u16x8*>((is_bottom ? bottom : packed) + src) =
            *reinterpret_cast<const u16x8*>(xp);
      }
    }
  }
}

template <bool FWD>
void launch_concat(void* bottom, void* packed, const int* perm, void* x0,
                   int64_t B, int P, int D, int64_t sb, int64_t sp,
                   hipStream_t stream) {
  const int64_t tiles = (B + CC_ROWS - 1) / CC_ROWS;
  if (tiles == 0) return;
  const int grid = (int)(tiles < CC_MAX_BLOCKS ? tiles : CC_MAX_BLOCKS);
  hipLaunchKernelGGL(cross_concat_kernel<FWD>, dim3(grid), dim3(CC_THREADS), 0,
                     stream, (unsigned short*)bottom, (unsigned short*)packed,
                     perm, (unsigned short*)x0, B, P, D, sb, sp);
}

}  // namespace

void launch_cross_concat_fwd(const void* bottom, const void* packed,
                             const int* perm, void* x0, int64_t B, int P,
                             int D, int64_t sb, int64_t sp,
                             hipStream_t stream) {
  // the forward instance only reads bottom and packed
  launch_concat<true>(const_cast<void*>(bottom), const_cast<void*>(packed),
                      perm, x0, B, P, D, sb, sp, stream);
}

void launch_cross_concat_bwd(const void* gx0, const int* perm, void* gbottom,
                             void* gpacked, int64_t B, int P, int D,
                             int64_t sb, int64_t sp, hipStream_t stream) {
  // the backward instance only reads gx0
  launch_concat<false>(gbottom, gpacked, perm, const_cast<void*>(gx0), B, P,
                       D, sb, sp, stream);
}
