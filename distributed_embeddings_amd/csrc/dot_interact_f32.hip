// Fused DLRM pairwise-dot interaction on fp32 inputs for gfx950 (fp32 MFMA).
//
// Same semantics as dot_interact.hip, fp32 in, fp32 accumulation, fp32 out:
// forward:  feats [B, F, D] -> out [B, out_w]
//           = [strictly-lower tril(feats feats^T) | feats[:, 0] | zeros]
// backward: gfeats = (G + G^T) feats, + gout[:, tri_n : tri_n + D] on feature 0
// for 1 <= F <= 32, D % 8 == 0, 8 <= D <= 256, with v_mfma_f32_32x32x2_f32:
//   A: lane l supplies row l % 32,    k = l / 32
//   B: lane l supplies column l % 32, k = l / 32
//   C: register r of lane l is row 8 * (r / 4) + 4 * (l / 32) + r % 4,
//      column l % 32
// One wave per sample; the waves of a block share nothing (no block barrier).
//
// Layouts, as for the narrow bf16 kernels: feature 0 is bottom + b * bstride,
// feature f >= 1 is packed + (perm[f - 1] * sp + b * sb) * D.  Stacked
// [B, F, D] is bottom = packed = feats, bstride = F * D, sb = F, sp = 1 and no
// perm (row f).  A perm entry outside [0, P) makes its feature a row of zeros
// whose gradient is not written: no address is formed from it.
//
// Data movement.  The sample is a [32][D / 4] grid of 16-B chunks, chunk
// i = lane + 64 * it: consecutive lanes take consecutive chunks of a row, so
// one load instruction covers 64 / (D / 4) whole rows (two at D = 128).  All
// chunks of a sample are loaded into registers, then written to a per-wave
// LDS image [32][D + 4] floats with rows >= F zero; the loads of the wave's
// next sample are issued right after that, ahead of the MFMAs of this one.
//
// Bank mapping of the image (64 banks of 4 B; LD = D + 4, D % 8 == 0, so
// LD / 4 is odd):
//  - forward operand: lane l reads 16 B at row l % 32, floats 8 s + 4 (l / 32)
//    .. + 3.  A 16-B access is served 16 lanes at a time; lanes 16 g .. + 15
//    read 16 consecutive rows of one column chunk, and row r starts on
//    16-B bank group r * (LD / 4) mod 16: LD / 4 odd makes the 16 distinct.
//  - backward operand: lane l reads 4 B at row k, float d0 + l % 32, with
//    k = k0 for lanes < 32 and k0 + 8 for the rest (see the k partition
//    below).  8 * LD = 8 D + 32 = 32 mod 64, so the halves sit on banks
//    c .. c + 31 and c + 32 .. c + 63: 64 distinct banks.
//
// Forward.  X X^T has A = B: the lane's 16-B read feeds four MFMAs, component
// c being columns 8 s + c (lanes < 32) and 8 s + 4 + c (the rest) - any
// partition of the D columns over (step, lane half) is a valid sum.  D / 2
// MFMAs and D / 8 LDS reads per sample; the upper triangle is computed and
// dropped.  The strictly-lower accumulators go into a per-wave image of the
// tril part, and the row [tril | bottom from image row 0 | zeros] leaves as
// 4-B stores of consecutive lanes (the row start is only 4-B aligned).
//
// Backward.  gfeats[i][d] = sum_k Gs[i][k] X[k][d], A = Gs, B = X, per tile of
// 32 columns d.  Which k goes to which (step, lane half) is free as well:
// step s takes k0 = 16 (s / 8) + s % 8 in lanes < 32 and k0 + 8 in the rest.
// The 16 A values of a lane are gathered once per sample from the staged gout
// row; a step whose k0 >= F is skipped on a scalar branch.  The bottom-concat
// gradient is register 0 of lanes < 32 of the C operand (row 0).  Register r
// is 32 consecutive floats of one feature row per lane half, stored straight
// to gbottom / gpacked.  A last partial tile (D % 32 != 0) has zero operands
// in the lanes beyond D, and those lanes store nothing.
//
// EXEC is all ones at every MFMA: the branches around them are on F, D and
// the wave's sample index.  No float atomics; one fixed summation order.

#include <hip/hip_runtime.h>

#include <stdexcept>

#include "ops_api.h"

#define WAVE 64
#define DIF_WPB_MAX 4       // waves per block at most
#define DIF_LDS_MAX 65536   // bytes per block at most
#define DIF_GRID_MAX 8192   // blocks, a stride beyond
#define DIF_STAGE 512       // floats: the tril part, <= 496

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef f32x4 __attribute__((aligned(4))) f32x4_u;  // out / gout rows

// LDS writes of one lane read back by another lane of the same wave
__device__ __forceinline__ void dif_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The lane's chunks of the [32][D / 4] grid: where each lies in memory (at
// sample 0) and in the image.  DC is the width class (NIT = DC / 8 chunk
// slots per lane); slots past the grid (D < DC) are neither loaded nor written.
template <int DC>
struct F32Chunks {
  static constexpr int NIT = DC / 8;
  int64_t off[NIT];  // element offset in bottom (row 0) or packed
  int at[NIT];       // float offset in the image
  unsigned in;       // slot it is inside the grid
  unsigned ok;       // ... and a row < F that perm places inside packed
  unsigned first;    // ... and row 0

  __device__ __forceinline__ F32Chunks(const int* __restrict__ perm, int lane,
                                       int F, int D, int64_t sp) {
    const int D4 = D >> 2, LD = D + 4;
    in = ok = first = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = lane + WAVE * it;
      const int row = i / D4, col = (i - row * D4) * 4;
      at[it] = row * LD + col;
      off[it] = col;
      if (row < 32) in |= 1u << it;
      if (row == 0) first |= 1u << it;
      int p = row;
      bool good = row < F;
      if (perm != nullptr && row >= 1 && row < F) {
        p = perm[row - 1];
        good = (unsigned)p < (unsigned)(F - 1);
      }
      if (good) ok |= 1u << it;
      if (good && row >= 1) off[it] = (int64_t)p * sp * D + col;
    }
  }

  // all of sample b's chunks, zeros where there is nothing to load
  __device__ __forceinline__ void load(f32x4 (&v)[NIT], const float* bb,
                                       const float* pb) const {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      v[it] = z;
      if ((ok >> it) & 1) {
        v[it] = *reinterpret_cast<const f32x4*>(
            (((first >> it) & 1) ? bb : pb) + off[it]);
      }
    }
  }

  __device__ __forceinline__ void to_image(const f32x4 (&v)[NIT],
                                           float* img) const {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if ((in >> it) & 1) *reinterpret_cast<f32x4*>(&img[at[it]]) = v[it];
    }
  }
};

// DFIX != 0: the width is the compile-time DFIX (= DC); else D <= DC at run time
template <int DC, int DFIX>
__global__ __launch_bounds__(DIF_WPB_MAX* WAVE) void dot_interact_f32_fwd(
    const float* __restrict__ bottom, const float* __restrict__ packed,
    const int* __restrict__ perm, float* __restrict__ out, int64_t B, int F,
    int Drt, int out_w, int tri_n, int64_t bstride, int64_t sb, int64_t sp) {
  extern __shared__ __attribute__((aligned(16))) float dif_lds[];
  using IO = F32Chunks<DC>;
  const int D = DFIX ? DFIX : Drt;
  const int LD = D + 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (WAVE - 1);
  float* img = dif_lds + wave * (32 * LD + DIF_STAGE);
  float* stage = img + 32 * LD;
  const int f = lane & 31, h = lane >> 5;
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= B) return;  // wave-uniform; no block barrier below
  const IO io(perm, lane, F, D, sp);
  const int64_t sbd = sb * D;

  f32x4 v[IO::NIT];
  io.load(v, bottom + b * bstride, packed + b * sbd);
  for (; b < B; b += n_waves) {
    io.to_image(v, img);
    dif_lds_fence();
    const int64_t bn = b + n_waves;
    if (bn < B) io.load(v, bottom + bn * bstride, packed + bn * sbd);

    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                  0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* xr = img + f * LD + h * 4;
    for (int s = 0; s < D / 8; ++s) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(xr + 8 * s);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[c], x[c], acc, 0, 0, 0);
      }
    }
    // strictly-lower elements of column f, 16 rows
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 8 * (r >> 2) + 4 * h + (r & 3);
      if (i > f && i < F) stage[i * (i - 1) / 2 + f] = acc[r];
    }
    dif_lds_fence();
    float* orow = out + b * (int64_t)out_w;
    const int width = tri_n + D;
    for (int c = lane; c < out_w; c += WAVE) {
      float o = 0.f;
      if (c < tri_n) {
        o = stage[c];
      } else if (c < width) {
        o = img[c - tri_n];  // bottom: image row 0, bit for bit
      }
      orow[c] = o;
    }
    dif_lds_fence();  // the next sample overwrites the images
  }
}

template <int DC, int DFIX>
__global__ __launch_bounds__(DIF_WPB_MAX* WAVE, DC > 128 ? 1 : 2) void
dot_interact_f32_bwd(
    const float* __restrict__ gout, const float* __restrict__ bottom,
    const float* __restrict__ packed, const int* __restrict__ perm,
    float* gbottom, float* gpacked, int64_t B, int F, int Drt, int out_w,
    int tri_n, int64_t bstride, int64_t sb, int64_t sp) {
  extern __shared__ __attribute__((aligned(16))) float dif_lds[];
  using IO = F32Chunks<DC>;
  const int D = DFIX ? DFIX : Drt;
  const int LD = D + 4, D4 = D >> 2;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (WAVE - 1);
  // per wave: the image, the tril part of the gout row, its bottom part
  float* img = dif_lds + wave * (32 * LD + DIF_STAGE + D);
  float* stage = img + 32 * LD;
  float* gb = stage + DIF_STAGE;
  const int f = lane & 31, h = lane >> 5;
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= B) return;  // wave-uniform; no block barrier below
  const IO io(perm, lane, F, D, sp);
  const int64_t sbd = sb * D;

  // the 16 result rows of the lane: where their gradient goes
  int64_t goff[16];
  unsigned gok = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = 8 * (r >> 2) + 4 * h + (r & 3);
    int p = i;
    bool good = i < F;
    if (perm != nullptr && i >= 1 && i < F) {
      p = perm[i - 1];
      good = (unsigned)p < (unsigned)(F - 1);
    }
    goff[r] = good && i >= 1 ? (int64_t)p * sp * D : 0;
    if (good) gok |= 1u << r;
  }

  // gout row: tril chunk c is floats 4 c .. 4 c + 3 (it may run up to 3
  // floats into the bottom part, never past the row: D >= 8)
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[IO::NIT], vt[2], vb;
#define DIF_LOAD_ROW(bb)                                                      \
  {                                                                           \
    const float* grow = gout + (bb) * (int64_t)out_w;                         \
    vt[0] = vt[1] = vb = z4;                                                  \
    if (lane * 4 < tri_n) {                                                   \
      vt[0] = *reinterpret_cast<const f32x4_u*>(&grow[lane * 4]);             \
    }                                                                         \
    if ((lane + WAVE) * 4 < tri_n) {                                          \
      vt[1] = *reinterpret_cast<const f32x4_u*>(&grow[(lane + WAVE) * 4]);    \
    }                                                                         \
    if (lane < D4) {                                                          \
      vb = *reinterpret_cast<const f32x4_u*>(&grow[tri_n + lane * 4]);        \
    }                                                                         \
    io.load(v, bottom + (bb)*bstride, packed + (bb)*sbd);                     \
  }
  DIF_LOAD_ROW(b)
  for (; b < B; b += n_waves) {
    io.to_image(v, img);
    *reinterpret_cast<f32x4*>(&stage[lane * 4]) = vt[0];
    *reinterpret_cast<f32x4*>(&stage[(lane + WAVE) * 4]) = vt[1];
    if (lane < D4) *reinterpret_cast<f32x4*>(&gb[lane * 4]) = vb;
    dif_lds_fence();
    const int64_t bn = b + n_waves;
    if (bn < B) DIF_LOAD_ROW(bn)

    // A operand Gs[i = f][k], k = 16 (s / 8) + s % 8 + 8 h: zero on the
    // diagonal and beyond F
    float ga[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int k = 16 * (s >> 3) + (s & 7) + 8 * h;
      const bool good = f < F && k < F && f != k;
      const int r = f > k ? f : k, c = f > k ? k : f;
      const float g = stage[good ? r * (r - 1) / 2 + c : 0];
      ga[s] = good ? g : 0.f;
    }
    float* gbb = gbottom + b * bstride;
    float* gpb = gpacked + b * sbd;
#pragma unroll 1
    for (int d0 = 0; d0 < D; d0 += 32) {
      const int d = d0 + f;
      const bool din = d < D;
      const int dc = din ? d : 0;
      f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                    0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      // bottom-concat gradient: row 0 is register 0 of lanes < 32
      const float g0 = gb[dc];
      acc[0] = (din && h == 0) ? g0 : 0.f;
      const float* xc = img + 8 * h * LD + dc;
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int k0 = 16 * (s >> 3) + (s & 7);
        if (k0 < F) {  // wave-uniform
          const float xv = xc[k0 * LD];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[s], din ? xv : 0.f, acc,
                                                     0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (din && ((gok >> r) & 1)) {
          const bool row0 = h == 0 && r == 0;
          (row0 ? gbb : gpb)[goff[r] + d] = acc[r];
        }
      }
    }
    dif_lds_fence();  // the next sample overwrites the images
  }
#undef DIF_LOAD_ROW
}

static void dif_check(int F, int D) {
  if (F < 1 || F > 32 || D < 8 || D > 256 || D % 8 != 0) {
    throw std::invalid_argument(
        "dot_interact f32 kernels: 1 <= F <= 32, D % 8 == 0, 8 <= D <= 256");
  }
}

// waves (= samples in flight) per block: as many as DIF_LDS_MAX holds
static int dif_wpb(size_t per_wave_bytes) {
  int wpb = DIF_WPB_MAX;
  while (wpb > 1 && wpb * per_wave_bytes > DIF_LDS_MAX) wpb >>= 1;
  return wpb;
}

static int dif_blocks(int64_t B, int wpb) {
  const int64_t blocks = (B + wpb - 1) / wpb;
  return (int)(blocks < DIF_GRID_MAX ? blocks : DIF_GRID_MAX);
}

#define DIF_DISPATCH(L)                                                       \
  if (D == 128) { L(128, 128); } else if (D == 64) { L(64, 64); }             \
  else if (D < 64) { L(64, 0); } else if (D < 128) { L(128, 0); }             \
  else { L(256, 0); }

static void dif_launch_fwd(const void* bottom, const void* packed,
                           const int* perm, void* out, int64_t B, int F, int D,
                           int out_w, int tri_n, int64_t bstride, int64_t sb,
                           int64_t sp, hipStream_t stream) {
  dif_check(F, D);
  if (B == 0) return;
  const size_t per_wave = (size_t)(32 * (D + 4) + DIF_STAGE) * sizeof(float);
  const int wpb = dif_wpb(per_wave);
  const int blocks = dif_blocks(B, wpb);
#define LFWD(DC, DFIX)                                                        \
  hipLaunchKernelGGL((dot_interact_f32_fwd<DC, DFIX>), dim3(blocks),          \
                     dim3(wpb* WAVE), wpb* per_wave, stream,                  \
                     (const float*)bottom, (const float*)packed, perm,        \
                     (float*)out, B, F, D, out_w, tri_n, bstride, sb, sp)
  DIF_DISPATCH(LFWD)
#undef LFWD
}

static void dif_launch_bwd(const void* gout, const void* bottom,
                           const void* packed, const int* perm, void* gbottom,
                           void* gpacked, int64_t B, int F, int D, int out_w,
                           int tri_n, int64_t bstride, int64_t sb, int64_t sp,
                           hipStream_t stream) {
  dif_check(F, D);
  if (B == 0) return;
  const size_t per_wave =
      (size_t)(32 * (D + 4) + DIF_STAGE + D) * sizeof(float);
  const int wpb = dif_wpb(per_wave);
  const int blocks = dif_blocks(B, wpb);
#define LBWD(DC, DFIX)                                                        \
  hipLaunchKernelGGL((dot_interact_f32_bwd<DC, DFIX>), dim3(blocks),          \
                     dim3(wpb* WAVE), wpb* per_wave, stream,                  \
                     (const float*)gout, (const float*)bottom,                \
                     (const float*)packed, perm, (float*)gbottom,             \
                     (float*)gpacked, B, F, D, out_w, tri_n, bstride, sb, sp)
  DIF_DISPATCH(LBWD)
#undef LBWD
}
#undef DIF_DISPATCH

void launch_dot_interact_f32_fwd(const void* feats, void* out, int64_t B,
                                 int F, int D, int out_w, int tri_n,
                                 hipStream_t stream) {
  dif_launch_fwd(feats, feats, nullptr, out, B, F, D, out_w, tri_n,
                 (int64_t)F * D, F, 1, stream);
}

void launch_dot_interact_f32_bwd(const void* gout, const void* feats,
                                 void* gfeats, int64_t B, int F, int D,
                                 int out_w, int tri_n, hipStream_t stream) {
  dif_launch_bwd(gout, feats, feats, nullptr, gfeats, gfeats, B, F, D, out_w,
                 tri_n, (int64_t)F * D, F, 1, stream);
}

void launch_dot_interact_f32_fwd_packed(const void* bottom, const void* packed,
                                        const int* perm, void* out, int64_t B,
                                        int F, int D, int out_w, int tri_n,
                                        int64_t sb, int64_t sp,
                                        hipStream_t stream) {
  dif_launch_fwd(bottom, packed, perm, out, B, F, D, out_w, tri_n, D, sb, sp,
                 stream);
}

void launch_dot_interact_f32_bwd_packed(const void* gout, const void* bottom,
                                        const void* packed, const int* perm,
                                        void* gbottom, void* gpacked, int64_t B,
                                        int F, int D, int out_w, int tri_n,
                                        int64_t sb, int64_t sp,
                                        hipStream_t stream) {
  dif_launch_bwd(gout, bottom, packed, perm, gbottom, gpacked, B, F, D, out_w,
                 tri_n, D, sb, sp, stream);
}
