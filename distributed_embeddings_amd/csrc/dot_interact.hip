// Fused DLRM pairwise-dot interaction for gfx950 (MFMA bf16).
//
// forward:  feats [B, F, D] bf16 (feature 0 = bottom-MLP output)
//        -> out [B, OUT] bf16 = [tril(feats @ feats^T) | feats[:,0,:] | 0-pad]
// backward: gout [B, OUT] bf16 -> gfeats [B, F, D] bf16
//           (gfeats = (G + G^T) @ feats, + bottom-concat grad into row 0)
//
// Replaces the reference's stack + bmm + tril boolean-mask + concat chain
// (examples/dlrm/utils.py:92-113) with one kernel each way: per sample the
// 32x32 Gram tile is 12 v_mfma_f32_16x16x32_bf16 ops (lower-triangle tiles
// only), staged through an LDS copy of the sample's [32, D] feature block.
// 33 <= F <= 64 takes the 64-row kernels at the end of this file: a 4x4 grid
// of 16x16 tiles, 10 of them on or below the diagonal.
// Requirements: bf16 inputs, D % 32 == 0, and F <= 32, or F <= 64 with
// D <= 256.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <stdexcept>

#include "ops_api.h"

#define WAVE 64

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// A/B fragment gather for v_mfma_f32_16x16x32_bf16:
//   A[row = lane%16][k = (lane/16)*8 + r],  B[k][col = lane%16] — r in [0,8).
// C/D: col = lane&15, row = (lane>>4)*4 + reg.
// (cdna_hip_programming.md §3; verified on hardware by the asymmetric
// bmm-oracle test in tests/test_gpu.py.)

// Forward: one wave per sample.
template <int FMAX>  // padded feature count (32)
__global__ void dot_interact_fwd(const __hip_bfloat16* __restrict__ feats,
                                 __hip_bfloat16* __restrict__ out, int64_t B,
                                 int F, int D, int out_w, int tri_n) {
  extern __shared__ short lds_all[];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int ldst = D + 8;  // +16B row pad: avoids 256B-row bank conflicts
  short* lds = lds_all + wave * FMAX * ldst;  // [FMAX][D+8] bf16 (as short)
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;

  for (int64_t b = wave_id; b < B; b += n_waves) {
    const short* src = reinterpret_cast<const short*>(feats) + b * (int64_t)F * D;
    // stage sample into LDS (pad rows >= F with zeros), 8 bf16 per lane-step
    const int total8 = FMAX * D / 8;
    for (int i = lane; i < total8; i += WAVE) {
      const int elem = i * 8;
      const int row = elem / D, col = elem % D;
      if (elem < F * D) {
        *reinterpret_cast<bf16x8*>(&lds[row * ldst + col]) =
            *reinterpret_cast<const bf16x8*>(&src[elem]);
      } else {
        bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<bf16x8*>(&lds[row * ldst + col]) = z;
      }
    }
    // per-wave LDS: hipcc inserts the lgkm waits for its own ds ops

    const int r16 = lane & 15;      // fragment row/col within 16
    const int khalf = lane >> 4;    // 0..3 -> k = khalf*8 + r

    // lower-triangle 16x16 tiles: (0,0), (1,0), (1,1)
    const int tiles_mi[3] = {0, 1, 1};
    const int tiles_ni[3] = {0, 0, 1};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int mi = tiles_mi[t], ni = tiles_ni[t];
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < D; k0 += 32) {
        // a_frag: rows of tile mi; b_frag: rows of tile ni (B = A^T)
        bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &lds[(mi * 16 + r16) * ldst + k0 + khalf * 8]);
        bf16x8 bfr = *reinterpret_cast<const bf16x8*>(
            &lds[(ni * 16 + r16) * ldst + k0 + khalf * 8]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, acc, 0, 0, 0);
      }
      // scatter lower-triangle entries
      __hip_bfloat16* orow = out + b * (int64_t)out_w;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = mi * 16 + (lane >> 4) * 4 + reg;
        const int j = ni * 16 + (lane & 15);
        if (i > j && i < F && j < F) {
          orow[i * (i - 1) / 2 + j] = __hip_bfloat16(acc[reg]);
        }
      }
    }
    // bottom-MLP re-concat + zero pad (bit copy of bf16 pattern)
    short* orow_s = reinterpret_cast<short*>(out + b * (int64_t)out_w);
    for (int c = lane; c < D; c += WAVE) {
      orow_s[tri_n + c] = lds[c];
    }
    for (int c = tri_n + D + lane; c < out_w; c += WAVE) {
      orow_s[c] = 0;
    }
  }
}

// Backward: one wave per sample.  gfeats = (G + G^T) @ feats + bottom grad.
template <int FMAX>
__global__ void dot_interact_bwd(const __hip_bfloat16* __restrict__ gout,
                                 const __hip_bfloat16* __restrict__ feats,
                                 __hip_bfloat16* __restrict__ gfeats, int64_t B,
                                 int F, int D, int out_w, int tri_n) {
  extern __shared__ short lds_all[];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  // layout per wave: [FMAX][D] feats  +  [FMAX][FMAX] G_sym
  short* lds = lds_all + wave * (FMAX * D + FMAX * FMAX);
  short* gsym = lds + FMAX * D;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;

  for (int64_t b = wave_id; b < B; b += n_waves) {
    const short* src = reinterpret_cast<const short*>(feats) + b * (int64_t)F * D;
    const int total8 = FMAX * D / 8;
    for (int i = lane; i < total8; i += WAVE) {
      const int elem = i * 8;
      if (elem < F * D) {
        *reinterpret_cast<bf16x8*>(&lds[elem]) =
            *reinterpret_cast<const bf16x8*>(&src[elem]);
      } else {
        bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<bf16x8*>(&lds[elem]) = z;
      }
    }
    // build G_sym [FMAX][FMAX] from the tril grad
    const __hip_bfloat16* grow = gout + b * (int64_t)out_w;
    for (int idx = lane; idx < FMAX * FMAX; idx += WAVE) {
      const int i = idx / FMAX, j = idx % FMAX;
      float g = 0.f;
      if (i < F && j < F && i != j) {
        const int r = i > j ? i : j, c = i > j ? j : i;
        g = float(grow[r * (r - 1) / 2 + c]);
      }
      __hip_bfloat16 hb(g);
      gsym[idx] = *reinterpret_cast<short*>(&hb);
    }

    const int r16 = lane & 15;
    const int khalf = lane >> 4;
    __hip_bfloat16* gf = gfeats + b * (int64_t)F * D;

    // grad_A = G_sym @ A : M=FMAX rows, N=D cols, K=FMAX (=32: one K step)
    for (int nj = 0; nj < D / 16; ++nj) {
#pragma unroll
      for (int mi = 0; mi < FMAX / 16; ++mi) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k0 = 0; k0 < FMAX; k0 += 32) {
          // A-op = G_sym[mi*16 + r16][k0 + khalf*8 + r]
          bf16x8 a = *reinterpret_cast<const bf16x8*>(
              &gsym[(mi * 16 + r16) * FMAX + k0 + khalf * 8]);
          // B-op[k][col] = feats[k][nj*16 + r16]: k = k0 + khalf*8 + r
          bf16x8 bfr;
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            bfr[r] = lds[(k0 + khalf * 8 + r) * D + nj * 16 + r16];
          }
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = mi * 16 + (lane >> 4) * 4 + reg;
          const int j = nj * 16 + (lane & 15);
          if (i < F && j < D) {
            float v = acc[reg];
            if (i == 0) v += float(grow[tri_n + j]);  // bottom-concat grad
            gf[i * D + j] = __hip_bfloat16(v);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Packed variants: feats live as TWO tensors — bottom [B, D] (feature 0) and
// packed [P, B, D] (P = F-1 embedding outputs, feature-major).  The packed
// block is exactly the fused-group lookup output (world==1) or the mp->dp
// all-to-all recv buffer (world>1) VIEWED in place, so the torch.stack /
// per-pair split+merge copies disappear from the step.  `perm[f-1]` maps
// feature f (model input order) to its packed row (worker order) — a small
// device-resident buffer built once from the plan, keeping the interaction
// column order identical at every world size.
// ---------------------------------------------------------------------------

// sb/sp: element-row strides of the packed block — feature-major [P,B,D]
// uses (sb=1, sp=B); sample-major [B,P,D] uses (sb=P, sp=1).
//
// Block-cooperative IO: each workgroup (WPB waves) handles WPB consecutive
// samples.  In the feature-major layout the WPB samples' rows are ADJACENT
// within each feature plane, so a cooperative load moves WPB*256 B
// contiguous per plane instead of per-wave 256 B scatters (measured 2-3x
// kernel time on the scattered variant).  The backward additionally stages
// its [F, D] grad in LDS (overwriting nothing the MFMA still needs) and
// writes it back cooperatively the same way.

// waves (= samples) per block: templated; DI_WPB_FWD / DI_WPB_BWD are the
// measured defaults (tools/bench_interact.py sweep with the fixed-width
// kernels below, profiles/interact_latency.md); DE_DI_WPB env selects 2/4/8
// for both directions, for measurement.  The first two kernels take a
// run-time D and serve the widths that have no fixed-width instance.
#define DI_WPB_FWD 4
#define DI_WPB_BWD 4
static int di_wpb(int dflt) {
  static int v = [] {
    const char* e = getenv("DE_DI_WPB");
    if (!e) return 0;
    int i = atoi(e);
    return (i == 2 || i == 4 || i == 8) ? i : 0;
  }();
  return v ? v : dflt;
}

template <int FMAX, int WPB>
__global__ void dot_interact_fwd_packed_rt(
    const __hip_bfloat16* __restrict__ bottom,
    const __hip_bfloat16* __restrict__ packed,
    const int* __restrict__ perm, __hip_bfloat16* __restrict__ out, int64_t B,
    int F, int D, int out_w, int tri_n, int64_t sb, int64_t sp) {
  extern __shared__ short lds_all[];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int tid = threadIdx.x;
  const int ldst = D + 8;
  short* lds = lds_all + wave * FMAX * ldst;
  const int d8 = D / 8;

  for (int64_t b0 = (int64_t)blockIdx.x * WPB; b0 < B;
       b0 += (int64_t)gridDim.x * WPB) {
    // cooperative load: chunk i -> (row, sample w, col); per row the WPB
    // samples' segments are contiguous in the feature-major layout
    for (int i = tid; i < FMAX * WPB * d8; i += WPB * WAVE) {
      const int row = i / (WPB * d8);
      const int rem = i % (WPB * d8);
      const int w = rem / d8;
      const int col = (rem % d8) * 8;
      const int64_t b = b0 + w;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (b < B) {
        if (row == 0) {
          v = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const short*>(bottom) + b * (int64_t)D + col);
        } else if (row < F) {
          v = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const short*>(packed) +
              ((int64_t)perm[row - 1] * sp + b * sb) * (int64_t)D + col);
        }
      }
      *reinterpret_cast<bf16x8*>(
          &lds_all[w * FMAX * ldst + row * ldst + col]) = v;
    }
    __syncthreads();

    const int64_t b = b0 + wave;
    if (b < B) {
      const int r16 = lane & 15;
      const int khalf = lane >> 4;
      const int tiles_mi[3] = {0, 1, 1};
      const int tiles_ni[3] = {0, 0, 1};
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int mi = tiles_mi[t], ni = tiles_ni[t];
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += 32) {
          bf16x8 a = *reinterpret_cast<const bf16x8*>(
              &lds[(mi * 16 + r16) * ldst + k0 + khalf * 8]);
          bf16x8 bfr = *reinterpret_cast<const bf16x8*>(
              &lds[(ni * 16 + r16) * ldst + k0 + khalf * 8]);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, acc, 0, 0, 0);
        }
        __hip_bfloat16* orow = out + b * (int64_t)out_w;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = mi * 16 + (lane >> 4) * 4 + reg;
          const int j = ni * 16 + (lane & 15);
          if (i > j && i < F && j < F) {
            orow[i * (i - 1) / 2 + j] = __hip_bfloat16(acc[reg]);
          }
        }
      }
      short* orow_s = reinterpret_cast<short*>(out + b * (int64_t)out_w);
      for (int c = lane; c < D; c += WAVE) {
        orow_s[tri_n + c] = lds[c];
      }
      for (int c = tri_n + D + lane; c < out_w; c += WAVE) {
        orow_s[c] = 0;
      }
    }
    __syncthreads();
  }
}

template <int FMAX, int WPB>
__global__ void dot_interact_bwd_packed_rt(
    const __hip_bfloat16* __restrict__ gout,
    const __hip_bfloat16* __restrict__ bottom,
    const __hip_bfloat16* __restrict__ packed, const int* __restrict__ perm,
    __hip_bfloat16* __restrict__ gbottom, __hip_bfloat16* __restrict__ gpacked,
    int64_t B, int F, int D, int out_w, int tri_n, int64_t sb, int64_t sp) {
  extern __shared__ short lds_all[];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int tid = threadIdx.x;
  // per wave: [FMAX][D] feats + [FMAX][FMAX] gsym.  The feats region is
  // REUSED for the grad: each nj column chunk is overwritten only after
  // both mi MFMA passes buffered their results in registers (keeps LDS at
  // 40KB/workgroup -> 4 workgroups/CU).
  const int per_wave = FMAX * D + FMAX * FMAX;
  short* lds = lds_all + wave * per_wave;
  short* gsym = lds + FMAX * D;
  const int d8 = D / 8;

  for (int64_t b0 = (int64_t)blockIdx.x * WPB; b0 < B;
       b0 += (int64_t)gridDim.x * WPB) {
    for (int i = tid; i < FMAX * WPB * d8; i += WPB * WAVE) {
      const int row = i / (WPB * d8);
      const int rem = i % (WPB * d8);
      const int w = rem / d8;
      const int col = (rem % d8) * 8;
      const int64_t b = b0 + w;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (b < B) {
        if (row == 0) {
          v = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const short*>(bottom) + b * (int64_t)D + col);
        } else if (row < F) {
          v = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const short*>(packed) +
              ((int64_t)perm[row - 1] * sp + b * sb) * (int64_t)D + col);
        }
      }
      *reinterpret_cast<bf16x8*>(
          &lds_all[w * per_wave + row * D + col]) = v;
    }
    __syncthreads();

    const int64_t b = b0 + wave;
    if (b < B) {
      const __hip_bfloat16* grow = gout + b * (int64_t)out_w;
      for (int idx = lane; idx < FMAX * FMAX; idx += WAVE) {
        const int i = idx / FMAX, j = idx % FMAX;
        float g = 0.f;
        if (i < F && j < F && i != j) {
          const int r = i > j ? i : j, c = i > j ? j : i;
          g = float(grow[r * (r - 1) / 2 + c]);
        }
        __hip_bfloat16 hb(g);
        gsym[idx] = *reinterpret_cast<short*>(&hb);
      }

      const int r16 = lane & 15;
      const int khalf = lane >> 4;
      for (int nj = 0; nj < D / 16; ++nj) {
        f32x4 accs[FMAX / 16];
#pragma unroll
        for (int mi = 0; mi < FMAX / 16; ++mi) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k0 = 0; k0 < FMAX; k0 += 32) {
            bf16x8 a = *reinterpret_cast<const bf16x8*>(
                &gsym[(mi * 16 + r16) * FMAX + k0 + khalf * 8]);
            bf16x8 bfr;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
              bfr[r] = lds[(k0 + khalf * 8 + r) * D + nj * 16 + r16];
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, acc, 0, 0, 0);
          }
          accs[mi] = acc;
        }
        // both mi passes read columns nj*16.. — now overwrite them in place
#pragma unroll
        for (int mi = 0; mi < FMAX / 16; ++mi) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int i = mi * 16 + (lane >> 4) * 4 + reg;
            const int j = nj * 16 + (lane & 15);
            float v = accs[mi][reg];
            if (i == 0) v += float(grow[tri_n + j]);
            __hip_bfloat16 hb(v);
            lds[i * D + j] = *reinterpret_cast<short*>(&hb);
          }
        }
      }
    }
    __syncthreads();

    // cooperative write-back: same (row, sample, col) mapping as the load
    for (int i = tid; i < FMAX * WPB * d8; i += WPB * WAVE) {
      const int row = i / (WPB * d8);
      const int rem = i % (WPB * d8);
      const int w = rem / d8;
      const int col = (rem % d8) * 8;
      const int64_t b = b0 + w;
      if (b >= B || row >= F) continue;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(
          &lds_all[w * per_wave + row * D + col]);
      if (row == 0) {
        *reinterpret_cast<bf16x8*>(
            reinterpret_cast<short*>(gbottom) + b * (int64_t)D + col) = v;
      } else {
        *reinterpret_cast<bf16x8*>(
            reinterpret_cast<short*>(gpacked) +
            ((int64_t)perm[row - 1] * sp + b * sb) * (int64_t)D + col) = v;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Packed kernels with a compile-time width (D = 32, 64, 128, 256); every
// other D % 32 == 0 takes the run-time-D kernels above.
//
// What the fixed width buys (gfx950 assembly, profiles/interact_latency.md):
//  - chunk -> (row, sample, col) is shifts and masks, and (sample, col) do not
//    depend on the pass, so a thread computes them once;
//  - perm is read once per thread, before the first feature load, and kept
//    in registers as the row's element offset, for the load and the
//    write-back alike;
//  - the cooperative loops are fully unrolled with all global loads of a
//    sample group issued before the first LDS write (D/16 x 16 B per thread
//    in flight), and the write-back reads LDS the same way ahead of its
//    stores.
//
// Chunk mapping, thread tid, pass it (D8 = D/8 chunks per row):
//   row = it * (64 / D8) + tid / (WPB * D8)
//   w   = (tid / D8) % WPB          sample within the block
//   col = (tid % D8) * 8
// so per row the WPB samples' segments are still contiguous (feature-major).
//
// The rows of out / gout start at b * out_w elements, which is 2-byte
// aligned and no more (out_w = 479 without padding at the bench's F and D);
// they are moved as 16-B vectors through a 2-byte-aligned type.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef bf16x8 __attribute__((aligned(2))) bf16x8_u;
typedef short v4i16_t __attribute__((vector_size(8)));
typedef __attribute__((address_space(3))) v4i16_t lds_v4i16_t;

// LDS writes of one lane read back by another lane of the same wave: the LDS
// executes a wave's operations in order, this keeps the compiler from moving
// them across.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ short f32_to_bf16_bits(float v) {
  __hip_bfloat16 hb(v);
  return *reinterpret_cast<short*>(&hb);
}

__device__ __forceinline__ float bf16_bits_to_f32(short s) {
  return __builtin_bit_cast(float, (unsigned)(unsigned short)s << 16);
}

// Backward LDS image: plain D-element rows whose 16-B chunks are XORed with
// a function of the row, so that the 16 rows of an MFMA tile put one column
// chunk on 16 different bank groups.  Without it every row of a 256-B-stride
// image starts on bank 0: the transposed reads (8 rows per 32-lane half) and
// the 8-B result stores (16 rows) serialize.  Element offset of (row, col):
template <int D>
__device__ __forceinline__ int swz(int row, int col) {
  const int sw = (((row & 3) << 2) | ((row >> 2) & 3)) & (D / 8 - 1);
  return row * D + ((((col >> 3) ^ sw) << 3) | (col & 7));
}

template <int D, int WPB>
struct PackedIO {
  static constexpr int D8 = D / 8;
  static constexpr int RPI = WAVE / D8;  // rows per pass
  static constexpr int NIT = 32 / RPI;   // passes = 16-B chunks per thread
  int r0, w, col;
  int64_t b;         // this thread's sample
  int64_t off[NIT];  // element offset of its chunk of pass `it` in bottom
                     // (row 0) or packed: the load and the write-back share it

  __device__ __forceinline__ PackedIO(const int* __restrict__ perm, int F,
                                      int64_t b0, int64_t sb, int64_t sp) {
    const int tid = threadIdx.x;
    r0 = tid / (WPB * D8);
    w = (tid / D8) % WPB;
    col = (tid % D8) * 8;
    b = b0 + w;
    int prow[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      // clamped index, not a branch: the NIT loads go out together.
      // F >= 2: the launcher sees to it
      const int row = it * RPI + r0;
      const int pi = row < 1 ? 0 : (row < F ? row - 1 : F - 2);
      prow[it] = perm[pi];
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      // rows >= F are never addressed
      const int row = it * RPI + r0;
      off[it] = row == 0 ? b * D + col
                         : (prow[it] * sp + b * sb) * (int64_t)D + col;
    }
    // perm is consumed here, in one wait, ahead of every predicated load: a
    // wait placed among those has to assume that none of them was issued and
    // so waits for all of them.  The empty asm pins the offsets to this point.
#pragma unroll
    for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(off[it]));
  }

  // global -> LDS image [w][32][LD] (+ PER_WAVE between samples), rows >= F
  // and samples >= B zero-filled
  template <int LD, int PER_WAVE, bool SWZ>
  __device__ __forceinline__ void load(const short* __restrict__ bottom,
                                       const short* __restrict__ packed,
                                       short* lds_all, int64_t B, int F) const {
    bf16x8 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * RPI + r0;
      const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      v[it] = z;
      if (b < B && row < F) {
        v[it] = *reinterpret_cast<const bf16x8*>(
            (row == 0 ? bottom : packed) + off[it]);
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * RPI + r0;
      const int at_lds = SWZ ? swz<D>(row, col) : row * LD + col;
      *reinterpret_cast<bf16x8*>(&lds_all[w * PER_WAVE + at_lds]) = v[it];
    }
  }
};

template <int D, int WPB>
__global__ __launch_bounds__(WPB* WAVE) void dot_interact_fwd_packed(
    const __hip_bfloat16* __restrict__ bottom,
    const __hip_bfloat16* __restrict__ packed,
    const int* __restrict__ perm, __hip_bfloat16* __restrict__ out, int64_t B,
    int F, int out_w, int tri_n, int64_t sb, int64_t sp) {
  extern __shared__ short lds_all[];
  constexpr int LD = D + 8;  // +16 B row pad, as the unpacked forward
  constexpr int PER_WAVE = 32 * LD;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (WAVE - 1);
  short* lds = lds_all + wave * PER_WAVE;
  // one block, one group of WPB samples: with a grid-stride loop here the
  // compiler hoists every LDS address out of it and runs out of registers
  const int64_t b0 = (int64_t)blockIdx.x * WPB;
  const PackedIO<D, WPB> io(perm, F, b0, sb, sp);
  {
    io.template load<LD, PER_WAVE, false>(
        reinterpret_cast<const short*>(bottom),
        reinterpret_cast<const short*>(packed), lds_all, B, F);
    __syncthreads();

    const int64_t b = b0 + wave;
    if (b < B) {
      const int r16 = lane & 15;
      const int khalf = lane >> 4;
      const int tiles_mi[3] = {0, 1, 1};
      const int tiles_ni[3] = {0, 0, 1};
      f32x4 accs[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int mi = tiles_mi[t], ni = tiles_ni[t];
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k0 = 0; k0 < D; k0 += 32) {
          bf16x8 a = *reinterpret_cast<const bf16x8*>(
              &lds[(mi * 16 + r16) * LD + k0 + khalf * 8]);
          bf16x8 bfr = *reinterpret_cast<const bf16x8*>(
              &lds[(ni * 16 + r16) * LD + k0 + khalf * 8]);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, acc, 0, 0, 0);
        }
        accs[t] = acc;
      }
      // Rows 1.. of the tile are dead once all three products are in
      // registers: the output row [tril | bottom | 0 up to a multiple of 8]
      // is assembled there (<= 496 + D + 7 of the 31 * LD elements) and
      // leaves as 16-B vectors.  Row 0 (bottom) stays where it is.
      wave_lds_fence();
      short* stage = lds + LD;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = tiles_mi[t] * 16 + khalf * 4 + reg;
          const int j = tiles_ni[t] * 16 + r16;
          if (i > j && i < F) {
            stage[i * (i - 1) / 2 + j] = f32_to_bf16_bits(accs[t][reg]);
          }
        }
      }
#pragma unroll
      for (int c = lane; c < D; c += WAVE) stage[tri_n + c] = lds[c];
      const int width = tri_n + D;
      const int width8 = (width + 7) & ~7;
      if (width + lane < width8) stage[width + lane] = 0;
      wave_lds_fence();

      short* orow = reinterpret_cast<short*>(out) + b * (int64_t)out_w;
      const int nfull = out_w >> 3;  // whole 16-B chunks of the row
      for (int c = lane; c < nfull; c += WAVE) {
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (c * 8 < width8) v = *reinterpret_cast<const bf16x8*>(&stage[c * 8]);
        *reinterpret_cast<bf16x8_u*>(&orow[c * 8]) = v;
      }
      const int e = nfull * 8 + lane;  // the row's last out_w % 8 elements
      if (e < out_w) orow[e] = e < width ? stage[e] : (short)0;
    }
    __syncthreads();
  }
}

// Backward, transposed product: gfeats^T[d][i] = sum_k X[k][d] * G[k][i].
//  - A operand X^T: ds_read_b64_tr_b16 of the [32][D] image (swz above).  The
//    16-lane group g takes rows 8g..8g+3 and 8g+4..8g+7 of columns
//    d0..d0+15; lane 4q+p of the group supplies row q, columns 4p..4p+3.
//    EXEC is all ones: the only branch around it is on the wave's own
//    sample index, held in an SGPR.  The two groups of a 32-lane half read
//    blocks 8 rows apart in the same columns: 32 distinct 8-B slots.
//  - B operand G[k][i] = G[i][k] (symmetric): 8 consecutive k of row i,
//    the same for every d0, so both 16-feature fragments are built once per
//    sample and kept in registers.
//  - C: lane holds d = d0 + 4*(lane>>4) + reg of feature i = lane & 15: one
//    8-B LDS store per tile.
// The sample's gout row comes in with 16-B loads into the 2 KB that held
// G_sym: tril chunks at [0, 496) (a chunk may run up to 7 elements into the
// bottom part, never past the row: D >= 32), the bottom part again at
// [1024 - D, 1024) so that it is 8-B aligned for the C-operand read.
// LDS per wave stays 32*D + 1024 elements.
template <int D, int WPB>
__global__ __launch_bounds__(WPB* WAVE, D >= 256 ? 2 : 4) void
dot_interact_bwd_packed(
    const __hip_bfloat16* __restrict__ gout,
    const __hip_bfloat16* __restrict__ bottom,
    const __hip_bfloat16* __restrict__ packed, const int* __restrict__ perm,
    __hip_bfloat16* __restrict__ gbottom, __hip_bfloat16* __restrict__ gpacked,
    int64_t B, int F, int out_w, int tri_n, int64_t sb, int64_t sp) {
  static_assert(496 + 7 + D <= 1024, "gout row staging needs D <= 256");
  extern __shared__ short lds_all[];
  constexpr int PER_WAVE = 32 * D + 1024;
  constexpr int D8 = D / 8;
  constexpr int NJ = D / 16;
  using IO = PackedIO<D, WPB>;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (WAVE - 1);
  short* lds = lds_all + wave * PER_WAVE;
  short* stage = lds + 32 * D;
  short* gb = stage + 1024 - D;
  // one block, one group of WPB samples (see the forward)
  const int64_t b0 = (int64_t)blockIdx.x * WPB;
  const IO io(perm, F, b0, sb, sp);
  {
    // the sample's gout row goes out ahead of the feature loads
    const int64_t b = b0 + wave;
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 vt = z, vb = z;
    if (b < B) {
      const short* grow = reinterpret_cast<const short*>(gout) +
                          b * (int64_t)out_w;
      if (lane * 8 < tri_n) {
        vt = *reinterpret_cast<const bf16x8_u*>(&grow[lane * 8]);
      }
      if (lane < D8) {
        vb = *reinterpret_cast<const bf16x8_u*>(&grow[tri_n + lane * 8]);
      }
    }
    io.template load<D, PER_WAVE, true>(
        reinterpret_cast<const short*>(bottom),
        reinterpret_cast<const short*>(packed), lds_all, B, F);
    if (b < B) {
      if (lane * 8 < tri_n) *reinterpret_cast<bf16x8*>(&stage[lane * 8]) = vt;
      if (lane < D8) *reinterpret_cast<bf16x8*>(&gb[lane * 8]) = vb;
    }
    __syncthreads();

    if (b < B) {
      const int r16 = lane & 15;
      const int khalf = lane >> 4;
      bf16x8 g[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = ni * 16 + r16, k = khalf * 8 + j;
          const bool ok = i < F && k < F && i != k;
          const int r = i > k ? i : k, c = i > k ? k : i;
          const short s = stage[ok ? r * (r - 1) / 2 + c : 0];
          g[ni][j] = ok ? s : (short)0;
        }
      }
      const int xrow = khalf * 8 + (r16 >> 2), xcol = (lane & 3) * 4;
      // NJB column tiles at a time: their X^T operands are all read before
      // the first of their results is stored, and a result only overwrites
      // columns that no later tile reads, so the gradient replaces the
      // features in place
      constexpr int NJB = NJ < 4 ? NJ : 4;
#pragma unroll
      for (int nj0 = 0; nj0 < NJ; nj0 += NJB) {
        bf16x8 a[NJB];
        bf16x4 gbv[NJB];
#pragma unroll
        for (int t = 0; t < NJB; ++t) {
          const int d0 = (nj0 + t) * 16;
          const v4i16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_v4i16_t*)(lds + swz<D>(xrow, d0 + xcol)));
          const v4i16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_v4i16_t*)(lds + swz<D>(xrow + 4, d0 + xcol)));
          a[t] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          gbv[t] = *reinterpret_cast<const bf16x4*>(&gb[d0 + khalf * 4]);
        }
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < NJB; ++t) {
          const int d0 = (nj0 + t) * 16;
          // bottom-concat gradient of feature 0: the C operand of its column
          f32x4 c0 = {0.f, 0.f, 0.f, 0.f};
          if (r16 == 0) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              c0[reg] = bf16_bits_to_f32(gbv[t][reg]);
            }
          }
          const f32x4 zc = {0.f, 0.f, 0.f, 0.f};
          const f32x4 acc0 =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], g[0], c0, 0, 0, 0);
          const f32x4 acc1 =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], g[1], zc, 0, 0, 0);
          const bf16x4 o0 = {
              f32_to_bf16_bits(acc0[0]), f32_to_bf16_bits(acc0[1]),
              f32_to_bf16_bits(acc0[2]), f32_to_bf16_bits(acc0[3])};
          const bf16x4 o1 = {
              f32_to_bf16_bits(acc1[0]), f32_to_bf16_bits(acc1[1]),
              f32_to_bf16_bits(acc1[2]), f32_to_bf16_bits(acc1[3])};
          *reinterpret_cast<bf16x4*>(&lds[swz<D>(r16, d0 + khalf * 4)]) = o0;
          *reinterpret_cast<bf16x4*>(
              &lds[swz<D>(16 + r16, d0 + khalf * 4)]) = o1;
        }
        wave_lds_fence();
      }
    }
    __syncthreads();

    // cooperative write-back: the load's mapping, LDS reads ahead of stores
    {
      const int64_t bw = io.b;
      bf16x8 v[IO::NIT];
#pragma unroll
      for (int it = 0; it < IO::NIT; ++it) {
        const int row = it * IO::RPI + io.r0;
        v[it] = *reinterpret_cast<const bf16x8*>(
            &lds_all[io.w * PER_WAVE + swz<D>(row, io.col)]);
      }
#pragma unroll
      for (int it = 0; it < IO::NIT; ++it) {
        const int row = it * IO::RPI + io.r0;
        if (bw < B && row < F) {
          short* dst = reinterpret_cast<short*>(row == 0 ? gbottom : gpacked);
          *reinterpret_cast<bf16x8*>(dst + io.off[it]) = v[it];
        }
      }
    }
    __syncthreads();
  }
}

#define DI_FOR_WPB(M) \
  if (wpb == 2) { M(2); } else if (wpb == 8) { M(8); } else { M(4); }

template <int D>
static void launch_fwd_packed_d(const void* bottom, const void* packed,
                                const int* perm, void* out, int64_t B, int F,
                                int out_w, int tri_n, int64_t sb, int64_t sp,
                                int wpb, int blocks, hipStream_t stream) {
  const size_t lds = (size_t)wpb * 32 * (D + 8) * sizeof(short);
#define LFWD(W)                                                                \
  hipLaunchKernelGGL((dot_interact_fwd_packed<D, W>), dim3(blocks),            \
                     dim3(W * WAVE), lds, stream,                              \
                     (const __hip_bfloat16*)bottom,                            \
                     (const __hip_bfloat16*)packed, perm, (__hip_bfloat16*)out,\
                     B, F, out_w, tri_n, sb, sp)
  DI_FOR_WPB(LFWD)
#undef LFWD
}

template <int D>
static void launch_bwd_packed_d(const void* gout, const void* bottom,
                                const void* packed, const int* perm,
                                void* gbottom, void* gpacked, int64_t B, int F,
                                int out_w, int tri_n, int64_t sb, int64_t sp,
                                int wpb, int blocks, hipStream_t stream) {
  const size_t lds = (size_t)wpb * (32 * D + 32 * 32) * sizeof(short);
#define LBWD(W)                                                                \
  hipLaunchKernelGGL((dot_interact_bwd_packed<D, W>), dim3(blocks),            \
                     dim3(W * WAVE), lds, stream, (const __hip_bfloat16*)gout, \
                     (const __hip_bfloat16*)bottom,                            \
                     (const __hip_bfloat16*)packed, perm,                      \
                     (__hip_bfloat16*)gbottom, (__hip_bfloat16*)gpacked, B, F, \
                     out_w, tri_n, sb, sp)
  DI_FOR_WPB(LBWD)
#undef LBWD
}

void launch_dot_interact_fwd_packed(const void* bottom, const void* packed,
                                    const int* perm, void* out, int64_t B,
                                    int F, int D, int out_w, int tri_n,
                                    int64_t sb, int64_t sp,
                                    hipStream_t stream) {
  const int wpb = di_wpb(DI_WPB_FWD);
  const int64_t groups = (B + wpb - 1) / wpb;
  // one block per sample group, and perm is read unconditionally
  const bool fixed_ok = groups <= INT32_MAX && F >= 2;
  int blocks = (int)groups;
#define LFWD_D(DD)                                                             \
  launch_fwd_packed_d<DD>(bottom, packed, perm, out, B, F, out_w, tri_n, sb,   \
                          sp, wpb, blocks, stream)
  if (fixed_ok && D == 128) { LFWD_D(128); return; }
  if (fixed_ok && D == 64) { LFWD_D(64); return; }
  if (fixed_ok && D == 32) { LFWD_D(32); return; }
  if (fixed_ok && D == 256) { LFWD_D(256); return; }
#undef LFWD_D
  if (groups > 32768) blocks = 32768;  // grid-stride kernels
  const size_t lds = (size_t)wpb * 32 * (D + 8) * sizeof(short);
#define LFWD(W)                                                                \
  hipLaunchKernelGGL((dot_interact_fwd_packed_rt<32, W>), dim3(blocks),        \
                     dim3(W * WAVE), lds, stream,                              \
                     (const __hip_bfloat16*)bottom,                            \
                     (const __hip_bfloat16*)packed, perm, (__hip_bfloat16*)out,\
                     B, F, D, out_w, tri_n, sb, sp)
  DI_FOR_WPB(LFWD)
#undef LFWD
}

void launch_dot_interact_bwd_packed(const void* gout, const void* bottom,
                                    const void* packed, const int* perm,
                                    void* gbottom, void* gpacked, int64_t B,
                                    int F, int D, int out_w, int tri_n,
                                    int64_t sb, int64_t sp,
                                    hipStream_t stream) {
  const int wpb = di_wpb(DI_WPB_BWD);
  const int64_t groups = (B + wpb - 1) / wpb;
  // one block per sample group, and perm is read unconditionally
  const bool fixed_ok = groups <= INT32_MAX && F >= 2;
  int blocks = (int)groups;
#define LBWD_D(DD)                                                             \
  launch_bwd_packed_d<DD>(gout, bottom, packed, perm, gbottom, gpacked, B, F,  \
                          out_w, tri_n, sb, sp, wpb, blocks, stream)
  if (fixed_ok && D == 128) { LBWD_D(128); return; }
  if (fixed_ok && D == 64) { LBWD_D(64); return; }
  if (fixed_ok && D == 32) { LBWD_D(32); return; }
  if (fixed_ok && D == 256) { LBWD_D(256); return; }
#undef LBWD_D
  if (groups > 32768) blocks = 32768;  // grid-stride kernels
  const size_t lds = (size_t)wpb * (32 * D + 32 * 32) * sizeof(short);
#define LBWD(W)                                                                \
  hipLaunchKernelGGL((dot_interact_bwd_packed_rt<32, W>), dim3(blocks),        \
                     dim3(W * WAVE), lds, stream, (const __hip_bfloat16*)gout, \
                     (const __hip_bfloat16*)bottom,                            \
                     (const __hip_bfloat16*)packed, perm,                      \
                     (__hip_bfloat16*)gbottom, (__hip_bfloat16*)gpacked, B, F, \
                     D, out_w, tri_n, sb, sp)
  DI_FOR_WPB(LBWD)
#undef LBWD
}
#undef DI_FOR_WPB

void launch_dot_interact_fwd(const void* feats, void* out, int64_t B, int F,
                             int D, int out_w, int tri_n, hipStream_t stream) {
  const int block = 256;
  const int waves = block / WAVE;
  int64_t blocks = (B + waves - 1) / waves;
  if (blocks > 8192) blocks = 8192;
  const size_t lds = (size_t)waves * 32 * (D + 8) * sizeof(short);
  hipLaunchKernelGGL((dot_interact_fwd<32>), dim3((int)blocks), dim3(block),
                     lds, stream, (const __hip_bfloat16*)feats,
                     (__hip_bfloat16*)out, B, F, D, out_w, tri_n);
}

void launch_dot_interact_bwd(const void* gout, const void* feats, void* gfeats,
                             int64_t B, int F, int D, int out_w, int tri_n,
                             hipStream_t stream) {
  const int block = 256;
  const int waves = block / WAVE;
  int64_t blocks = (B + waves - 1) / waves;
  if (blocks > 8192) blocks = 8192;
  const size_t lds = (size_t)waves * (32 * D + 32 * 32) * sizeof(short);
  hipLaunchKernelGGL((dot_interact_bwd<32>), dim3((int)blocks), dim3(block),
                     lds, stream, (const __hip_bfloat16*)gout,
                     (const __hip_bfloat16*)feats, (__hip_bfloat16*)gfeats, B,
                     F, D, out_w, tri_n);
}

// ---------------------------------------------------------------------------
// 33 <= F <= 64: the same kernels over a 64-row padded feature block, one wave
// per sample.  The kernels above are left as they are, so that F <= 32 runs
// the code and the launch shapes it always ran.
//
// Forward: the 4x4 grid of 16x16 Gram tiles has 10 tiles on or below the
// diagonal, D/32 MFMAs each (40 per sample at D = 128).  A tile row that lies
// wholly beyond F is skipped: F <= 48 computes 6 tiles.  The test is on F
// alone, so it is a scalar branch.
// Backward: G_sym is [64][64]; (G + G^T) X takes two k-steps of 32 per
// 16 x 16 result tile, 4 * D/16 * 2 MFMAs per sample.
//
// LDS per sample: forward 64 * (D + 8) * 2 B (17 KB at D = 128), backward
// (64 * D + 64 * 64) * 2 B (24 KB at D = 128, 40 KB at D = 256).  A block
// holds 1, 2 or 4 samples and never more than DI64_LDS_MAX bytes, which
// every launch gets without asking for a larger dynamic allocation.
// ---------------------------------------------------------------------------

#define DI64_LDS_MAX 65536

// Gram tiles of the [FMAX][ldst] image `lds`, run-time D, scattered straight
// into the sample's output row
template <int FMAX>
__device__ __forceinline__ void gram_tril_scatter(const short* lds, int ldst,
                                                  int D, int F,
                                                  __hip_bfloat16* orow,
                                                  int lane) {
  const int r16 = lane & 15;
  const int khalf = lane >> 4;
#pragma unroll
  for (int mi = 0; mi < FMAX / 16; ++mi) {
    if (mi * 16 < F) {  // wave-uniform
#pragma unroll
      for (int ni = 0; ni <= mi; ++ni) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += 32) {
          bf16x8 a = *reinterpret_cast<const bf16x8*>(
              &lds[(mi * 16 + r16) * ldst + k0 + khalf * 8]);
          bf16x8 bfr = *reinterpret_cast<const bf16x8*>(
              &lds[(ni * 16 + r16) * ldst + k0 + khalf * 8]);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = mi * 16 + khalf * 4 + reg;
          const int j = ni * 16 + r16;
          if (i > j && i < F) {
            orow[i * (i - 1) / 2 + j] = __hip_bfloat16(acc[reg]);
          }
        }
      }
    }
  }
}

// dot_interact_fwd with the tile list generalised to FMAX / 16 tile rows
template <int FMAX>
__global__ void dot_interact_fwd_tiles(const __hip_bfloat16* __restrict__ feats,
                                       __hip_bfloat16* __restrict__ out,
                                       int64_t B, int F, int D, int out_w,
                                       int tri_n) {
  extern __shared__ short lds_all[];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int ldst = D + 8;
  short* lds = lds_all + wave * FMAX * ldst;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;

  for (int64_t b = wave_id; b < B; b += n_waves) {
    const short* src = reinterpret_cast<const short*>(feats) + b * (int64_t)F * D;
    const int total8 = FMAX * D / 8;
    for (int i = lane; i < total8; i += WAVE) {
      const int elem = i * 8;
      const int row = elem / D, col = elem % D;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (elem < F * D) v = *reinterpret_cast<const bf16x8*>(&src[elem]);
      *reinterpret_cast<bf16x8*>(&lds[row * ldst + col]) = v;
    }
    wave_lds_fence();
    gram_tril_scatter<FMAX>(lds, ldst, D, F, out + b * (int64_t)out_w, lane);
    short* orow_s = reinterpret_cast<short*>(out + b * (int64_t)out_w);
    for (int c = lane; c < D; c += WAVE) {
      orow_s[tri_n + c] = lds[c];
    }
    for (int c = tri_n + D + lane; c < out_w; c += WAVE) {
      orow_s[c] = 0;
    }
    wave_lds_fence();
  }
}

// dot_interact_fwd_packed_rt with the tile list generalised
template <int FMAX, int WPB>
__global__ void dot_interact_fwd_packed_rt_tiles(
    const __hip_bfloat16* __restrict__ bottom,
    const __hip_bfloat16* __restrict__ packed,
    const int* __restrict__ perm, __hip_bfloat16* __restrict__ out, int64_t B,
    int F, int D, int out_w, int tri_n, int64_t sb, int64_t sp) {
  extern __shared__ short lds_all[];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int tid = threadIdx.x;
  const int ldst = D + 8;
  short* lds = lds_all + wave * FMAX * ldst;
  const int d8 = D / 8;

  for (int64_t b0 = (int64_t)blockIdx.x * WPB; b0 < B;
       b0 += (int64_t)gridDim.x * WPB) {
    for (int i = tid; i < FMAX * WPB * d8; i += WPB * WAVE) {
      const int row = i / (WPB * d8);
      const int rem = i % (WPB * d8);
      const int w = rem / d8;
      const int col = (rem % d8) * 8;
      const int64_t b = b0 + w;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (b < B) {
        if (row == 0) {
          v = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const short*>(bottom) + b * (int64_t)D + col);
        } else if (row < F) {
          v = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const short*>(packed) +
              ((int64_t)perm[row - 1] * sp + b * sb) * (int64_t)D + col);
        }
      }
      *reinterpret_cast<bf16x8*>(
          &lds_all[w * FMAX * ldst + row * ldst + col]) = v;
    }
    __syncthreads();

    const int64_t b = b0 + wave;
    if (b < B) {
      gram_tril_scatter<FMAX>(lds, ldst, D, F, out + b * (int64_t)out_w, lane);
      short* orow_s = reinterpret_cast<short*>(out + b * (int64_t)out_w);
      for (int c = lane; c < D; c += WAVE) {
        orow_s[tri_n + c] = lds[c];
      }
      for (int c = tri_n + D + lane; c < out_w; c += WAVE) {
        orow_s[c] = 0;
      }
    }
    __syncthreads();
  }
}

// PackedIO over 64 rows: the same chunk mapping, 64 / RPI passes.  The
// write-back goes in groups of 8 passes to bound the registers it holds.
template <int D, int WPB>
struct PackedIO64 {
  static constexpr int D8 = D / 8;
  static constexpr int RPI = WAVE / D8;  // rows per pass
  static constexpr int NIT = 64 / RPI;   // passes = 16-B chunks per thread
  int r0, w, col;
  int64_t b;         // this thread's sample
  int64_t off[NIT];  // element offset of its chunk of pass `it` in bottom
                     // (row 0) or packed

  __device__ __forceinline__ PackedIO64(const int* __restrict__ perm, int F,
                                        int64_t b0, int64_t sb, int64_t sp) {
    const int tid = threadIdx.x;
    r0 = tid / (WPB * D8);
    w = (tid / D8) % WPB;
    col = (tid % D8) * 8;
    b = b0 + w;
    int prow[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      // clamped index, not a branch (F >= 33 here)
      const int row = it * RPI + r0;
      const int pi = row < 1 ? 0 : (row < F ? row - 1 : F - 2);
      prow[it] = perm[pi];
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * RPI + r0;
      off[it] = row == 0 ? b * D + col
                         : (prow[it] * sp + b * sb) * (int64_t)D + col;
    }
    // one wait for perm, ahead of every predicated load (see PackedIO)
#pragma unroll
    for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(off[it]));
  }

  // global -> LDS image [w][64][LD] (+ PER_WAVE between samples), rows >= F
  // and samples >= B zero-filled
  template <int LD, int PER_WAVE, bool SWZ>
  __device__ __forceinline__ void load(const short* __restrict__ bottom,
                                       const short* __restrict__ packed,
                                       short* lds_all, int64_t B, int F) const {
    bf16x8 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * RPI + r0;
      const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      v[it] = z;
      if (b < B && row < F) {
        v[it] = *reinterpret_cast<const bf16x8*>(
            (row == 0 ? bottom : packed) + off[it]);
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * RPI + r0;
      const int at_lds = SWZ ? swz<D>(row, col) : row * LD + col;
      *reinterpret_cast<bf16x8*>(&lds_all[w * PER_WAVE + at_lds]) = v[it];
    }
  }

  // swizzled LDS image -> global, rows < F of samples < B
  template <int PER_WAVE>
  __device__ __forceinline__ void store(const short* lds_all, short* gbottom,
                                        short* gpacked, int64_t B,
                                        int F) const {
    constexpr int G = NIT < 8 ? NIT : 8;
#pragma unroll
    for (int it0 = 0; it0 < NIT; it0 += G) {
      bf16x8 v[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int row = (it0 + g) * RPI + r0;
        v[g] = *reinterpret_cast<const bf16x8*>(
            &lds_all[w * PER_WAVE + swz<D>(row, col)]);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int row = (it0 + g) * RPI + r0;
        if (b < B && row < F) {
          *reinterpret_cast<bf16x8*>((row == 0 ? gbottom : gpacked) +
                                     off[it0 + g]) = v[g];
        }
      }
    }
  }
};

// Forward, compile-time width.  As dot_interact_fwd_packed: padded rows, all
// products in registers before the output row is assembled in the dead rows
// 1.. of the image (<= 2016 + D + 7 of its 63 * LD elements), 16-B stores
// through a 2-byte-aligned type.
template <int D, int WPB>
__global__ __launch_bounds__(WPB* WAVE) void dot_interact_fwd_packed64(
    const __hip_bfloat16* __restrict__ bottom,
    const __hip_bfloat16* __restrict__ packed,
    const int* __restrict__ perm, __hip_bfloat16* __restrict__ out, int64_t B,
    int F, int out_w, int tri_n, int64_t sb, int64_t sp) {
  extern __shared__ short lds_all[];
  constexpr int LD = D + 8;
  constexpr int PER_WAVE = 64 * LD;
  constexpr int NK = D / 32;
  static_assert(2016 + D + 7 <= 63 * LD, "output row staging");
  static_assert((size_t)WPB * PER_WAVE * sizeof(short) <= DI64_LDS_MAX, "LDS");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (WAVE - 1);
  short* lds = lds_all + wave * PER_WAVE;
  const int64_t b0 = (int64_t)blockIdx.x * WPB;
  const PackedIO64<D, WPB> io(perm, F, b0, sb, sp);
  io.template load<LD, PER_WAVE, false>(
      reinterpret_cast<const short*>(bottom),
      reinterpret_cast<const short*>(packed), lds_all, B, F);
  __syncthreads();

  const int64_t b = b0 + wave;
  if (b >= B) return;  // no barrier below
  const int r16 = lane & 15;
  const int khalf = lane >> 4;
  f32x4 accs[10];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    if (mi * 16 < F) {  // wave-uniform: F is a kernel argument
      bf16x8 a[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        a[k] = *reinterpret_cast<const bf16x8*>(
            &lds[(mi * 16 + r16) * LD + k * 32 + khalf * 8]);
      }
#pragma unroll
      for (int ni = 0; ni <= mi; ++ni) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const bf16x8 bfr =
              ni == mi ? a[k]
                       : *reinterpret_cast<const bf16x8*>(
                             &lds[(ni * 16 + r16) * LD + k * 32 + khalf * 8]);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[k], bfr, acc, 0, 0, 0);
        }
        accs[mi * (mi + 1) / 2 + ni] = acc;
      }
    }
  }
  wave_lds_fence();
  short* stage = lds + LD;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    if (mi * 16 < F) {
#pragma unroll
      for (int ni = 0; ni <= mi; ++ni) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = mi * 16 + khalf * 4 + reg;
          const int j = ni * 16 + r16;
          if (i > j && i < F) {
            stage[i * (i - 1) / 2 + j] =
                f32_to_bf16_bits(accs[mi * (mi + 1) / 2 + ni][reg]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = lane; c < D; c += WAVE) stage[tri_n + c] = lds[c];
  const int width = tri_n + D;
  const int width8 = (width + 7) & ~7;
  if (width + lane < width8) stage[width + lane] = 0;
  wave_lds_fence();

  short* orow = reinterpret_cast<short*>(out) + b * (int64_t)out_w;
  const int nfull = out_w >> 3;  // whole 16-B chunks of the row
  for (int c = lane; c < nfull; c += WAVE) {
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c * 8 < width8) v = *reinterpret_cast<const bf16x8*>(&stage[c * 8]);
    *reinterpret_cast<bf16x8_u*>(&orow[c * 8]) = v;
  }
  const int e = nfull * 8 + lane;  // the row's last out_w % 8 elements
  if (e < out_w) orow[e] = e < width ? stage[e] : (short)0;
}

// Backward, compile-time width.  As dot_interact_bwd_packed (transposed
// product, X^T through ds_read_b64_tr_b16 under an all-ones EXEC, swizzled
// image, gradient in place), with two k-steps and up to four feature tiles.
// The gout row lands in the 8 KB that held G_sym: tril chunks at [0, 2016 + 7),
// the bottom part again at [4096 - D, 4096); the eight G fragments of a lane
// are gathered from it once and kept in registers.
template <int D, int WPB>
__global__ __launch_bounds__(WPB* WAVE) void dot_interact_bwd_packed64(
    const __hip_bfloat16* __restrict__ gout,
    const __hip_bfloat16* __restrict__ bottom,
    const __hip_bfloat16* __restrict__ packed, const int* __restrict__ perm,
    __hip_bfloat16* __restrict__ gbottom, __hip_bfloat16* __restrict__ gpacked,
    int64_t B, int F, int out_w, int tri_n, int64_t sb, int64_t sp) {
  static_assert(2016 + 7 + D <= 4096, "gout row staging needs D <= 256");
  extern __shared__ short lds_all[];
  constexpr int PER_WAVE = 64 * D + 4096;
  constexpr int D8 = D / 8;
  constexpr int NJ = D / 16;
  static_assert((size_t)WPB * PER_WAVE * sizeof(short) <= DI64_LDS_MAX, "LDS");
  using IO = PackedIO64<D, WPB>;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (WAVE - 1);
  short* lds = lds_all + wave * PER_WAVE;
  short* stage = lds + 64 * D;
  short* gb = stage + 4096 - D;
  const int64_t b0 = (int64_t)blockIdx.x * WPB;
  const IO io(perm, F, b0, sb, sp);

  // the sample's gout row goes out ahead of the feature loads
  const int64_t b = b0 + wave;
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 vt[4] = {z, z, z, z};
  bf16x8 vb = z;
  if (b < B) {
    const short* grow = reinterpret_cast<const short*>(gout) +
                        b * (int64_t)out_w;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      // a chunk may run up to 7 elements into the bottom part, never past
      // the row: D >= 32
      const int c = (p * WAVE + lane) * 8;
      if (c < tri_n) vt[p] = *reinterpret_cast<const bf16x8_u*>(&grow[c]);
    }
    if (lane < D8) {
      vb = *reinterpret_cast<const bf16x8_u*>(&grow[tri_n + lane * 8]);
    }
  }
  io.template load<D, PER_WAVE, true>(
      reinterpret_cast<const short*>(bottom),
      reinterpret_cast<const short*>(packed), lds_all, B, F);
  if (b < B) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int c = (p * WAVE + lane) * 8;
      if (c < tri_n) *reinterpret_cast<bf16x8*>(&stage[c]) = vt[p];
    }
    if (lane < D8) *reinterpret_cast<bf16x8*>(&gb[lane * 8]) = vb;
  }
  __syncthreads();

  if (b < B) {  // wave-uniform: `wave` is in an SGPR
    const int r16 = lane & 15;
    const int khalf = lane >> 4;
    // g[ni][ks]: B operand G[k][i], i = ni*16 + r16, k = ks*32 + khalf*8 + j
    bf16x8 g[4][2];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = ni * 16 + r16, k = ks * 32 + khalf * 8 + j;
          const bool ok = i < F && k < F && i != k;
          const int r = i > k ? i : k, c = i > k ? k : i;
          const short s = stage[ok ? r * (r - 1) / 2 + c : 0];
          g[ni][ks][j] = ok ? s : (short)0;
        }
      }
    }
    const int xrow = khalf * 8 + (r16 >> 2), xcol = (lane & 3) * 4;
    // NJB column tiles at a time: all their X^T operands (both k-steps) are
    // read before the first of their results is stored, and a result only
    // overwrites columns that no later tile reads
    constexpr int NJB = NJ < 4 ? NJ : 4;
#pragma unroll
    for (int nj0 = 0; nj0 < NJ; nj0 += NJB) {
      bf16x8 a[NJB][2];
      bf16x4 gbv[NJB];
#pragma unroll
      for (int t = 0; t < NJB; ++t) {
        const int d0 = (nj0 + t) * 16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const v4i16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_v4i16_t*)(lds + swz<D>(ks * 32 + xrow, d0 + xcol)));
          const v4i16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_v4i16_t*)(lds + swz<D>(ks * 32 + xrow + 4, d0 + xcol)));
          a[t][ks] =
              bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
        gbv[t] = *reinterpret_cast<const bf16x4*>(&gb[d0 + khalf * 4]);
      }
      wave_lds_fence();
#pragma unroll
      for (int t = 0; t < NJB; ++t) {
        const int d0 = (nj0 + t) * 16;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          if (ni * 16 < F) {  // wave-uniform; rows >= F are never written back
            // bottom-concat gradient of feature 0: the C operand of its column
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (ni == 0 && r16 == 0) {
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                acc[reg] = bf16_bits_to_f32(gbv[t][reg]);
              }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][ks], g[ni][ks],
                                                            acc, 0, 0, 0);
            }
            const bf16x4 o = {
                f32_to_bf16_bits(acc[0]), f32_to_bf16_bits(acc[1]),
                f32_to_bf16_bits(acc[2]), f32_to_bf16_bits(acc[3])};
            *reinterpret_cast<bf16x4*>(
                &lds[swz<D>(ni * 16 + r16, d0 + khalf * 4)]) = o;
          }
        }
      }
      wave_lds_fence();
    }
  }
  __syncthreads();

  // cooperative write-back: the load's mapping, LDS reads ahead of stores
  io.template store<PER_WAVE>(lds_all, reinterpret_cast<short*>(gbottom),
                              reinterpret_cast<short*>(gpacked), B, F);
}

// Samples per block on this path: DE_DI_WPB (1, 2, 4; 8 counts as 4) or the
// measured default, then the largest of {4, 2, 1} not above it whose block
// stays within DI64_LDS_MAX.  One sample always fits (D <= 256).
static int di_wpb64(size_t per_wave_bytes, int dflt) {
  static int env = [] {
    const char* e = getenv("DE_DI_WPB");
    const int i = e ? atoi(e) : 0;
    return (i == 1 || i == 2 || i == 4 || i == 8) ? i : 0;
  }();
  int w = env ? env : dflt;
  if (w > 4) w = 4;
  while (w > 1 && (size_t)w * per_wave_bytes > DI64_LDS_MAX) w >>= 1;
  return w;
}

static void di64_check(int F, int D) {
  if (F <= 32 || F > 64 || D % 32 != 0 || D < 32 || D > 256) {
    throw std::invalid_argument(
        "dot_interact 64-row kernels: 33 <= F <= 64, D % 32 == 0, D <= 256");
  }
}

#define DI64_FOR_WPB(M) \
  if (wpb == 1) { M(1); } else if (wpb == 2) { M(2); } else { M(4); }

// Measured defaults (DI_SWEEP=1 tools/bench_interact.py --features 40 / 64,
// profiles/interact_latency.md), all admissible: D = 128 admits 1 and 2 both
// ways, D = 64 also 4.  Every other width runs the run-time-D kernels,
// measured at D = 96; the clamp in di_wpb64 lowers their 2 to 1 where the
// backward block would not fit (D >= 224).
static int di64_wpb_default(bool fwd, int D) {
  if (D == 128) return 1;
  if (D == 64) return fwd ? 2 : 4;
  return fwd ? 1 : 2;
}

template <int D, int W>
static void launch_fwd_packed64_dw(const void* bottom, const void* packed,
                                   const int* perm, void* out, int64_t B,
                                   int F, int out_w, int tri_n, int64_t sb,
                                   int64_t sp, int blocks,
                                   hipStream_t stream) {
  constexpr size_t lds = (size_t)W * 64 * (D + 8) * sizeof(short);
  if constexpr (lds <= DI64_LDS_MAX) {
    hipLaunchKernelGGL((dot_interact_fwd_packed64<D, W>), dim3(blocks),
                       dim3(W * WAVE), lds, stream,
                       (const __hip_bfloat16*)bottom,
                       (const __hip_bfloat16*)packed, perm,
                       (__hip_bfloat16*)out, B, F, out_w, tri_n, sb, sp);
  } else {
    throw std::logic_error("dot_interact: samples per block over the LDS limit");
  }
}

template <int D, int W>
static void launch_bwd_packed64_dw(const void* gout, const void* bottom,
                                   const void* packed, const int* perm,
                                   void* gbottom, void* gpacked, int64_t B,
                                   int F, int out_w, int tri_n, int64_t sb,
                                   int64_t sp, int blocks,
                                   hipStream_t stream) {
  constexpr size_t lds = (size_t)W * (64 * D + 64 * 64) * sizeof(short);
  if constexpr (lds <= DI64_LDS_MAX) {
    hipLaunchKernelGGL((dot_interact_bwd_packed64<D, W>), dim3(blocks),
                       dim3(W * WAVE), lds, stream,
                       (const __hip_bfloat16*)gout,
                       (const __hip_bfloat16*)bottom,
                       (const __hip_bfloat16*)packed, perm,
                       (__hip_bfloat16*)gbottom, (__hip_bfloat16*)gpacked, B,
                       F, out_w, tri_n, sb, sp);
  } else {
    throw std::logic_error("dot_interact: samples per block over the LDS limit");
  }
}

void launch_dot_interact_fwd_packed64(const void* bottom, const void* packed,
                                      const int* perm, void* out, int64_t B,
                                      int F, int D, int out_w, int tri_n,
                                      int64_t sb, int64_t sp,
                                      hipStream_t stream) {
  di64_check(F, D);
  if (B == 0) return;
  const size_t per_wave = (size_t)64 * (D + 8) * sizeof(short);
  const int wpb = di_wpb64(per_wave, di64_wpb_default(true, D));
  const int64_t groups = (B + wpb - 1) / wpb;
  int blocks = (int)groups;
  if (groups <= INT32_MAX) {  // one block per sample group
#define LFWD_D(DD, W)                                                         \
  launch_fwd_packed64_dw<DD, W>(bottom, packed, perm, out, B, F, out_w,       \
                                tri_n, sb, sp, blocks, stream)
#define LFWD128(W) LFWD_D(128, W)
#define LFWD64(W) LFWD_D(64, W)
    if (D == 128) { DI64_FOR_WPB(LFWD128) return; }
    if (D == 64) { DI64_FOR_WPB(LFWD64) return; }
#undef LFWD64
#undef LFWD128
#undef LFWD_D
  }
  if (groups > 32768) blocks = 32768;  // grid-stride kernel
  const size_t lds = (size_t)wpb * per_wave;
#define LFWD(W)                                                                \
  hipLaunchKernelGGL((dot_interact_fwd_packed_rt_tiles<64, W>), dim3(blocks),  \
                     dim3(W * WAVE), lds, stream,                              \
                     (const __hip_bfloat16*)bottom,                            \
                     (const __hip_bfloat16*)packed, perm, (__hip_bfloat16*)out,\
                     B, F, D, out_w, tri_n, sb, sp)
  DI64_FOR_WPB(LFWD)
#undef LFWD
}

void launch_dot_interact_bwd_packed64(const void* gout, const void* bottom,
                                      const void* packed, const int* perm,
                                      void* gbottom, void* gpacked, int64_t B,
                                      int F, int D, int out_w, int tri_n,
                                      int64_t sb, int64_t sp,
                                      hipStream_t stream) {
  di64_check(F, D);
  if (B == 0) return;
  const size_t per_wave = (size_t)(64 * D + 64 * 64) * sizeof(short);
  const int wpb = di_wpb64(per_wave, di64_wpb_default(false, D));
  const int64_t groups = (B + wpb - 1) / wpb;
  int blocks = (int)groups;
  if (groups <= INT32_MAX) {  // one block per sample group
#define LBWD_D(DD, W)                                                         \
  launch_bwd_packed64_dw<DD, W>(gout, bottom, packed, perm, gbottom, gpacked, \
                                B, F, out_w, tri_n, sb, sp, blocks, stream)
#define LBWD128(W) LBWD_D(128, W)
#define LBWD64(W) LBWD_D(64, W)
    if (D == 128) { DI64_FOR_WPB(LBWD128) return; }
    if (D == 64) { DI64_FOR_WPB(LBWD64) return; }
#undef LBWD64
#undef LBWD128
#undef LBWD_D
  }
  if (groups > 32768) blocks = 32768;  // grid-stride kernel
  const size_t lds = (size_t)wpb * per_wave;
#define LBWD(W)                                                                \
  hipLaunchKernelGGL((dot_interact_bwd_packed_rt<64, W>), dim3(blocks),        \
                     dim3(W * WAVE), lds, stream, (const __hip_bfloat16*)gout, \
                     (const __hip_bfloat16*)bottom,                            \
                     (const __hip_bfloat16*)packed, perm,                      \
                     (__hip_bfloat16*)gbottom, (__hip_bfloat16*)gpacked, B, F, \
                     D, out_w, tri_n, sb, sp)
  DI64_FOR_WPB(LBWD)
#undef LBWD
}
#undef DI64_FOR_WPB

// stacked [B, F, D] layout: waves per block from the same LDS limit
static int di64_waves(size_t per_wave_bytes) {
  int w = 4;
  while (w > 1 && (size_t)w * per_wave_bytes > DI64_LDS_MAX) w >>= 1;
  return w;
}

void launch_dot_interact_fwd64(const void* feats, void* out, int64_t B, int F,
                               int D, int out_w, int tri_n,
                               hipStream_t stream) {
  di64_check(F, D);
  if (B == 0) return;
  const size_t per_wave = (size_t)64 * (D + 8) * sizeof(short);
  const int waves = di64_waves(per_wave);
  int64_t blocks = (B + waves - 1) / waves;
  if (blocks > 32768) blocks = 32768;
  hipLaunchKernelGGL((dot_interact_fwd_tiles<64>), dim3((int)blocks),
                     dim3(waves * WAVE), waves * per_wave, stream,
                     (const __hip_bfloat16*)feats, (__hip_bfloat16*)out, B, F,
                     D, out_w, tri_n);
}

void launch_dot_interact_bwd64(const void* gout, const void* feats,
                               void* gfeats, int64_t B, int F, int D,
                               int out_w, int tri_n, hipStream_t stream) {
  di64_check(F, D);
  if (B == 0) return;
  const size_t per_wave = (size_t)(64 * D + 64 * 64) * sizeof(short);
  const int waves = di64_waves(per_wave);
  int64_t blocks = (B + waves - 1) / waves;
  if (blocks > 32768) blocks = 32768;
  hipLaunchKernelGGL((dot_interact_bwd<64>), dim3((int)blocks),
                     dim3(waves * WAVE), waves * per_wave, stream,
                     (const __hip_bfloat16*)gout,
                     (const __hip_bfloat16*)feats, (__hip_bfloat16*)gfeats, B,
                     F, D, out_w, tri_n);
}
