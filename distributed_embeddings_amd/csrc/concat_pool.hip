// Fused concat + average pool of the synthetic models' interaction (gfx950).
//
//   X [B, W]   = the inputs [B, w_t] side by side (never materialised)
//   out[b, o]  = (sum of X[b, o*S .. min((o+1)*S, W))) / (columns in the window)
//                for o < Wp = ceil(W / S)
//   out[b, Wp + n] = numerical[b, n]
//
// and the backward gin_t[b, j] = gout[b, (begin_t + j) / S] / cnt.  This is
// cat + AvgPool1d(S, stride=S, ceil_mode=True) + cat in one pass over the
// inputs: fp32 sums in ascending column order, one fp32 division, one
// round-to-nearest-even store.  No atomics; every output element has one
// writer.
//
// Work split.  A block owns a tile of CP_ROWS consecutive samples x a span of
// OC output columns, i.e. OC*S concatenated columns [c0, c1).  Spans start at
// multiples of S, so no window straddles two blocks.  OC = min(64, CAP / S)
// (rounded down to a multiple of 8 when above 8) keeps the span inside an LDS
// row of CAP = 1024 bytes / sizeof(T) columns, whatever the stride.
// blockIdx.y selects the span, so everything about the span, the descriptor
// search included, is wave-uniform scalar work; blockIdx.x strides over the
// sample tiles.
//
// Forward.  Input t is contiguous [B, w_t], so its rows of one sample tile
// are one contiguous run of CP_ROWS * w_t elements, read with 16-byte loads
// by consecutive lanes whatever w_t is.  The block's four waves take the
// inputs that overlap the span in turn; a wave keeps CP_UNROLL 16-byte loads
// per lane in flight before the first LDS write, and stores them into the
// image [CP_ROWS][pitch] in the input's storage type at the element's
// concatenated column (minus the span's 16-byte-aligned origin).  Every w_t is
// a multiple of the 16-byte chunk, so chunks are aligned in the concatenated
// column index; a chunk that straddles a span edge is loaded whole by both
// neighbours and each reads its own elements of it.  After one barrier a
// thread forms eight adjacent windows of one sample from LDS and writes them
// with one (bf16) or two (fp32) 16-byte stores through a 2- or 4-byte aligned
// vector type, as dot_interact.hip does: an output row of Wp + Nn columns is
// not 16-byte aligned in general.  A span's last, short group goes out as
// scalar stores.  The block that owns the last span copies the tile's
// numerical columns.
//
// Backward.  Same tiling.  The gout[rows, OC] tile is read, divided by the
// window length in fp32, rounded once to the gradient type and kept as an
// LDS image [CP_ROWS][64 + pad].  The waves then walk the same inputs and
// chunks as the forward and assemble 16-byte chunks of gin_t (element c is
// image column c / S - span origin), stored to the address the forward loaded
// from.  A chunk on a span edge is written element by element by each of the
// two blocks, its own elements only.
//
// LDS banks (derived, no counter run).  64 banks of 4 bytes.  The forward
// image's pitch is 1072 bytes = 268 dwords = 12 mod 64 for both types, so
// the 16-byte staging stores of sixteen lanes that hold one chunk of sixteen
// consecutive rows (a width-8 bf16 input) start at banks 0, 12, 24, ... , 52:
// sixteen disjoint groups of four banks.  Lanes that hold consecutive chunks
// of one row are conflict-free trivially.  The window reads are element reads
// at 8*S elements between the lanes of one row and 268 dwords between rows;
// they conflict a few ways for most S.  That is accepted: a tile reads each
// staged element once, about 56 reads per thread at S = 7, against 28 KB of
// global loads per tile.
//
// Descriptors {pointer, begin column, width} travel by value in the kernel
// arguments, as in pack_ids.hip: no descriptor tensor, no copy, capturable.
// A launch carries kConcatPoolMaxInputs of them; the host splits the spans
// into ranges whose inputs fit, an input on a border going into both.

#include <hip/hip_runtime.h>

#include <stdexcept>

#include "ops_api.h"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_WAVES = CP_THREADS / 64;
constexpr int CP_ROWS = 32;
constexpr int CP_MAX_OC = 64;
constexpr int CP_GROUP = 8;        // adjacent windows per thread
constexpr int CP_UNROLL = 4;       // 16-byte loads in flight per lane
constexpr int CP_ROW_BYTES = 1024; // span columns of one image row
constexpr int CP_PITCH_BYTES = CP_ROW_BYTES + 2 * 16 + 16;  // 1072
constexpr int CP_MAX_BLOCKS_X = 1024;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef u16x8 __attribute__((aligned(2))) u16x8_u;
typedef f32x4 __attribute__((aligned(4))) f32x4_u;

struct ConcatPoolArgs {
  ConcatPoolInput in[kConcatPoolMaxInputs];
};

struct ConcatPoolShape {
  int64_t B;
  int32_t W;           // concatenated width
  int32_t S;           // stride = window
  int32_t Wp;          // ceil(W / S)
  int32_t Nn;          // numerical columns
  int32_t OC;          // output columns per span
  int32_t span_first;  // span of blockIdx.y == 0
  int32_t nin;         // descriptors of this launch
  int32_t num_bf16;
};
static_assert(sizeof(ConcatPoolArgs) + sizeof(ConcatPoolShape) + 32 <= 4096 - 256,
              "concat_pool argument block must stay under 4 KB");

__device__ __forceinline__ float to_float(unsigned short v) {
  return __uint_as_float((unsigned)v << 16);
}
__device__ __forceinline__ float to_float(float v) { return v; }

__device__ __forceinline__ unsigned short f2bf_rne(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
template <typename T> __device__ __forceinline__ T from_float(float f);
template <> __device__ __forceinline__ float from_float<float>(float f) { return f; }
template <> __device__ __forceinline__ unsigned short from_float<unsigned short>(float f) {
  return f2bf_rne(f);
}

// Index of the last descriptor whose begin is <= c (begins ascend, in[0].begin
// <= c by the host's choice of the launch's inputs).
__device__ __forceinline__ int first_input(const ConcatPoolArgs& a, int nin, int c) {
  int lo = 0, hi = nin - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.in[mid].begin <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The span of this block: output columns [o0, o0 + ocs), concatenated columns
// [c0, c1), image origin img0 = c0 rounded down to a chunk.
struct Span {
  int o0, ocs, c0, c1;
};
__device__ __forceinline__ Span block_span(const ConcatPoolShape& p) {
  Span s;
  s.o0 = (p.span_first + (int)blockIdx.y) * p.OC;
  s.ocs = p.Wp - s.o0 < p.OC ? p.Wp - s.o0 : p.OC;
  s.c0 = s.o0 * p.S;
  const int c1 = s.c0 + s.ocs * p.S;
  s.c1 = c1 < p.W ? c1 : p.W;
  return s;
}

template <typename T, typename OT>
__global__ __launch_bounds__(CP_THREADS) void concat_pool_fwd_kernel(
    ConcatPoolArgs a, ConcatPoolShape p, const void* __restrict__ numerical,
    OT* __restrict__ out) {
  constexpr int CH = 16 / (int)sizeof(T);
  constexpr int PITCH = CP_PITCH_BYTES / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) T img[CP_ROWS * PITCH];

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const Span sp = block_span(p);
  const int S = p.S;
  const int OW = p.Wp + p.Nn;
  const int img0 = sp.c0 & ~(CH - 1);
  const int t0 = first_input(a, p.nin, sp.c0);
  const int groups = (sp.ocs + CP_GROUP - 1) / CP_GROUP;
  const bool last_span = sp.c1 == p.W;

  const int64_t tiles = (p.B + CP_ROWS - 1) / CP_ROWS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t b0 = tile * CP_ROWS;
    const int rows = (int)(p.B - b0 < CP_ROWS ? p.B - b0 : CP_ROWS);

    for (int t = t0 + wave; t < p.nin; t += CP_WAVES) {
      const int begin = a.in[t].begin;
      if (begin >= sp.c1) break;
      const int width = a.in[t].width;
      const T* __restrict__ src =
          static_cast<const T*>(a.in[t].ptr) + b0 * width;
      const int lo = begin > img0 ? begin : img0;
      const int hi = begin + width < sp.c1 ? begin + width : sp.c1;
      const int k0 = (lo - begin) / CH;
      const int nk = (hi - begin + CH - 1) / CH - k0;
      const int n = rows * nk;
      const int col0 = begin - img0;  // image column of the input's column 0
      for (int i0 = 0; i0 < n; i0 += 64 * CP_UNROLL) {
        u32x4 v[CP_UNROLL];
        int at[CP_UNROLL];
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u) {
          const int i = i0 + u * 64 + lane;
          at[u] = -1;
          if (i < n) {
            const int r = i / nk;
            const int k = k0 + (i - r * nk);
            v[u] = *reinterpret_cast<const u32x4*>(src + r * width + k * CH);
            at[u] = r * PITCH + col0 + k * CH;
          }
        }
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u)
          if (at[u] >= 0) *reinterpret_cast<u32x4*>(img + at[u]) = v[u];
      }
    }
    __syncthreads();

    const int ntask = rows * groups;
    for (int i = threadIdx.x; i < ntask; i += CP_THREADS) {
      const int r = i / groups;
      const int ol = (i - r * groups) * CP_GROUP;
      const int nvalid = sp.ocs - ol < CP_GROUP ? sp.ocs - ol : CP_GROUP;
      const T* __restrict__ win = img + r * PITCH + (sp.c0 - img0) + ol * S;
      OT res[CP_GROUP];
#pragma unroll
      for (int j = 0; j < CP_GROUP; ++j) {
        res[j] = from_float<OT>(0.f);
        if (j < nvalid) {
          const int left = p.W - (sp.c0 + (ol + j) * S);
          const int cnt = left < S ? left : S;
          float sum = 0.f;
          for (int s = 0; s < cnt; ++s) sum += to_float(win[j * S + s]);
          res[j] = from_float<OT>(sum / (float)cnt);
        }
      }
      OT* __restrict__ dst = out + (b0 + r) * OW + sp.o0 + ol;
      if (nvalid == CP_GROUP) {
        if constexpr (sizeof(OT) == 2) {
          u16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = res[j];
          *reinterpret_cast<u16x8_u*>(dst) = o;
        } else {
          f32x4 o0 = {res[0], res[1], res[2], res[3]};
          f32x4 o1 = {res[4], res[5], res[6], res[7]};
          *reinterpret_cast<f32x4_u*>(dst) = o0;
          *reinterpret_cast<f32x4_u*>(dst + 4) = o1;
        }
      } else {
#pragma unroll
        for (int j = 0; j < CP_GROUP; ++j)
          if (j < nvalid) dst[j] = res[j];
      }
    }

    if (last_span && p.Nn > 0) {
      const int n = rows * p.Nn;
      for (int i = threadIdx.x; i < n; i += CP_THREADS) {
        const int r = i / p.Nn;
        const int c = i - r * p.Nn;
        const int64_t at = (b0 + r) * p.Nn + c;
        const float v = p.num_bf16
            ? to_float(static_cast<const unsigned short*>(numerical)[at])
            : static_cast<const float*>(numerical)[at];
        out[(b0 + r) * OW + p.Wp + c] = from_float<OT>(v);
      }
    }
    __syncthreads();  // the next tile's staging overwrites the image
  }
}

template <typename T, typename GT>
__global__ __launch_bounds__(CP_THREADS) void concat_pool_bwd_kernel(
    ConcatPoolArgs a, ConcatPoolShape p, const GT* __restrict__ gout) {
  constexpr int CH = 16 / (int)sizeof(T);
  // 33 (bf16) or 65 (fp32) dwords: consecutive rows shift by one bank
  constexpr int PITCH = CP_MAX_OC + 4 / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) T img[CP_ROWS * PITCH];

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const Span sp = block_span(p);
  const unsigned S = (unsigned)p.S;
  const int OW = p.Wp + p.Nn;
  const int img0 = sp.c0 & ~(CH - 1);
  const int t0 = first_input(a, p.nin, sp.c0);

  const int64_t tiles = (p.B + CP_ROWS - 1) / CP_ROWS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t b0 = tile * CP_ROWS;
    const int rows = (int)(p.B - b0 < CP_ROWS ? p.B - b0 : CP_ROWS);

    const int nload = rows * sp.ocs;
    for (int i = threadIdx.x; i < nload; i += CP_THREADS) {
      const int r = i / sp.ocs;
      const int o = i - r * sp.ocs;
      const int left = p.W - (sp.c0 + o * (int)S);
      const int cnt = left < (int)S ? left : (int)S;
      const float g = to_float(gout[(b0 + r) * OW + sp.o0 + o]);
      img[r * PITCH + o] = from_float<T>(g / (float)cnt);
    }
    __syncthreads();

    for (int t = t0 + wave; t < p.nin; t += CP_WAVES) {
      const int begin = a.in[t].begin;
      if (begin >= sp.c1) break;
      const int width = a.in[t].width;
      T* __restrict__ dst = static_cast<T*>(a.in[t].ptr) + b0 * width;
      const int lo = begin > img0 ? begin : img0;
      const int hi = begin + width < sp.c1 ? begin + width : sp.c1;
      const int k0 = (lo - begin) / CH;
      const int nk = (hi - begin + CH - 1) / CH - k0;
      const int n = rows * nk;
      for (int i = lane; i < n; i += 64) {
        const int r = i / nk;
        const int k = k0 + (i - r * nk);
        const int cs = begin + k * CH;  // concatenated column of element 0
        // window of the chunk's first own element, then walk
        const int cf = cs > sp.c0 ? cs : sp.c0;
        unsigned q = (unsigned)cf / S;
        unsigned rem = (unsigned)cf - q * S;
        q -= (unsigned)sp.o0;
        const T* __restrict__ row = img + r * PITCH;
        T* __restrict__ d = dst + r * width + k * CH;
        if (cs >= sp.c0 && cs + CH <= sp.c1) {
          __attribute__((aligned(16))) T vals[CH];
#pragma unroll
          for (int e = 0; e < CH; ++e) {
            vals[e] = row[q];
            if (++rem == S) { rem = 0; ++q; }
          }
          *reinterpret_cast<u32x4*>(d) = *reinterpret_cast<const u32x4*>(vals);
        } else {
#pragma unroll
          for (int e = 0; e < CH; ++e) {
            const int c = cs + e;
            if (c >= sp.c0 && c < sp.c1) {
              d[e] = row[q];
              if (++rem == S) { rem = 0; ++q; }
            }
          }
        }
      }
    }
    __syncthreads();  // the next tile's loads overwrite the image
  }
}

int span_columns(int S, bool in_bf16) {
  const int cap = CP_ROW_BYTES / (in_bf16 ? 2 : 4);
  int oc = cap / S;
  if (oc > CP_MAX_OC) oc = CP_MAX_OC;
  if (oc > CP_GROUP) oc &= ~(CP_GROUP - 1);
  return oc;
}

// Calls launch(args, shape, spans) for consecutive span ranges whose
// overlapping inputs fit one argument block.
template <typename F>
void for_each_launch(const ConcatPoolInput* in, int nin, bool in_bf16,
                     int Nn, int64_t B, int W, int S, bool num_bf16,
                     F&& launch) {
  if (nin < 1 || W < 1 || B < 0 || Nn < 0)
    throw std::invalid_argument("concat_pool: bad shape");
  if (S < 1 || S > kConcatPoolMaxStride)
    throw std::invalid_argument("concat_pool: stride out of range");
  const int ch = in_bf16 ? 8 : 4;
  int at = 0;
  for (int t = 0; t < nin; ++t) {
    if (in[t].begin != at || in[t].width < ch || in[t].width % ch != 0)
      throw std::invalid_argument("concat_pool: bad input descriptor");
    at += in[t].width;
  }
  if (at != W) throw std::invalid_argument("concat_pool: widths do not add up");
  if (B == 0) return;

  ConcatPoolShape p{};
  p.B = B;
  p.W = W;
  p.S = S;
  p.Wp = (int)(((int64_t)W + S - 1) / S);
  p.Nn = Nn;
  p.OC = span_columns(S, in_bf16);
  p.num_bf16 = num_bf16 ? 1 : 0;
  const int nspans = (p.Wp + p.OC - 1) / p.OC;
  const int64_t span_cols = (int64_t)p.OC * S;
  const int64_t tiles = (B + CP_ROWS - 1) / CP_ROWS;
  const unsigned bx =
      (unsigned)(tiles < CP_MAX_BLOCKS_X ? tiles : CP_MAX_BLOCKS_X);

  int first = 0;  // first input that reaches into span s
  for (int s = 0; s < nspans;) {
    while ((int64_t)in[first].begin + in[first].width <= s * span_cols) ++first;
    // widen [s, e) while its inputs [first, last] fit; a span is at most
    // 1024 bytes of columns, so one span always fits
    int e = s, last = first;
    while (e < nspans && e - s < 65535) {
      int64_t c1 = (e + 1) * span_cols;
      if (c1 > W) c1 = W;
      int l = last;
      while (l + 1 < nin && in[l + 1].begin < c1) ++l;
      if (l - first + 1 > kConcatPoolMaxInputs) break;
      last = l;
      ++e;
    }
    ConcatPoolArgs args{};
    for (int t = first; t <= last; ++t) args.in[t - first] = in[t];
    p.span_first = s;
    p.nin = last - first + 1;
    launch(args, p, dim3(bx, (unsigned)(e - s)));
    s = e;
  }
}

}  // namespace

void launch_concat_pool_fwd(const ConcatPoolInput* in, int nin, bool in_bf16,
                            const void* numerical, bool num_bf16, int Nn,
                            void* out, bool out_bf16, int64_t B, int W, int S,
                            hipStream_t stream) {
  for_each_launch(in, nin, in_bf16, Nn, B, W, S, num_bf16,
                  [&](const ConcatPoolArgs& args, const ConcatPoolShape& p,
                      dim3 grid) {
    const dim3 block(CP_THREADS);
    if (in_bf16 && out_bf16)
      hipLaunchKernelGGL((concat_pool_fwd_kernel<unsigned short, unsigned short>),
                         grid, block, 0, stream, args, p, numerical,
                         (unsigned short*)out);
    else if (in_bf16)
      hipLaunchKernelGGL((concat_pool_fwd_kernel<unsigned short, float>), grid,
                         block, 0, stream, args, p, numerical, (float*)out);
    else if (out_bf16)
      hipLaunchKernelGGL((concat_pool_fwd_kernel<float, unsigned short>), grid,
                         block, 0, stream, args, p, numerical,
                         (unsigned short*)out);
    else
      hipLaunchKernelGGL((concat_pool_fwd_kernel<float, float>), grid, block,
                         0, stream, args, p, numerical, (float*)out);
  });
}

void launch_concat_pool_bwd(const void* gout, bool gout_bf16,
                            const ConcatPoolInput* gin, int nin, bool in_bf16,
                            int Nn, int64_t B, int W, int S,
                            hipStream_t stream) {
  for_each_launch(gin, nin, in_bf16, Nn, B, W, S, false,
                  [&](const ConcatPoolArgs& args, const ConcatPoolShape& p,
                      dim3 grid) {
    const dim3 block(CP_THREADS);
    if (in_bf16 && gout_bf16)
      hipLaunchKernelGGL((concat_pool_bwd_kernel<unsigned short, unsigned short>),
                         grid, block, 0, stream, args, p,
                         (const unsigned short*)gout);
    else if (in_bf16)
      hipLaunchKernelGGL((concat_pool_bwd_kernel<unsigned short, float>), grid,
                         block, 0, stream, args, p, (const float*)gout);
    else if (gout_bf16)
      hipLaunchKernelGGL((concat_pool_bwd_kernel<float, unsigned short>), grid,
                         block, 0, stream, args, p,
                         (const unsigned short*)gout);
    else
      hipLaunchKernelGGL((concat_pool_bwd_kernel<float, float>), grid, block,
                         0, stream, args, p, (const float*)gout);
  });
}
