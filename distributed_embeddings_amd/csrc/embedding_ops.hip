// CDNA4 (gfx950 / MI355X) kernels for distributed_embeddings_amd.
//
// Hand-written HIP implementations of the reference's native op set
// (capabilities of the reference's cc/kernels/embedding_lookup_kernels.cu,
// re-designed for 64-wide wavefronts, LDS and HBM3E — not a port):
//
//   * csr_lookup_forward  — CSR segmented gather-reduce (K1-K3 equivalent).
//     Wave64 tiling: width<=64 uses sub-wave tiles (64/TILE rows per wave),
//     width>64 uses one wave per row with per-lane vectorized float4/float2
//     loads; widths >256 loop over 256-element chunks.  Grid-stride over rows.
//     Power-law skew: rows longer than an adaptive threshold are pushed to a
//     device-side list, expanded to exact (row, 128-id chunk) work items, and
//     reduced by a second kernel with atomic combine (no host sync).  The
//     opt-in deterministic mode stores the chunk partials to a slab and adds
//     them in a fixed order instead: no float atomics in the forward, the
//     sparse backward or the fused optimizers.
//   * csr_lookup_forward_q8 / quantize_rows / dequantize_rows — the same
//     forward from int8 row-wise quantized tables (width bytes + fp32 scale +
//     fp32 bias per row, inference only): the wide and long kernels above
//     instantiated on q8_t, plus the device-side quantizer and its inverse.
//   * csr_lookup_forward_q4 / quantize_rows_q4 / dequantize_rows_q4 — the
//     same again for int4 row-wise tables in FBGEMM's fused 4-bit layout
//     (width / 2 bytes of nibbles + fp16 scale + fp16 bias per row), on q4_t.
//   * row_to_split        — COO rows -> CSR splits by per-row binary search
//     (K4 equivalent).
//   * csr_lookup_backward — rowid expansion + packed (id<<32|pos) keys-only
//     radix sort (hand-written, radix_sort.hip; rocPRIM via
//     DE_USE_ROCPRIM_SORT=1) + head-flag scan unique + segmented sum reusing
//     the forward kernels with per-id weights (K5-K7 equivalent).
//   * csr_lookup_weight_grad — gradient of the per-id weights of a weighted
//     lookup (the forward's per_id_w): one lane group per id, no atomics.
//   * csr_fused_optimizer_apply — the same pipeline with the SGD, Adagrad or
//     row-wise Adagrad update applied in place (no host sync;
//     hipGraph-capturable).  bf16 tables can take the update with stochastic
//     rounding: counter-based bits per table element, step counter on the
//     device (stochastic_round_bf16 is the same rounding as an op).
//   * integer_lookup     — open-addressing (linear probe) int64 hash
//     resident in torch buffers; two-kernel design (free-slot scan, then
//     insert_and_find with device-scope 64-bit atomicCAS) replacing the
//     reference's cooperative cuCollections kernel (K8-K9 equivalent).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>
#include <cstring>
#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "ops_api.h"

#define WAVE 64

// ---------------------------------------------------------------------------
// Param dtype abstraction: tables are fp32 or bf16 (storage); all arithmetic
// accumulates in fp32.  bf16 load = bit-shift; store = RNE via __hip_bfloat16.
// ---------------------------------------------------------------------------
struct bf16_t { unsigned short b; };

__device__ __forceinline__ float pt_load(const float* p) { return *p; }
__device__ __forceinline__ float pt_load(const bf16_t* p) {
  union { unsigned int u; float f; } c;
  c.u = ((unsigned int)p->b) << 16;
  return c.f;
}
__device__ __forceinline__ void pt_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void pt_store(bf16_t* p, float v) {
  __hip_bfloat16 h(v);
  p->b = *reinterpret_cast<unsigned short*>(&h);
}
// vectorized row loads: 4 contiguous elements starting at p (aligned)
__device__ __forceinline__ void pt_load4(const float* p, float* o) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void pt_load4(const bf16_t* p, float* o) {
  const short4 v = *reinterpret_cast<const short4*>(p);
  union { unsigned int u; float f; } c;
  c.u = ((unsigned int)(unsigned short)v.x) << 16; o[0] = c.f;
  c.u = ((unsigned int)(unsigned short)v.y) << 16; o[1] = c.f;
  c.u = ((unsigned int)(unsigned short)v.z) << 16; o[2] = c.f;
  c.u = ((unsigned int)(unsigned short)v.w) << 16; o[3] = c.f;
}
__device__ __forceinline__ void pt_load2(const float* p, float* o) {
  const float2 v = *reinterpret_cast<const float2*>(p);
  o[0] = v.x; o[1] = v.y;
}
__device__ __forceinline__ void pt_load2(const bf16_t* p, float* o) {
  const short2 v = *reinterpret_cast<const short2*>(p);
  union { unsigned int u; float f; } c;
  c.u = ((unsigned int)(unsigned short)v.x) << 16; o[0] = c.f;
  c.u = ((unsigned int)(unsigned short)v.y) << 16; o[1] = c.f;
}
// vectorized stores (RNE for bf16): 4/2 contiguous elements
__device__ __forceinline__ void pt_store4(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void pt_store4(bf16_t* p, const float* v) {
  short4 s;
  __hip_bfloat16 h0(v[0]), h1(v[1]), h2(v[2]), h3(v[3]);
  s.x = *reinterpret_cast<short*>(&h0);
  s.y = *reinterpret_cast<short*>(&h1);
  s.z = *reinterpret_cast<short*>(&h2);
  s.w = *reinterpret_cast<short*>(&h3);
  *reinterpret_cast<short4*>(p) = s;
}
__device__ __forceinline__ void pt_store2(float* p, const float* v) {
  *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
}
__device__ __forceinline__ void pt_store2(bf16_t* p, const float* v) {
  short2 s;
  __hip_bfloat16 h0(v[0]), h1(v[1]);
  s.x = *reinterpret_cast<short*>(&h0);
  s.y = *reinterpret_cast<short*>(&h1);
  *reinterpret_cast<short2*>(p) = s;
}
// 8 contiguous elements (int4 tables): two 16-B stores of fp32, one of bf16
__device__ __forceinline__ void pt_store8(float* p, const float* v) {
  pt_store4(p, v);
  pt_store4(p + 4, v + 4);
}
__device__ __forceinline__ void pt_store8(bf16_t* p, const float* v) {
  unsigned int d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    __hip_bfloat16 lo(v[2 * j]), hi(v[2 * j + 1]);
    d[j] = (unsigned int)*reinterpret_cast<unsigned short*>(&lo) |
           ((unsigned int)*reinterpret_cast<unsigned short*>(&hi) << 16);
  }
  *reinterpret_cast<uint4*>(p) = make_uint4(d[0], d[1], d[2], d[3]);
}
// VEC (4, 2 or 1) contiguous elements with the widest matching access
template <int VEC, typename T>
__device__ __forceinline__ void pt_loadv(const T* p, float* o) {
  if constexpr (VEC == 4) pt_load4(p, o);
  else if constexpr (VEC == 2) pt_load2(p, o);
  else o[0] = pt_load(p);
}
// stores also take VEC == 8
template <int VEC, typename T>
__device__ __forceinline__ void pt_storev(T* p, const float* v) {
  if constexpr (VEC == 8) pt_store8(p, v);
  else if constexpr (VEC == 4) pt_store4(p, v);
  else if constexpr (VEC == 2) pt_store2(p, v);
  else pt_store(p, v[0]);
}

// ---------------------------------------------------------------------------
// Stochastic rounding of fp32 to bf16 (optimizer writes to bf16 tables only).
//
// A finite x with bit pattern u and 16 random bits r is stored as
// (u + r) >> 16: away from zero with probability low16(u) / 65536, unbiased,
// and a bf16-representable x never moves.  Above the largest finite bf16 the
// result may be +-inf, as with RNE.  Inf and NaN take the RNE path: adding r
// to a NaN payload can carry into the sign bit.
//
// r is a function of (seed, step, o) alone, o = row * width + col being the
// element's offset in the local table -- not of the thread, tile or kernel:
//   key = mix64(seed ^ mix64(step))
//   h   = mix64(key + (o >> 2))
//   r   = (h >> (16 * (o & 3))) & 0xFFFF
// so one 64-bit hash serves an aligned group of four elements.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t k) {
  // splitmix64 finalizer
  k += 0x9E3779B97F4A7C15ull;
  k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
  k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
  return k ^ (k >> 31);
}

__device__ __forceinline__ uint64_t sr_key(uint64_t seed, uint64_t step) {
  return mix64(seed ^ mix64(step));
}
// the 64 bits shared by the four elements o & ~3 .. o | 3
__device__ __forceinline__ uint64_t sr_hash(uint64_t key, int64_t o) {
  return mix64(key + ((uint64_t)o >> 2));
}
__device__ __forceinline__ unsigned int sr_pick(uint64_t h, int64_t o) {
  return (unsigned int)(h >> (16 * (int)(o & 3))) & 0xFFFFu;
}
__device__ __forceinline__ unsigned int sr_bits(uint64_t seed, uint64_t step,
                                                int64_t o) {
  return sr_pick(sr_hash(sr_key(seed, step), o), o);
}

__device__ __forceinline__ unsigned short bf16_rne_bits(float v) {
  __hip_bfloat16 h(v);
  return *reinterpret_cast<unsigned short*>(&h);
}
__device__ __forceinline__ unsigned short bf16_sr_bits(float v,
                                                       unsigned int r) {
  union { float f; unsigned int u; } c;
  c.f = v;
  if ((c.u & 0x7F800000u) == 0x7F800000u) return bf16_rne_bits(v);
  return (unsigned short)((c.u + r) >> 16);  // finite: no carry past bit 31
}

// What a kernel keeps of the {seed, step} pair.  Rounding is a template flag
// of the update kernels (SR, instantiated for bf16 tables only): `on` is a
// compile-time constant after inlining, so an SR = false kernel is the
// nearest-even kernel, instruction for instruction, and reads no pair.
struct SrState {
  uint64_t key;
  bool on;
};
template <bool SR>
__device__ __forceinline__ SrState sr_load(const int64_t* __restrict__ sr) {
  if constexpr (SR) return {sr_key((uint64_t)sr[0], (uint64_t)sr[1]), true};
  else return {0, false};
}

// The hash of o's group of four when rounding is on (0 otherwise), for
// callers that store several elements of one group.
__device__ __forceinline__ uint64_t sr_group_hash(SrState sr, int64_t o) {
  return sr.on ? sr_hash(sr.key, o) : 0;
}

// Optimizer stores: element o of the table gets v.  fp32 stores v; bf16
// rounds stochastically when sr.on and to nearest-even otherwise.  The
// scalar store takes h = sr_group_hash(sr, o).
__device__ __forceinline__ void pt_store_sr(float* p, float v, SrState,
                                            uint64_t, int64_t) {
  *p = v;
}
__device__ __forceinline__ void pt_store_sr(bf16_t* p, float v, SrState sr,
                                            uint64_t h, int64_t o) {
  p->b = sr.on ? bf16_sr_bits(v, sr_pick(h, o)) : bf16_rne_bits(v);
}
// o is a multiple of 2: both elements share one hash
__device__ __forceinline__ void pt_store2_sr(float* p, const float* v, SrState,
                                             int64_t) {
  pt_store2(p, v);
}
__device__ __forceinline__ void pt_store2_sr(bf16_t* p, const float* v,
                                             SrState sr, int64_t o) {
  if (!sr.on) {
    pt_store2(p, v);
    return;
  }
  const uint64_t h = sr_hash(sr.key, o);
  short2 s;
  s.x = (short)bf16_sr_bits(v[0], sr_pick(h, o));
  s.y = (short)bf16_sr_bits(v[1], sr_pick(h, o + 1));
  *reinterpret_cast<short2*>(p) = s;
}
// o is a multiple of 4: the hash's four 16-bit fields in order
__device__ __forceinline__ void pt_store4_sr(float* p, const float* v, SrState,
                                             int64_t) {
  pt_store4(p, v);
}
__device__ __forceinline__ void pt_store4_sr(bf16_t* p, const float* v,
                                             SrState sr, int64_t o) {
  if (!sr.on) {
    pt_store4(p, v);
    return;
  }
  const uint64_t h = sr_hash(sr.key, o);
  short4 s;
  s.x = (short)bf16_sr_bits(v[0], (unsigned int)h & 0xFFFFu);
  s.y = (short)bf16_sr_bits(v[1], (unsigned int)(h >> 16) & 0xFFFFu);
  s.z = (short)bf16_sr_bits(v[2], (unsigned int)(h >> 32) & 0xFFFFu);
  s.w = (short)bf16_sr_bits(v[3], (unsigned int)(h >> 48));
  *reinterpret_cast<short4*>(p) = s;
}
template <int VEC, typename T>
__device__ __forceinline__ void pt_storev_sr(T* p, const float* v, SrState sr,
                                             int64_t o) {
  if constexpr (VEC == 4) pt_store4_sr(p, v, sr, o);
  else if constexpr (VEC == 2) pt_store2_sr(p, v, sr, o);
  else pt_store_sr(p, v[0], sr, sr_group_hash(sr, o), o);
}

static inline int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// Device helpers shared by the forward, backward and fused-update kernels.
// ---------------------------------------------------------------------------

// Where the calling lane's wave sits in a 1-D grid of wave64 blocks.
struct WaveCoord {
  int lane;
  int64_t wave_id, n_waves;
};
__device__ __forceinline__ WaveCoord wave_coord() {
  return {(int)(threadIdx.x & (WAVE - 1)),
          ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6,
          ((int64_t)gridDim.x * blockDim.x) >> 6};
}

// Sub-wave tiling: `tile` (pow2 <= WAVE) lanes own one work item, so a wave
// holds rpw items and lane = sub * tile + tl.  Narrow kernels pass the
// compile-time TILE, wide kernels the runtime tile_w; kernels that give a
// whole wave to each item pass WAVE.
struct TileCoord {
  int rpw, sub, tl;
};
__device__ __forceinline__ TileCoord tile_coord(int lane, int tile) {
  return {WAVE / tile, lane / tile, lane % tile};
}

// Wide gather-accumulate: acc[v] = sum over k in [ks, ke) of
// w[k] * src[idx[k]][col0 + v], in k order.  The dispatch only picks a VEC
// that divides width and col0 is a multiple of VEC, so col0 < width means
// all VEC columns are inside the row.  CHECK skips ids outside [0, vocab).
template <int VEC, bool HAS_W, bool CHECK, typename ST>
__device__ __forceinline__ void wide_accumulate(
    const ST* __restrict__ src, const int64_t* __restrict__ idx,
    const float* __restrict__ w, int64_t vocab, int width, int col0,
    int64_t ks, int64_t ke, float* acc /* size VEC */) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
  for (int64_t k = ks; k < ke; ++k) {
    const int64_t i = idx[k];
    if (CHECK && (i < 0 || i >= vocab)) continue;
    const float wk = HAS_W ? w[k] : 1.f;
    float r[VEC];
    pt_loadv<VEC>(src + i * (int64_t)width + col0, r);
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] += wk * r[v];
  }
}

// int8 row-wise quantized rows (inference tables): a row of the packed
// [vocab, width + 8] byte table is width bytes q, then fp32 scale, then fp32
// bias, and stands for scale * q[c] + bias.  width % 4 == 0, so the row
// stride is a multiple of 4 and every dword below is aligned.
struct q8_t { unsigned char b; };

#define Q8_TAIL 8  // bytes of scale + bias behind the quantized columns

__device__ __forceinline__ const unsigned char* q8_row(const q8_t* src,
                                                       int64_t i, int width) {
  return reinterpret_cast<const unsigned char*>(src) +
         i * (int64_t)(width + Q8_TAIL);
}
__device__ __forceinline__ unsigned int q8_load4(const unsigned char* row,
                                                 int col0) {
  return *reinterpret_cast<const unsigned int*>(row + col0);
}
__device__ __forceinline__ float q8_scale(const unsigned char* row, int width) {
  return *reinterpret_cast<const float*>(row + width);
}
__device__ __forceinline__ float q8_bias(const unsigned char* row, int width) {
  return *reinterpret_cast<const float*>(row + width + 4);
}
// byte v of a dword of four quantized columns, as a float (0..255, exact)
__device__ __forceinline__ float q8_byte(unsigned int q, int v) {
  return (float)((q >> (8 * v)) & 0xffu);
}

// The quantized wide gather-accumulate: same contract as wide_accumulate
// above with `width` the logical width, one dword (VEC == 4 columns) per lane.
// The bias is factored out of the column sum,
//   acc[v] = sum_k (w_k * scale_k) * q_k[v]  +  sum_k w_k * bias_k,
// so a term costs one FMA per column.  An id outside [0, vocab) is skipped in
// BOTH sums: its loads are pointed at row 0 (the launcher guarantees
// vocab > 0) and its two coefficients are zeroed, which keeps the loop
// branch-free.  Four independent id -> row chains are in flight; terms join
// the sums in k order.
template <int VEC, bool HAS_W, bool CHECK>
__device__ __forceinline__ void wide_accumulate(
    const q8_t* __restrict__ src, const int64_t* __restrict__ idx,
    const float* __restrict__ w, int64_t vocab, int width, int col0,
    int64_t ks, int64_t ke, float* acc /* size VEC */) {
  static_assert(VEC == 4, "a quantized lane owns one dword of columns");
  constexpr int UNROLL = 4;
  float aq[VEC] = {0.f, 0.f, 0.f, 0.f};
  float ab = 0.f;
  int64_t k = ks;
  for (; k + UNROLL <= ke; k += UNROLL) {
    int64_t i[UNROLL];
    bool ok[UNROLL];
    unsigned int q[UNROLL];
    float sc[UNROLL], bi[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) i[u] = idx[k + u];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      ok[u] = !CHECK || (i[u] >= 0 && i[u] < vocab);
      const unsigned char* row = q8_row(src, ok[u] ? i[u] : 0, width);
      q[u] = q8_load4(row, col0);
      sc[u] = q8_scale(row, width);
      bi[u] = q8_bias(row, width);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const float wk = HAS_W ? w[k + u] : 1.f;
      const float ws = ok[u] ? wk * sc[u] : 0.f;
      ab += ok[u] ? wk * bi[u] : 0.f;
#pragma unroll
      for (int v = 0; v < VEC; ++v) aq[v] += ws * q8_byte(q[u], v);
    }
  }
  for (; k < ke; ++k) {
    const int64_t i = idx[k];
    const bool ok = !CHECK || (i >= 0 && i < vocab);
    const unsigned char* row = q8_row(src, ok ? i : 0, width);
    // all three loads before the selects: a load inside a `?:` arm becomes
    // a branch of its own, and one-hot lookups live in this loop
    const unsigned int q = q8_load4(row, col0);
    const float sc = q8_scale(row, width), bi = q8_bias(row, width);
    const float wk = HAS_W ? w[k] : 1.f;
    const float ws = ok ? wk * sc : 0.f;
    ab += ok ? wk * bi : 0.f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) aq[v] += ws * q8_byte(q, v);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = aq[v] + ab;
}

// int4 row-wise quantized rows (inference tables): a row of the packed
// [vocab, width / 2 + 4] byte table is width / 2 bytes of nibbles (column 2j
// in the low nibble of byte j, column 2j + 1 in the high one), then fp16
// scale, then fp16 bias, and stands for scale * q[c] + bias.  width % 8 == 0,
// so a lane's dword is eight whole columns — column col0 + v is bits
// [4v, 4v + 4) — and the row stride and the scale/bias dword are 4-byte
// aligned.
struct q4_t { unsigned char b; };

#define Q4_TAIL 4  // bytes of scale + bias behind the nibbles

__device__ __forceinline__ const unsigned char* q4_row(const q4_t* src,
                                                       int64_t i, int width) {
  return reinterpret_cast<const unsigned char*>(src) +
         i * (int64_t)(width / 2 + Q4_TAIL);
}
__device__ __forceinline__ unsigned int q4_load8(const unsigned char* row,
                                                 int col0) {
  return *reinterpret_cast<const unsigned int*>(row + col0 / 2);
}
// scale (low half) and bias (high half) as stored: one dword
__device__ __forceinline__ unsigned int q4_tail(const unsigned char* row,
                                                int width) {
  return *reinterpret_cast<const unsigned int*>(row + width / 2);
}
__device__ __forceinline__ float half_bits_to_float(unsigned int h) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}
__device__ __forceinline__ float q4_scale(unsigned int tail) {
  return half_bits_to_float(tail & 0xffffu);
}
__device__ __forceinline__ float q4_bias(unsigned int tail) {
  return half_bits_to_float(tail >> 16);
}
// the eight columns of a dword as floats (0..15, exact): the even columns
// are the bytes of q & 0x0f0f0f0f, the odd ones those of (q >> 4) & ...
__device__ __forceinline__ void q4_unpack8(unsigned int q, float* f) {
  const unsigned int even = q & 0x0f0f0f0fu, odd = (q >> 4) & 0x0f0f0f0fu;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = (float)((even >> (8 * j)) & 0xffu);
    f[2 * j + 1] = (float)((odd >> (8 * j)) & 0xffu);
  }
}

// The int4 wide gather-accumulate: the int8 overload's shape with one dword
// of eight columns (VEC == 8) per lane and scale and bias from one dword —
// bias factored out of the column sum, an id outside [0, vocab) pointed at
// row 0 with both coefficients zeroed (the launcher guarantees vocab > 0),
// four id -> row chains in flight, terms added in k order, fp32 throughout.
template <int VEC, bool HAS_W, bool CHECK>
__device__ __forceinline__ void wide_accumulate(
    const q4_t* __restrict__ src, const int64_t* __restrict__ idx,
    const float* __restrict__ w, int64_t vocab, int width, int col0,
    int64_t ks, int64_t ke, float* acc /* size VEC */) {
  static_assert(VEC == 8, "an int4 lane owns one dword of eight columns");
  constexpr int UNROLL = 4;
  float aq[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) aq[v] = 0.f;
  float ab = 0.f;
  int64_t k = ks;
  for (; k + UNROLL <= ke; k += UNROLL) {
    int64_t i[UNROLL];
    bool ok[UNROLL];
    unsigned int q[UNROLL], tail[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) i[u] = idx[k + u];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      ok[u] = !CHECK || (i[u] >= 0 && i[u] < vocab);
      const unsigned char* row = q4_row(src, ok[u] ? i[u] : 0, width);
      q[u] = q4_load8(row, col0);
      tail[u] = q4_tail(row, width);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const float wk = HAS_W ? w[k + u] : 1.f;
      const float ws = ok[u] ? wk * q4_scale(tail[u]) : 0.f;
      ab += ok[u] ? wk * q4_bias(tail[u]) : 0.f;
      float f[VEC];
      q4_unpack8(q[u], f);
#pragma unroll
      for (int v = 0; v < VEC; ++v) aq[v] += ws * f[v];
    }
  }
  for (; k < ke; ++k) {
    const int64_t i = idx[k];
    const bool ok = !CHECK || (i >= 0 && i < vocab);
    const unsigned char* row = q4_row(src, ok ? i : 0, width);
    // both loads before the selects, as in the int8 overload
    const unsigned int q = q4_load8(row, col0);
    const unsigned int tail = q4_tail(row, width);
    const float wk = HAS_W ? w[k] : 1.f;
    const float ws = ok ? wk * q4_scale(tail) : 0.f;
    ab += ok ? wk * q4_bias(tail) : 0.f;
    float f[VEC];
    q4_unpack8(q, f);
#pragma unroll
    for (int v = 0; v < VEC; ++v) aq[v] += ws * f[v];
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = aq[v] + ab;
}

// Narrow strided reduce: lane column tl = lane % TILE sums
// w[k] * src[idx[k]][tl] over k = k0, k0 + KSTRIDE, ... < ke.
//   KSTRIDE == 1: each TILE-lane sub-tile owns its own segment, k0 = ks.
//   KSTRIDE == WAVE/TILE: the wave's sub-tiles share one segment
//     (k0 = ks + sub) and a shuffle fold leaves the total on sub-tile 0.
// UNROLL (pow2) terms are loaded at once and added as a pairwise tree —
// (t0+t1)+(t2+t3) for 4, t0+t1 for 2 — before joining the running sum; the
// summation order is part of each caller's bit-exact contract.
template <int TILE, int KSTRIDE, int UNROLL, bool HAS_W, bool CHECK,
          typename ST>
__device__ __forceinline__ float narrow_reduce(
    const ST* __restrict__ src, const int64_t* __restrict__ idx,
    const float* __restrict__ w, int64_t vocab, int width, int64_t ks,
    int64_t ke, int lane) {
  static_assert(KSTRIDE == 1 || KSTRIDE == WAVE / TILE, "bad k-stride");
  const int tl = lane % TILE;
  auto oob = [&](int64_t i) { return CHECK && (i < 0 || i >= vocab); };
  auto term = [&](int64_t k, int64_t i) {
    return (HAS_W ? w[k] : 1.f) * pt_load(&src[i * (int64_t)width + tl]);
  };
  float acc = 0.f;
  if (tl < width) {
    int64_t k = ks + (KSTRIDE > 1 ? lane / TILE : 0);
    // UNROLL independent idx->row load chains in flight
    for (; k + (UNROLL - 1) * KSTRIDE < ke; k += UNROLL * KSTRIDE) {
      int64_t i[UNROLL];
      float t[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) i[u] = idx[k + u * KSTRIDE];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        t[u] = oob(i[u]) ? 0.f : term(k + u * KSTRIDE, i[u]);
#pragma unroll
      for (int s = 1; s < UNROLL; s *= 2) {
#pragma unroll
        for (int u = 0; u < UNROLL; u += 2 * s) t[u] += t[u + s];
      }
      acc += t[0];
    }
    for (; k < ke; k += KSTRIDE) {
      const int64_t i = idx[k];
      if (!oob(i)) acc += term(k, i);
    }
  }
  if constexpr (KSTRIDE > 1) {
#pragma unroll
    for (int off = WAVE / 2; off >= TILE; off >>= 1)
      acc += __shfl_down(acc, off);
  }
  return acc;
}

// Update rule of the element-wise kernels, a template parameter.
enum : int { RULE_SGD = 0, RULE_ADAGRAD = 1, RULE_ADAM = 2 };

// Lazy Adam's constants.  Its state is m [vocab, width] followed by v
// [vocab, width]: the kernels get m's base and v_off = vocab * width.
// omb = 1 - b, rounded once from double on the host.  The other rules carry
// the struct unread.
struct AdamArgs {
  float b1, b2, omb1, omb2;
  int64_t v_off;
};

// SGD: w -= lr * g.   Adagrad: s += g^2; w -= lr * g / (sqrt(s) + eps).
// Lazy Adam: m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
//            w -= a_t * m / (sqrt(v) + eps), where the caller passes
//            a_t = lr * sqrt(1 - b2^t) / (1 - b1^t) as lr (adam_advance_step).

// Lazy Adam on registers: updates m and v and returns the new weight.  Both
// sums are fmas by name in either rounding mode, for the reason given in
// row_update_value: m and v are the nearest-even run's bit for bit.
__device__ __forceinline__ float adam_value(float w, float& m, float& v,
                                            float g, float a_t, float eps,
                                            const AdamArgs& ad) {
  m = __builtin_fmaf(ad.b1, m, ad.omb1 * g);
  v = __builtin_fmaf(ad.b2, v, ad.omb2 * (g * g));
  return w - a_t * m / (sqrtf(v) + eps);
}

// The new value of a weight w (fp32) and, for Adagrad and Adam, the state
// update; state points at the element's s, or at its m.
template <int RULE>
__device__ __forceinline__ float row_update_value(float w, float* state,
                                                  float g, float lr, float eps,
                                                  bool rounding,
                                                  const AdamArgs& ad) {
  if constexpr (RULE == RULE_ADAM) {
    float m = state[0], v = state[ad.v_off];
    w = adam_value(w, m, v, g, lr, eps, ad);
    state[0] = m;
    state[ad.v_off] = v;
    return w;
  }
  if (RULE == RULE_ADAGRAD) {
    // The nearest-even kernels contract this sum to one fma.  The rounding
    // kernels ask for it by name: their wide VEC = 2 instantiation otherwise
    // came out as a packed multiply and a packed add, and the state differed
    // from the nearest-even run's in the last bit.  Rounding is to touch the
    // weights only.
    const float st = rounding ? __builtin_fmaf(g, g, *state) : *state + g * g;
    *state = st;
    return w - lr * g / (sqrtf(st) + eps);
  }
  return w - lr * g;
}

// w is element o of the table and h = sr_group_hash(sr, o): they pick the
// stochastic-rounding bits of a bf16 store.
template <int RULE, typename PT>
__device__ __forceinline__ void apply_row_update(PT* w, float* state, float g,
                                                 float lr, float eps,
                                                 SrState sr, uint64_t h,
                                                 int64_t o,
                                                 const AdamArgs& ad) {
  pt_store_sr(w,
              row_update_value<RULE>(pt_load(w), state, g, lr, eps, sr.on, ad),
              sr, h, o);
}

// Row-wise Adagrad: one fp32 accumulator per row,
//   s += mean_c(g[c]^2);  w[c] -= lr * g[c] / (sqrt(s) + eps).
// The helpers below are the pieces its three kernels share.

// Sum of v over the `tile` (pow2 <= WAVE) lanes of the caller's lane group.
// The xor butterfly never leaves the group and every lane of the group ends
// with the same bits, so every lane of the group has to call it.
__device__ __forceinline__ float tile_sum(float v, int tile) {
  for (int off = tile >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Adds the group's mean square to state[0] and returns sqrt(new state) + eps
// to every lane of the `tile`-lane group.  Only the group's first lane of a
// `live` group touches memory; the others get the new value by shuffle, so
// every lane of the group has to call this as well.
__device__ __forceinline__ float rowwise_denom(float* state, float ssq,
                                               int width, int lane, int tile,
                                               bool live, float eps) {
  const int leader = lane & ~(tile - 1);
  float st = 0.f;
  if (live && lane == leader) {
    st = *state + ssq / (float)width;
    *state = st;
  }
  st = __shfl(st, leader);
  return sqrtf(st) + eps;
}

// One wave applies one row whose summed gradient g[0..width) sits in memory
// nobody writes during the kernel (the optimizer step's grad rows, the
// finalize kernel's completed scratch rows): squares first, update second.
// row0 is the table offset of w[0].
template <typename PT>
__device__ __forceinline__ void rowwise_wave_update(
    PT* __restrict__ w, float* __restrict__ state, const float* __restrict__ g,
    int width, int lane, float lr, float eps, SrState sr, int64_t row0) {
  float ssq = 0.f;
  for (int c = lane; c < width; c += WAVE) ssq += g[c] * g[c];
  ssq = tile_sum(ssq, WAVE);
  const float denom = rowwise_denom(state, ssq, width, lane, WAVE, true, eps);
  for (int c = lane; c < width; c += WAVE) {
    const int64_t o = row0 + c;
    pt_store_sr(&w[c], pt_load(&w[c]) - lr * g[c] / denom, sr,
                sr_group_hash(sr, o), o);
  }
}

// ---------------------------------------------------------------------------
// Forward: CSR segmented gather-reduce.
// ---------------------------------------------------------------------------

// CSR segmented gather-reduce, two-kernel adaptive design:
//   Kernel A (csr_fwd_*) owns one row per wave (or sub-wave tile).  Rows with
//   segments <= LONG_T reduce in registers and store directly (no atomics).
//   Longer rows (power-law mega-segments, tiny-vocab backward) are zero-
//   filled and pushed to a device-side long-row list.
//   Kernel B (csr_fwd_long) consumes an exact device-built (long row,
//   LONG_T-chunk) work list (expand_long_work), one wave per chunk, and
//   combines partials with atomicAdd.  No host sync, no full-output memset.
// This is the wave64 answer to the reference's blockDim.y reduction
// splitting + round-robin step counter (embedding_lookup_kernels.cu:195-226).
#define LONG_T 128

// Narrow kernel A: width <= 64.  TILE = pow2 >= width; 64/TILE rows per wave.
// OT: output storage type (float, or bf16 when the consumer wants bf16
// directly — saves the separate cast kernel + half the store traffic; the
// long-row path requires fp32 atomics so bf16-out launches disable it).
template <int TILE, bool MEAN, bool HAS_W, typename PT, typename OT>
__global__ void csr_fwd_narrow(const PT* __restrict__ params,
                               const int64_t* __restrict__ values,
                               const int64_t* __restrict__ splits,
                               const float* __restrict__ per_id_w,
                               OT* __restrict__ out, int64_t num_rows,
                               int64_t vocab, int width, int64_t long_thresh,
                               int64_t* __restrict__ long_rows,
                               int32_t* __restrict__ long_count) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, TILE);
  for (int64_t base = wc.wave_id * tc.rpw; base < num_rows;
       base += wc.n_waves * tc.rpw) {
    const int64_t row = base + tc.sub;
    if (row >= num_rows || tc.tl >= width) continue;
    const int64_t s = splits[row], e = splits[row + 1];
    if (e - s > long_thresh) {
      pt_store(&out[row * width + tc.tl], 0.f);
      if (tc.tl == 0) long_rows[atomicAdd(long_count, 1)] = row;
      continue;
    }
    float acc = narrow_reduce<TILE, 1, 4, HAS_W, true>(
        params, values, per_id_w, vocab, width, s, e, wc.lane);
    if (MEAN && e > s) acc /= (float)(e - s);
    pt_store(&out[row * width + tc.tl], acc);
  }
}

// Wide kernel A: width > 64.  tile_w lanes per row, VEC elements per lane:
// a width-128 VEC-4 table runs 2 rows per wave with every lane loading.
template <int VEC, bool MEAN, bool HAS_W, typename PT, typename OT>
__global__ void csr_fwd_wide(const PT* __restrict__ params,
                             const int64_t* __restrict__ values,
                             const int64_t* __restrict__ splits,
                             const float* __restrict__ per_id_w,
                             OT* __restrict__ out, int64_t num_rows,
                             int64_t vocab, int width, int64_t long_thresh,
                             int64_t* __restrict__ long_rows,
                             int32_t* __restrict__ long_count,
                             int tile_w /* pow2 lanes per row, <= WAVE */) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, tile_w);
  for (int64_t base = wc.wave_id * tc.rpw; base < num_rows;
       base += wc.n_waves * tc.rpw) {
    const int64_t row = base + tc.sub;
    if (row >= num_rows) continue;
    const int64_t s = splits[row], e = splits[row + 1];
    if (e - s > long_thresh) {
      for (int c = tc.tl; c < width; c += tile_w)
        pt_store(&out[row * width + c], 0.f);
      if (tc.tl == 0) long_rows[atomicAdd(long_count, 1)] = row;
      continue;
    }
    const float inv = (MEAN && e > s) ? 1.f / (float)(e - s) : 1.f;
    for (int col0 = tc.tl * VEC; col0 < width; col0 += tile_w * VEC) {
      float acc[VEC];
      wide_accumulate<VEC, HAS_W, true>(params, values, per_id_w, vocab, width,
                                        col0, s, e, acc);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] *= inv;
      pt_storev<VEC>(out + row * (int64_t)width + col0, acc);
    }
  }
}

// Builds the exact (long-row, chunk) work list so consumer kernels never
// probe empty chunk slots.  Item encoding: (li << 24) | chunk.  Long row li
// owns the items base .. base + chunks - 1, in chunk order; WITH_BASE
// (deterministic mode) also records work_base[li] = base.  The base comes
// from an integer atomic and may differ between runs: it only names slots.
template <bool WITH_BASE>
__global__ void expand_long_work(const int64_t* __restrict__ long_rows,
                                 const int32_t* __restrict__ long_count,
                                 const int64_t* __restrict__ splits,
                                 int64_t* __restrict__ work_items,
                                 int32_t* __restrict__ n_work,
                                 int32_t* __restrict__ work_base) {
  const WaveCoord wc = wave_coord();
  const int64_t n_long = *long_count;
  for (int64_t li = wc.wave_id; li < n_long; li += wc.n_waves) {
    const int64_t row = long_rows[li];
    const int64_t len = splits[row + 1] - splits[row];
    const int64_t chunks = (len + LONG_T - 1) / LONG_T;
    int base = 0;
    if (wc.lane == 0) {
      base = atomicAdd(n_work, (int32_t)chunks);
      if constexpr (WITH_BASE) work_base[li] = base;
    }
    base = __shfl(base, 0);
    for (int64_t c = wc.lane; c < chunks; c += WAVE) {
      work_items[base + c] = (li << 24) | c;
    }
  }
}

// One decoded work item: ids [ks, ke) of long row `row` = segment [s, e),
// which is entry li of the long-row list.
struct LongChunk {
  int64_t li, row, s, e, ks, ke;
};
__device__ __forceinline__ LongChunk long_chunk(
    const int64_t* __restrict__ work_items,
    const int64_t* __restrict__ long_rows, const int64_t* __restrict__ splits,
    int64_t item) {
  const int64_t w = work_items[item];
  LongChunk c;
  c.li = w >> 24;
  c.row = long_rows[c.li];
  c.s = splits[c.row];
  c.e = splits[c.row + 1];
  c.ks = c.s + (w & 0xffffff) * LONG_T;
  c.ke = min(c.ks + (int64_t)LONG_T, c.e);
  return c;
}

// Kernel B: long rows.  Work item = (long row, LONG_T-chunk).  Narrow
// (TILE > 0): one wave per item, all 64 lanes active — the 64/TILE sub-tiles
// each reduce a strided share of the chunk.  Wide (TILE == 0): tile_w lanes
// per item as in kernel A.  Partials combine with global atomicAdd (out
// pre-zeroed by A).  DET (deterministic mode): `out` is the slab, fp32
// [n_items_max, width], and item `item` stores the value it would have added
// to slab row `item` with plain vector stores; long_slab_group_sum and
// long_slab_combine then add the rows in a fixed order.
template <int TILE, int VEC, bool MEAN, bool HAS_W, bool DET, typename PT>
__global__ void csr_fwd_long(const PT* __restrict__ params,
                             const int64_t* __restrict__ values,
                             const int64_t* __restrict__ splits,
                             const float* __restrict__ per_id_w,
                             float* __restrict__ out, int64_t vocab, int width,
                             const int64_t* __restrict__ long_rows,
                             const int64_t* __restrict__ work_items,
                             const int32_t* __restrict__ n_work_ptr,
                             int tile_w) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, TILE > 0 ? WAVE : tile_w);
  const int64_t n_items = *n_work_ptr;
  for (int64_t ibase = wc.wave_id * tc.rpw; ibase < n_items;
       ibase += wc.n_waves * tc.rpw) {
    const int64_t item = ibase + tc.sub;
    if (item >= n_items) continue;
    const LongChunk c = long_chunk(work_items, long_rows, splits, item);
    if (c.ks >= c.e) continue;
    const float inv = (MEAN && c.e > c.s) ? 1.f / (float)(c.e - c.s) : 1.f;
    float* orow = out + (DET ? item : c.row) * (int64_t)width;
    if constexpr (TILE > 0) {
      const float acc = narrow_reduce<TILE, WAVE / TILE, 4, HAS_W, true>(
          params, values, per_id_w, vocab, width, c.ks, c.ke, wc.lane);
      if (wc.lane < TILE && wc.lane < width) {
        if constexpr (DET) orow[wc.lane] = acc * inv;
        else atomicAdd(&orow[wc.lane], acc * inv);
      }
    } else {
      for (int col0 = tc.tl * VEC; col0 < width; col0 += tile_w * VEC) {
        float acc[VEC];
        wide_accumulate<VEC, HAS_W, true>(params, values, per_id_w, vocab,
                                          width, col0, c.ks, c.ke, acc);
        if constexpr (DET) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] *= inv;
          pt_storev<VEC>(orow + col0, acc);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            atomicAdd(&orow[col0 + v], acc[v] * inv);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Deterministic mode: fixed-order combine of the long rows' slab partials.
//
// Long row li with chunks = ceil(len / LONG_T) owns the slab rows
// base .. base + chunks - 1 (base = work_base[li]), row base + c holding the
// partial p_c of its chunk c.  The row's sum is defined per column as
//   S_g = ((p_{gG} + p_{gG+1}) + ...) + p_{min(gG+G, chunks)-1}
//         for each group g of SLAB_G consecutive chunks, left to right,
//   t   = ((S_0 + S_1) + ...) + S_{ceil(chunks / G) - 1}, left to right,
// all in fp32.  It is a function of the partials and of `chunks` alone --
// not of the grid, the wave, li or base -- and for chunks <= SLAB_G it is the
// plain left-to-right sum.  long_slab_group_sum forms the S_g, one wave per
// group, in place (S_g replaces p_{gG}; a mega-segment of 13k chunks keeps
// 200 waves busy); long_slab_combine adds the S_g of one row and stores.
// Only the adds are ordered: SLAB_FLIGHT loads are in flight ahead of them.
// ---------------------------------------------------------------------------
#define SLAB_G 64
#define SLAB_FLIGHT 8

// p[0] + p[stride] + ... + p[(n - 1) * stride], left to right; n >= 1 and
// wave-uniform.
__device__ __forceinline__ float slab_ordered_sum(const float* p,
                                                  int64_t stride, int64_t n) {
  float t = p[0];
  int64_t j = 1;
  for (; j + SLAB_FLIGHT <= n; j += SLAB_FLIGHT) {
    float v[SLAB_FLIGHT];
#pragma unroll
    for (int u = 0; u < SLAB_FLIGHT; ++u) v[u] = p[(j + u) * stride];
#pragma unroll
    for (int u = 0; u < SLAB_FLIGHT; ++u) t = t + v[u];
  }
  for (; j < n; ++j) t = t + p[j * stride];
  return t;
}

// Level 1: the wave that meets the first item of a group (chunk % SLAB_G ==
// 0) sums the group's slab rows into that first row.  No other wave reads or
// writes the group's rows, and a lane touches its own columns only, so the
// in-place store needs no fence.  Rows of one chunk group of one are left as
// they are.
__global__ void long_slab_group_sum(float* slab, int width,
                                    const int64_t* __restrict__ long_rows,
                                    const int64_t* __restrict__ splits,
                                    const int64_t* __restrict__ work_items,
                                    const int32_t* __restrict__ n_work_ptr) {
  const WaveCoord wc = wave_coord();
  const int64_t n_items = *n_work_ptr;
  for (int64_t item = wc.wave_id; item < n_items; item += wc.n_waves) {
    const int64_t w = work_items[item];
    const int64_t chunk = w & 0xffffff;
    if (chunk % SLAB_G != 0) continue;
    const int64_t row = long_rows[w >> 24];
    const int64_t len = splits[row + 1] - splits[row];
    const int64_t chunks = (len + LONG_T - 1) / LONG_T;
    const int64_t n = min((int64_t)SLAB_G, chunks - chunk);
    if (n < 2) continue;
    float* first = slab + item * (int64_t)width;
    for (int c = wc.lane; c < width; c += WAVE)
      first[c] = slab_ordered_sum(first + c, width, n);
  }
}

// Level 2: one wave per long row adds the row's group sums in group order and
// stores the total -- to out[row] (forward and sparse backward; OT fp32, or
// bf16 rounded to nearest-even), or with TO_SCRATCH to scratch row li, which
// the fused optimizers' finalize kernels then read.
template <bool TO_SCRATCH, typename OT>
__global__ void long_slab_combine(const float* __restrict__ slab,
                                  OT* __restrict__ dst, int width,
                                  const int64_t* __restrict__ long_rows,
                                  const int32_t* __restrict__ long_count,
                                  const int64_t* __restrict__ splits,
                                  const int32_t* __restrict__ work_base) {
  const WaveCoord wc = wave_coord();
  const int64_t n_long = *long_count;
  for (int64_t li = wc.wave_id; li < n_long; li += wc.n_waves) {
    const int64_t row = long_rows[li];
    const int64_t len = splits[row + 1] - splits[row];
    const int64_t chunks = (len + LONG_T - 1) / LONG_T;
    const int64_t groups = (chunks + SLAB_G - 1) / SLAB_G;
    const float* first = slab + (int64_t)work_base[li] * width;
    OT* drow = dst + (TO_SCRATCH ? li : row) * (int64_t)width;
    for (int c = wc.lane; c < width; c += WAVE)
      pt_store(&drow[c], slab_ordered_sum(first + c, (int64_t)SLAB_G * width,
                                          groups));
  }
}

// ---------------------------------------------------------------------------
// Host-side dispatch shared by the forward and fused-update launches.
// ---------------------------------------------------------------------------

static int pick_grid(int64_t work_items, int block_waves) {
  // >> 256 workgroups to fill 8 XCDs x 32 CUs; cap to bound launch cost.
  int64_t blocks = cdiv64(work_items, block_waves);
  if (blocks > 16384) blocks = 16384;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// Lanes per row and waves needed to give `rows` rows one tile each.  Narrow
// (TILE > 0): TILE lanes.  Wide: tile_w = pow2 lanes covering width / VEC.
struct RowTiling {
  int tile_w;
  int64_t row_waves;
};
template <int TILE, int VEC>
static RowTiling row_tiling(int width, int64_t rows) {
  int tile_w = WAVE;
  if constexpr (TILE == 0) {
    tile_w = next_pow2((width + VEC - 1) / VEC);
    if (tile_w > WAVE) tile_w = WAVE;
  }
  return {tile_w, cdiv64(rows, WAVE / (TILE > 0 ? TILE : tile_w))};
}

template <int N>
using Int = std::integral_constant<int, N>;

// Calls f(Int<TILE>, Int<VEC>).  Narrow widths get TILE = pow2 >= width and
// VEC 0; wide ones TILE 0 and the largest VEC of 4, 2, 1 that divides width,
// which is what lets the kernels drop partial-vector handling.
template <typename F>
static void dispatch_width(int width, F&& f) {
  if (width > 64) {
    if (width % 4 == 0) f(Int<0>{}, Int<4>{});
    else if (width % 2 == 0) f(Int<0>{}, Int<2>{});
    else f(Int<0>{}, Int<1>{});
    return;
  }
  switch (next_pow2(width)) {
    case 1: f(Int<1>{}, Int<0>{}); break;
    case 2: f(Int<2>{}, Int<0>{}); break;
    case 4: f(Int<4>{}, Int<0>{}); break;
    case 8: f(Int<8>{}, Int<0>{}); break;
    case 16: f(Int<16>{}, Int<0>{}); break;
    case 32: f(Int<32>{}, Int<0>{}); break;
    default: f(Int<64>{}, Int<0>{}); break;
  }
}

// Calls f(std::true_type) or f(std::false_type).
template <typename F>
static void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// Calls f(Int<RULE>).
template <typename F>
static void dispatch_rule(int rule, F&& f) {
  switch (rule) {
    case RULE_ADAM: f(Int<RULE_ADAM>{}); break;
    case RULE_ADAGRAD: f(Int<RULE_ADAGRAD>{}); break;
    default: f(Int<RULE_SGD>{}); break;
  }
}

// Calls f(std::true_type) for a bf16 table with a {seed, step} pair and
// f(std::false_type) otherwise: fp32 tables get no rounding instantiation.
template <typename PT, typename F>
static void dispatch_sr(const int64_t* sr, F&& f) {
  if constexpr (std::is_same<PT, float>::value) f(std::false_type{});
  else dispatch_bool(sr != nullptr, f);
}

// Storage type selected by a dispatch_bool tag.
template <typename IsBf16>
using storage_t = std::conditional_t<IsBf16::value, bf16_t, float>;

// Adaptive long threshold of the forward: when there are plenty of rows the
// chip is full without splitting, so only true outliers (>4x the average and
// >LONG_T) offload; with few rows split aggressively for parallelism.  bf16
// out: the atomic long-row combine needs fp32, so the split is disabled —
// every row reduces in-register in kernel A (callers request bf16 out only on
// bounded-hotness forwards).  The deterministic combine stores through
// pt_store and passes float_out = true for bf16 out as well.
static int64_t forward_long_threshold(int64_t row_waves, int64_t nnz,
                                      int64_t num_rows, bool float_out) {
  if (!float_out) return INT64_MAX;
  const int64_t ave = num_rows > 0 ? nnz / num_rows : 0;
  int64_t long_thresh = LONG_T;
  if (row_waves >= 4096) {
    long_thresh = 4 * (ave > 0 ? ave : 1);
    if (long_thresh < LONG_T) long_thresh = LONG_T;
    if (long_thresh > 8192) long_thresh = 8192;
  }
  return long_thresh;
}

// Kernel A's long-row list starts empty, and so does the work list.
static void reset_long_lists(int32_t* long_count, int32_t* n_work,
                             hipStream_t stream) {
  hipMemsetAsync(long_count, 0, sizeof(int32_t), stream);
  hipMemsetAsync(n_work, 0, sizeof(int32_t), stream);
}

// The forward's long pass behind kernel A: expand the long-row list to
// (row, chunk) work items, then reduce them into the fp32 output.
template <int TILE, int VEC, bool MEAN, bool HAS_W, typename PT>
static void launch_forward_long_pass(const PT* params, const int64_t* values,
                                     const int64_t* splits,
                                     const float* per_id_w, float* out,
                                     int64_t vocab, int width,
                                     int64_t* long_rows, int32_t* long_count,
                                     int64_t* work_items, int32_t* n_work,
                                     int tile_w, hipStream_t stream) {
  const dim3 block(256);
  hipLaunchKernelGGL(expand_long_work<false>, dim3(512), block, 0, stream,
                     long_rows, long_count, splits, work_items, n_work,
                     (int32_t*)nullptr);
  hipLaunchKernelGGL((csr_fwd_long<TILE, VEC, MEAN, HAS_W, false, PT>),
                     dim3(2048), block, 0, stream, params, values, splits,
                     per_id_w, out, vocab, width, long_rows, work_items, n_work,
                     tile_w);
}

// Deterministic mode: where to put the long rows' partials.  slab is fp32
// [work item capacity, width], work_base int32 [long-row capacity]; a null
// slab means the mode is off.
struct DetBuffers {
  float* slab;
  int32_t* work_base;
};

// The fixed-order sum of every long row's slab partials, stored to
// dst[row] (or, TO_SCRATCH, to scratch row li).
template <bool TO_SCRATCH, typename OT>
static void launch_slab_combine(const DetBuffers& det, OT* dst, int width,
                                const int64_t* long_rows,
                                const int32_t* long_count,
                                const int64_t* splits,
                                const int64_t* work_items,
                                const int32_t* n_work, hipStream_t stream) {
  const dim3 block(256);
  hipLaunchKernelGGL(long_slab_group_sum, dim3(2048), block, 0, stream,
                     det.slab, width, long_rows, splits, work_items, n_work);
  hipLaunchKernelGGL((long_slab_combine<TO_SCRATCH, OT>), dim3(256), block, 0,
                     stream, det.slab, dst, width, long_rows, long_count,
                     splits, det.work_base);
}

// The deterministic long pass: the same work list with each row's base
// recorded, partials into the slab, then the fixed-order combine into out
// (fp32 or bf16).
template <int TILE, int VEC, bool MEAN, bool HAS_W, typename PT, typename OT>
static void launch_forward_long_pass_det(
    const PT* params, const int64_t* values, const int64_t* splits,
    const float* per_id_w, OT* out, int64_t vocab, int width,
    int64_t* long_rows, int32_t* long_count, int64_t* work_items,
    int32_t* n_work, int tile_w, const DetBuffers& det, hipStream_t stream) {
  const dim3 block(256);
  hipLaunchKernelGGL(expand_long_work<true>, dim3(512), block, 0, stream,
                     long_rows, long_count, splits, work_items, n_work,
                     det.work_base);
  hipLaunchKernelGGL((csr_fwd_long<TILE, VEC, MEAN, HAS_W, true, PT>),
                     dim3(2048), block, 0, stream, params, values, splits,
                     per_id_w, det.slab, vocab, width, long_rows, work_items,
                     n_work, tile_w);
  launch_slab_combine<false>(det, out, width, long_rows, long_count, splits,
                             work_items, n_work, stream);
}

template <typename PT, typename OT>
static void launch_csr_lookup_forward_t(const PT* params, const int64_t* values,
                                        const int64_t* splits,
                                        const float* per_id_w, OT* out,
                                        int64_t num_rows, int64_t nnz,
                                        int64_t vocab, int width, bool mean,
                                        int64_t* long_rows, int32_t* long_count,
                                        int64_t* work_items, int32_t* n_work,
                                        const DetBuffers& det,
                                        hipStream_t stream) {
  const dim3 block(256);
  reset_long_lists(long_count, n_work, stream);
  dispatch_width(width, [&](auto tile, auto vec) {
    constexpr int TILE = decltype(tile)::value, VEC = decltype(vec)::value;
    constexpr bool kFloatOut = std::is_same<OT, float>::value;
    const RowTiling t = row_tiling<TILE, VEC>(width, num_rows);
    const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
    const int64_t long_thresh = forward_long_threshold(
        t.row_waves, nnz, num_rows, kFloatOut || det.slab != nullptr);
    dispatch_bool(mean, [&](auto mean_t) {
      dispatch_bool(per_id_w != nullptr, [&](auto has_w_t) {
        constexpr bool MEAN = decltype(mean_t)::value;
        constexpr bool HAS_W = decltype(has_w_t)::value;
        if constexpr (TILE > 0)
          hipLaunchKernelGGL((csr_fwd_narrow<TILE, MEAN, HAS_W, PT, OT>), grid,
                             block, 0, stream, params, values, splits,
                             per_id_w, out, num_rows, vocab, width,
                             long_thresh, long_rows, long_count);
        else
          hipLaunchKernelGGL((csr_fwd_wide<VEC, MEAN, HAS_W, PT, OT>), grid,
                             block, 0, stream, params, values, splits,
                             per_id_w, out, num_rows, vocab, width,
                             long_thresh, long_rows, long_count, t.tile_w);
        if (det.slab != nullptr)
          launch_forward_long_pass_det<TILE, VEC, MEAN, HAS_W>(
              params, values, splits, per_id_w, out, vocab, width, long_rows,
              long_count, work_items, n_work, t.tile_w, det, stream);
        else if constexpr (kFloatOut)
          launch_forward_long_pass<TILE, VEC, MEAN, HAS_W>(
              params, values, splits, per_id_w, (float*)out, vocab, width,
              long_rows, long_count, work_items, n_work, t.tile_w, stream);
      });
    });
  });
}

void launch_csr_lookup_forward(const void* params, bool params_bf16,
                               const int64_t* values, const int64_t* splits,
                               const float* per_id_w, void* out, bool out_bf16,
                               int64_t num_rows, int64_t nnz, int64_t vocab,
                               int width, bool mean, int64_t* long_rows,
                               int32_t* long_count, int64_t* work_items,
                               int32_t* n_work, float* det_slab,
                               int32_t* det_work_base, hipStream_t stream) {
  const DetBuffers det{det_slab, det_work_base};
  dispatch_bool(params_bf16, [&](auto p_bf16) {
    dispatch_bool(out_bf16, [&](auto o_bf16) {
      using PT = storage_t<decltype(p_bf16)>;
      using OT = storage_t<decltype(o_bf16)>;
      launch_csr_lookup_forward_t((const PT*)params, values, splits, per_id_w,
                                  (OT*)out, num_rows, nnz, vocab, width, mean,
                                  long_rows, long_count, work_items, n_work,
                                  det, stream);
    });
  });
}

// ---------------------------------------------------------------------------
// int8 row-wise quantized tables: forward, quantize_rows, dequantize_rows.
// ---------------------------------------------------------------------------

// The quantized forward is csr_fwd_wide / csr_fwd_long instantiated on q8_t
// at every width: tile_w = pow2(width / 4) lanes own a row (64 rows per wave
// at width 4, 2 at width 128), the column loop runs from width 260 on, and
// the long-row list, its expansion and the atomic combine are the fp32
// tables' own.  vocab must be > 0 (see the q8_t wide_accumulate).
//
// int4 tables (QT = q4_t, VEC = 8) run the same two kernels with
// tile_w = pow2(width / 8) lanes per row: 64 rows per wave at width 8, 4 at
// width 128, and the column loop from width 520 on.
template <int VEC, typename QT, typename OT>
static void launch_csr_lookup_forward_packed_t(
    const QT* params, const int64_t* values, const int64_t* splits,
    const float* per_id_w, OT* out, int64_t num_rows, int64_t nnz,
    int64_t vocab, int width, bool mean, int64_t* long_rows,
    int32_t* long_count, int64_t* work_items, int32_t* n_work,
    const DetBuffers& det, hipStream_t stream) {
  constexpr bool kFloatOut = std::is_same<OT, float>::value;
  const dim3 block(256);
  reset_long_lists(long_count, n_work, stream);
  const RowTiling t = row_tiling<0, VEC>(width, num_rows);
  const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
  const int64_t long_thresh = forward_long_threshold(
      t.row_waves, nnz, num_rows, kFloatOut || det.slab != nullptr);
  dispatch_bool(mean, [&](auto mean_t) {
    dispatch_bool(per_id_w != nullptr, [&](auto has_w_t) {
      constexpr bool MEAN = decltype(mean_t)::value;
      constexpr bool HAS_W = decltype(has_w_t)::value;
      hipLaunchKernelGGL((csr_fwd_wide<VEC, MEAN, HAS_W, QT, OT>), grid, block,
                         0, stream, params, values, splits, per_id_w, out,
                         num_rows, vocab, width, long_thresh, long_rows,
                         long_count, t.tile_w);
      if (det.slab != nullptr)
        launch_forward_long_pass_det<0, VEC, MEAN, HAS_W>(
            params, values, splits, per_id_w, out, vocab, width, long_rows,
            long_count, work_items, n_work, t.tile_w, det, stream);
      else if constexpr (kFloatOut)
        launch_forward_long_pass<0, VEC, MEAN, HAS_W>(
            params, values, splits, per_id_w, (float*)out, vocab, width,
            long_rows, long_count, work_items, n_work, t.tile_w, stream);
    });
  });
}

void launch_csr_lookup_forward_q8(const void* packed, const int64_t* values,
                                  const int64_t* splits, const float* per_id_w,
                                  void* out, bool out_bf16, int64_t num_rows,
                                  int64_t nnz, int64_t vocab, int width,
                                  bool mean, int64_t* long_rows,
                                  int32_t* long_count, int64_t* work_items,
                                  int32_t* n_work, float* det_slab,
                                  int32_t* det_work_base, hipStream_t stream) {
  const DetBuffers det{det_slab, det_work_base};
  dispatch_bool(out_bf16, [&](auto o_bf16) {
    using OT = storage_t<decltype(o_bf16)>;
    launch_csr_lookup_forward_packed_t<4>(
        (const q8_t*)packed, values, splits, per_id_w, (OT*)out, num_rows, nnz,
        vocab, width, mean, long_rows, long_count, work_items, n_work, det,
        stream);
  });
}

void launch_csr_lookup_forward_q4(const void* packed, const int64_t* values,
                                  const int64_t* splits, const float* per_id_w,
                                  void* out, bool out_bf16, int64_t num_rows,
                                  int64_t nnz, int64_t vocab, int width,
                                  bool mean, int64_t* long_rows,
                                  int32_t* long_count, int64_t* work_items,
                                  int32_t* n_work, float* det_slab,
                                  int32_t* det_work_base, hipStream_t stream) {
  const DetBuffers det{det_slab, det_work_base};
  dispatch_bool(out_bf16, [&](auto o_bf16) {
    using OT = storage_t<decltype(o_bf16)>;
    launch_csr_lookup_forward_packed_t<8>(
        (const q4_t*)packed, values, splits, per_id_w, (OT*)out, num_rows, nnz,
        vocab, width, mean, long_rows, long_count, work_items, n_work, det,
        stream);
  });
}

// min / max of v over the `tile` (pow2 <= WAVE) lanes of the caller's lane
// group, by xor butterfly as in tile_sum: every lane of the group calls it.
__device__ __forceinline__ float tile_min(float v, int tile) {
  for (int off = tile >> 1; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float tile_max(float v, int tile) {
  for (int off = tile >> 1; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// quantize_rows: in [n, width] fp32 or bf16 -> packed [n, width + 8].  One
// tile_w-lane group per row, four columns per lane and trip.  Pass 1 finds
// the row's min and max (butterfly inside the group), pass 2 re-reads the
// lane's columns — they are in L1/L2 — quantizes them and stores one dword;
// the group's first lane stores scale and bias.
//   bias = min, scale = (max - min) / 255,
//   q = clamp(rint((x - bias) * (255 / (max - min))), 0, 255)
// and q = 0, scale = 0 for a constant row, which then dequantizes to bias.
// A group whose row is past n keeps running with live == false, so the
// shuffles never read a lane that has left the loop.
template <typename ST>
__global__ void quantize_rows_kernel(const ST* __restrict__ in,
                                     unsigned char* __restrict__ out,
                                     int64_t n, int width, int tile_w) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, tile_w);
  for (int64_t base = wc.wave_id * tc.rpw; base < n;
       base += wc.n_waves * tc.rpw) {
    const int64_t row = base + tc.sub;
    const bool live = row < n;
    const ST* src = in + (live ? row : 0) * (int64_t)width;
    float lo = INFINITY, hi = -INFINITY;
    if (live) {
      for (int col0 = tc.tl * 4; col0 < width; col0 += tile_w * 4) {
        float x[4];
        pt_load4(src + col0, x);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          lo = fminf(lo, x[v]);
          hi = fmaxf(hi, x[v]);
        }
      }
    }
    lo = tile_min(lo, tile_w);
    hi = tile_max(hi, tile_w);
    if (!live) continue;
    const float range = hi - lo;
    const float scale = range / 255.f;
    const float inv = range > 0.f ? 255.f / range : 0.f;
    unsigned char* dst = out + row * (int64_t)(width + Q8_TAIL);
    for (int col0 = tc.tl * 4; col0 < width; col0 += tile_w * 4) {
      float x[4];
      pt_load4(src + col0, x);
      unsigned int q = 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float r = fminf(fmaxf(rintf((x[v] - lo) * inv), 0.f), 255.f);
        q |= (unsigned int)r << (8 * v);
      }
      *reinterpret_cast<unsigned int*>(dst + col0) = q;
    }
    if (tc.tl == 0) {
      *reinterpret_cast<float*>(dst + width) = scale;
      *reinterpret_cast<float*>(dst + width + 4) = lo;
    }
  }
}

// dequantize_rows: packed [n, width + 8] -> fp32 [n, width] as
// fma(scale, q, bias): one rounding per element, written as an explicit fmaf
// so the bits do not depend on the compiler's contraction choices.
__global__ void dequantize_rows_kernel(const q8_t* __restrict__ in,
                                       float* __restrict__ out, int64_t n,
                                       int width, int tile_w) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, tile_w);
  for (int64_t base = wc.wave_id * tc.rpw; base < n;
       base += wc.n_waves * tc.rpw) {
    const int64_t row = base + tc.sub;
    if (row >= n) continue;
    const unsigned char* src = q8_row(in, row, width);
    const float scale = q8_scale(src, width), bias = q8_bias(src, width);
    for (int col0 = tc.tl * 4; col0 < width; col0 += tile_w * 4) {
      const unsigned int q = q8_load4(src, col0);
      float x[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) x[v] = fmaf(scale, q8_byte(q, v), bias);
      pt_store4(out + row * (int64_t)width + col0, x);
    }
  }
}

void launch_quantize_rows_q8(const void* in, bool in_bf16, void* packed,
                             int64_t n, int width, hipStream_t stream) {
  if (n <= 0) return;
  const dim3 block(256);
  const RowTiling t = row_tiling<0, 4>(width, n);
  const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
  dispatch_bool(in_bf16, [&](auto i_bf16) {
    using ST = storage_t<decltype(i_bf16)>;
    hipLaunchKernelGGL((quantize_rows_kernel<ST>), grid, block, 0, stream,
                       (const ST*)in, (unsigned char*)packed, n, width,
                       t.tile_w);
  });
}

void launch_dequantize_rows_q8(const void* packed, float* out, int64_t n,
                               int width, hipStream_t stream) {
  if (n <= 0) return;
  const dim3 block(256);
  const RowTiling t = row_tiling<0, 4>(width, n);
  const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
  hipLaunchKernelGGL(dequantize_rows_kernel, grid, block, 0, stream,
                     (const q8_t*)packed, out, n, width, t.tile_w);
}

// quantize_rows_q4: in [n, width] fp32 or bf16 -> packed [n, width / 2 + 4],
// the bytes of FBGEMM's fused 4-bit row-wise quantizer.  The int8 kernel's
// shape with eight columns per lane and trip and one dword of nibbles stored:
//   b = fp16(min) (nearest-even), range = max - b,
//   s = fp16(range == 0 ? 1 : range / 15), and s = 1 if s == 0 or 1/s == inf,
//   q = clamp(rint((x - b) * (1 / s)), 0, 15)
// with b and s widened back to fp32 before use.  A constant row of an
// fp16-representable value stores q = 0, scale 1 and that value; any other
// constant has range = x - fp16(x) != 0 and takes the general path.  Rows
// with |x| > 65504 or NaN are outside the contract (fp16 overflows), as they
// are for FBGEMM.
template <typename ST>
__global__ void quantize_rows_q4_kernel(const ST* __restrict__ in,
                                        unsigned char* __restrict__ out,
                                        int64_t n, int width, int tile_w) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, tile_w);
  for (int64_t base = wc.wave_id * tc.rpw; base < n;
       base += wc.n_waves * tc.rpw) {
    const int64_t row = base + tc.sub;
    const bool live = row < n;
    const ST* src = in + (live ? row : 0) * (int64_t)width;
    float lo = INFINITY, hi = -INFINITY;
    if (live) {
      for (int col0 = tc.tl * 8; col0 < width; col0 += tile_w * 8) {
        float x[8];
        pt_load4(src + col0, x);
        pt_load4(src + col0 + 4, x + 4);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          lo = fminf(lo, x[v]);
          hi = fmaxf(hi, x[v]);
        }
      }
    }
    lo = tile_min(lo, tile_w);
    hi = tile_max(hi, tile_w);
    if (!live) continue;
    const _Float16 bias_h = (_Float16)lo;
    const float bias = (float)bias_h;
    const float range = hi - bias;
    _Float16 scale_h = (_Float16)(range == 0.f ? 1.f : range / 15.f);
    float scale = (float)scale_h;
    if (scale == 0.f || isinf(1.f / scale)) {
      scale_h = (_Float16)1.f;
      scale = 1.f;
    }
    const float inv = 1.f / scale;
    unsigned char* dst = out + row * (int64_t)(width / 2 + Q4_TAIL);
    for (int col0 = tc.tl * 8; col0 < width; col0 += tile_w * 8) {
      float x[8];
      pt_load4(src + col0, x);
      pt_load4(src + col0 + 4, x + 4);
      unsigned int q = 0;
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const float r = fminf(fmaxf(rintf((x[v] - bias) * inv), 0.f), 15.f);
        q |= (unsigned int)r << (4 * v);
      }
      *reinterpret_cast<unsigned int*>(dst + col0 / 2) = q;
    }
    if (tc.tl == 0)
      *reinterpret_cast<unsigned int*>(dst + width / 2) =
          (unsigned int)__builtin_bit_cast(unsigned short, scale_h) |
          ((unsigned int)__builtin_bit_cast(unsigned short, bias_h) << 16);
  }
}

// dequantize_rows_q4: packed [n, width / 2 + 4] -> fp32 [n, width] as
// fma(scale, q, bias), scale and bias widened from fp16.
__global__ void dequantize_rows_q4_kernel(const q4_t* __restrict__ in,
                                          float* __restrict__ out, int64_t n,
                                          int width, int tile_w) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, tile_w);
  for (int64_t base = wc.wave_id * tc.rpw; base < n;
       base += wc.n_waves * tc.rpw) {
    const int64_t row = base + tc.sub;
    if (row >= n) continue;
    const unsigned char* src = q4_row(in, row, width);
    const unsigned int tail = q4_tail(src, width);
    const float scale = q4_scale(tail), bias = q4_bias(tail);
    for (int col0 = tc.tl * 8; col0 < width; col0 += tile_w * 8) {
      float x[8];
      q4_unpack8(q4_load8(src, col0), x);
#pragma unroll
      for (int v = 0; v < 8; ++v) x[v] = fmaf(scale, x[v], bias);
      pt_store8(out + row * (int64_t)width + col0, x);
    }
  }
}

void launch_quantize_rows_q4(const void* in, bool in_bf16, void* packed,
                             int64_t n, int width, hipStream_t stream) {
  if (n <= 0) return;
  const dim3 block(256);
  const RowTiling t = row_tiling<0, 8>(width, n);
  const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
  dispatch_bool(in_bf16, [&](auto i_bf16) {
    using ST = storage_t<decltype(i_bf16)>;
    hipLaunchKernelGGL((quantize_rows_q4_kernel<ST>), grid, block, 0, stream,
                       (const ST*)in, (unsigned char*)packed, n, width,
                       t.tile_w);
  });
}

void launch_dequantize_rows_q4(const void* packed, float* out, int64_t n,
                               int width, hipStream_t stream) {
  if (n <= 0) return;
  const dim3 block(256);
  const RowTiling t = row_tiling<0, 8>(width, n);
  const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
  hipLaunchKernelGGL(dequantize_rows_q4_kernel, grid, block, 0, stream,
                     (const q4_t*)packed, out, n, width, t.tile_w);
}

// ---------------------------------------------------------------------------
// row_to_split: COO row coords (sorted) -> CSR splits, one thread per output.
// ---------------------------------------------------------------------------

__global__ void row_to_split_kernel(const int64_t* __restrict__ rows,
                                    int64_t nnz, int64_t num_rows,
                                    int64_t* __restrict__ splits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > num_rows) return;
  // lower_bound of i in rows[0..nnz)
  int64_t lo = 0, hi = nnz;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rows[mid] < i) lo = mid + 1; else hi = mid;
  }
  splits[i] = lo;
}

void launch_row_to_split(const int64_t* rows, int64_t nnz, int64_t num_rows,
                         int64_t* splits, hipStream_t stream) {
  const int block = 256;
  const int grid = (int)cdiv64(num_rows + 1, block);
  hipLaunchKernelGGL(row_to_split_kernel, dim3(grid), dim3(block), 0, stream,
                     rows, nnz, num_rows, splits);
}

// ---------------------------------------------------------------------------
// Backward pipeline.
// ---------------------------------------------------------------------------

// Expand CSR offsets to per-id row ids and, when MEAN || USER_W, the per-id
// weight w[k] = c_r * user_w[k]: c_r is 1/len for MEAN and 1 otherwise, and
// user_w[k] counts as 1 without USER_W.
template <bool MEAN, bool USER_W>
__global__ void expand_row_ids(const int64_t* __restrict__ splits,
                               int64_t num_rows, int32_t* __restrict__ row_ids,
                               float* __restrict__ w,
                               const float* __restrict__ user_w) {
  const WaveCoord wc = wave_coord();
  for (int64_t row = wc.wave_id; row < num_rows; row += wc.n_waves) {
    const int64_t s = splits[row], e = splits[row + 1];
    const float iw = (MEAN && e > s) ? 1.f / (float)(e - s) : 1.f;
    for (int64_t k = s + wc.lane; k < e; k += WAVE) {
      row_ids[k] = (int32_t)row;
      if (USER_W) w[k] = iw * user_w[k];
      else if (MEAN) w[k] = iw;
    }
  }
}

// Head flags over sorted ids (ids clamped: OOB sorted to the end as sentinel).
__global__ void mark_heads(const int64_t* __restrict__ sorted_ids, int64_t n,
                           int64_t vocab, int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t id = sorted_ids[i];
  const bool valid = id >= 0 && id < vocab;
  head[i] = (valid && (i == 0 || sorted_ids[i - 1] != id)) ? 1 : 0;
}

// Scatter unique ids + segment starts using the inclusive-scanned head flags.
__global__ void scatter_unique(const int64_t* __restrict__ sorted_ids,
                               const int32_t* __restrict__ head,
                               const int32_t* __restrict__ pos, int64_t n,
                               int64_t* __restrict__ unique_ids,
                               int64_t* __restrict__ seg_offsets,
                               int32_t* __restrict__ num_unique) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (head[i]) {
    const int32_t u = pos[i] - 1;
    unique_ids[u] = sorted_ids[i];
    seg_offsets[u] = i;
  }
  // valid count; trailing OOB ids (sorted last) carry no head flag
  if (i == n - 1) *num_unique = pos[i];
}

// *valid_end = first index with id >= vocab.  OOB ids (negatives included)
// are masked to the `vocab` sentinel before the sort, so they all sort last
// and the last unique segment ends here.
__global__ void find_valid_bounds(const int64_t* __restrict__ sorted_ids,
                                  int64_t n, int64_t vocab,
                                  int64_t* __restrict__ valid_end) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted_ids[mid] < vocab) lo = mid + 1; else hi = mid;
  }
  *valid_end = lo;
}

size_t csr_backward_temp_bytes(int64_t nnz) {
  // only the head-flag inclusive scan uses rocPRIM temp storage now (the
  // sort is the hand-written radix_sort.hip path)
  size_t scan_bytes = 0;
  rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr,
                          (int32_t*)nullptr, (size_t)nnz);
  return scan_bytes;
}

// Orchestration is done on the host side (bindings.cpp) because output
// allocation needs num_unique; these launchers expose the pieces.
// Short segments (the common forward-input shape: hotness 1..tens): one
// THREAD per row — a wave per hotness-1 row left 63 of 64 lanes idle and
// made this trivial expansion ~100x slower than its write bandwidth.
template <bool MEAN, bool USER_W>
__global__ void expand_row_ids_thread(const int64_t* __restrict__ splits,
                                      int64_t num_rows,
                                      int32_t* __restrict__ row_ids,
                                      float* __restrict__ w,
                                      const float* __restrict__ user_w) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < num_rows; row += stride) {
    const int64_t s = splits[row], e = splits[row + 1];
    const float iw = (MEAN && e > s) ? 1.f / (float)(e - s) : 1.f;
    for (int64_t k = s; k < e; ++k) {
      row_ids[k] = (int32_t)row;
      if (USER_W) w[k] = iw * user_w[k];
      else if (MEAN) w[k] = iw;
    }
  }
}

void launch_expand_row_ids(const int64_t* splits, int64_t num_rows,
                           int64_t nnz, int32_t* row_ids, float* w, bool mean,
                           const float* user_w, hipStream_t stream) {
  const int block = 256;
  const int64_t ave = num_rows > 0 ? nnz / num_rows : 0;
  dispatch_bool(mean, [&](auto mean_t) {
    dispatch_bool(user_w != nullptr, [&](auto user_w_t) {
      constexpr bool MEAN = decltype(mean_t)::value;
      constexpr bool USER_W = decltype(user_w_t)::value;
      float* wp = (MEAN || USER_W) ? w : nullptr;
      if (ave <= 16)
        hipLaunchKernelGGL((expand_row_ids_thread<MEAN, USER_W>),
                           dim3(pick_grid(num_rows, block)), dim3(block), 0,
                           stream, splits, num_rows, row_ids, wp, user_w);
      else
        hipLaunchKernelGGL((expand_row_ids<MEAN, USER_W>),
                           dim3(pick_grid(num_rows, block / WAVE)),
                           dim3(block), 0, stream, splits, num_rows, row_ids,
                           wp, user_w);
    });
  });
}

hipError_t run_inclusive_scan_i32(void* temp, size_t temp_bytes,
                                  const int32_t* in, int32_t* out, int64_t n,
                                  hipStream_t stream) {
  return rocprim::inclusive_scan(temp, temp_bytes, in, out, (size_t)n,
                                 rocprim::plus<int32_t>(), stream);
}

void launch_mark_heads(const int64_t* sorted_ids, int64_t n, int64_t vocab,
                       int32_t* head, hipStream_t stream) {
  const int block = 256;
  const int64_t grid = cdiv64(n, block);
  hipLaunchKernelGGL(mark_heads, dim3((int)grid), dim3(block), 0, stream,
                     sorted_ids, n, vocab, head);
}

void launch_scatter_unique(const int64_t* sorted_ids, const int32_t* head,
                           const int32_t* pos, int64_t n, int64_t* unique_ids,
                           int64_t* seg_offsets, int32_t* num_unique,
                           hipStream_t stream) {
  const int block = 256;
  const int64_t grid = cdiv64(n, block);
  hipLaunchKernelGGL(scatter_unique, dim3((int)grid), dim3(block), 0, stream,
                     sorted_ids, head, pos, n, unique_ids, seg_offsets,
                     num_unique);
}

// Packed variant: (masked_id << 32) | position — the whole sort pipeline
// moves ONE u64 array (digits live in bits [32, 32+log2(vocab+1))).
__global__ void mask_oob_pack(const int64_t* __restrict__ ids, int64_t n,
                              int64_t vocab, uint64_t* __restrict__ packed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  const uint64_t m = (id < 0 || id >= vocab) ? (uint64_t)vocab : (uint64_t)id;
  packed[i] = (m << 32) | (uint32_t)i;
}

__global__ void unpack_sorted(const uint64_t* __restrict__ packed, int64_t n,
                              int64_t* __restrict__ sorted_ids,
                              int32_t* __restrict__ sorted_pos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t p = packed[i];
  sorted_ids[i] = (int64_t)(p >> 32);
  sorted_pos[i] = (int32_t)(uint32_t)(p & 0xffffffffu);
}

void launch_mask_oob_pack(const int64_t* ids, int64_t n, int64_t vocab,
                          uint64_t* packed, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(mask_oob_pack, dim3((int)cdiv64(n, block)), dim3(block),
                     0, stream, ids, n, vocab, packed);
}

void launch_unpack_sorted(const uint64_t* packed, int64_t n,
                          int64_t* sorted_ids, int32_t* sorted_pos,
                          hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(unpack_sorted, dim3((int)cdiv64(n, block)), dim3(block),
                     0, stream, packed, n, sorted_ids, sorted_pos);
}

hipError_t run_sort_keys_u64(void* temp, size_t temp_bytes,
                             const uint64_t* keys_in, uint64_t* keys_out,
                             int64_t n, int begin_bit, int end_bit,
                             hipStream_t stream) {
  return rocprim::radix_sort_keys(temp, temp_bytes, keys_in, keys_out,
                                  (size_t)n, (unsigned)begin_bit,
                                  (unsigned)end_bit, stream);
}

size_t rocprim_sort_keys_temp_bytes(int64_t n) {
  size_t bytes = 0;
  rocprim::radix_sort_keys(nullptr, bytes, (const uint64_t*)nullptr,
                           (uint64_t*)nullptr, (size_t)n);
  return bytes;
}

// Permute row ids (+ mean weights) by the sorted payload, widening to i64 so
// the segmented sum can reuse the forward gather-reduce kernels directly.
__global__ void gather_sorted(const int32_t* __restrict__ perm,
                              const int32_t* __restrict__ row_ids,
                              const float* __restrict__ w, int64_t n,
                              int64_t* __restrict__ srow,
                              float* __restrict__ sw) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t p = perm[i];
  srow[i] = (int64_t)row_ids[p];
  if (sw) sw[i] = w[p];
}

void launch_gather_sorted(const int32_t* perm, const int32_t* row_ids,
                          const float* w, int64_t n, int64_t* srow, float* sw,
                          hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(gather_sorted, dim3((int)cdiv64(n, block)), dim3(block), 0,
                     stream, perm, row_ids, w, n, srow, sw);
}

__global__ void set_seg_end(int64_t* __restrict__ seg_offsets,
                            const int32_t* __restrict__ num_unique,
                            const int64_t* __restrict__ valid_end) {
  seg_offsets[*num_unique] = *valid_end;
}

void launch_set_seg_end(int64_t* seg_offsets, const int32_t* num_unique,
                        const int64_t* valid_end, hipStream_t stream) {
  hipLaunchKernelGGL(set_seg_end, dim3(1), dim3(1), 0, stream, seg_offsets,
                     num_unique, valid_end);
}

void launch_find_valid_bounds(const int64_t* sorted_ids, int64_t n,
                              int64_t vocab, int64_t* valid_end,
                              hipStream_t stream) {
  hipLaunchKernelGGL(find_valid_bounds, dim3(1), dim3(1), 0, stream, sorted_ids,
                     n, vocab, valid_end);
}

// Pads seg_offsets[i >= num_unique] to the first OOB position so padded
// segments are empty and the update kernels need no host-side count.
__global__ void pad_seg_offsets(int64_t* __restrict__ seg, int64_t n,
                                const int32_t* __restrict__ num_unique,
                                const int64_t* __restrict__ valid_end) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i >= *num_unique) seg[i] = *valid_end;
}

void launch_pad_seg_offsets(int64_t* seg, int64_t n, const int32_t* num_unique,
                            const int64_t* valid_end, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(pad_seg_offsets, dim3((int)cdiv64(n + 1, block)),
                     dim3(block), 0, stream, seg, n, num_unique, valid_end);
}

// Short segments: one wave (narrow) or tile_w lanes (wide) per unique id,
// direct (non-atomic) update.  Grid-strides only over the REAL segment count
// (*nu_ptr), not the padded nnz-sized buffer.  srow comes from our own
// expansion, so the gathers need no bounds check.
template <int TILE, int VEC, bool HAS_W, int RULE, bool SR, typename PT,
          typename GT>
__global__ void sorted_opt_update(PT* __restrict__ weight,
                                  float* __restrict__ state, float eps,
                                  const int64_t* __restrict__ sorted_ids,
                                  const int64_t* __restrict__ seg,
                                  const int64_t* __restrict__ srow,
                                  const float* __restrict__ sw,
                                  const GT* __restrict__ grad_out,
                                  const float* __restrict__ lr_ptr,
                                  const int32_t* __restrict__ nu_ptr,
                                  int64_t long_thresh, int width,
                                  int64_t* __restrict__ long_rows,
                                  int32_t* __restrict__ long_count,
                                  int tile_w,
                                  const int64_t* __restrict__ sr_ptr,
                                  AdamArgs ad) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, TILE > 0 ? WAVE : tile_w);
  const float lr = *lr_ptr;
  const int64_t n_segs = *nu_ptr;
  const SrState sr = sr_load<SR>(sr_ptr);
  for (int64_t rbase = wc.wave_id * tc.rpw; rbase < n_segs;
       rbase += wc.n_waves * tc.rpw) {
    const int64_t r = rbase + tc.sub;
    if (r >= n_segs) continue;
    const int64_t s = seg[r], e = seg[r + 1];
    if (s >= e) continue;
    if (e - s > long_thresh) {
      if (tc.tl == 0) long_rows[atomicAdd(long_count, 1)] = r;
      continue;
    }
    const int64_t row0 = sorted_ids[s] * (int64_t)width;
    if constexpr (TILE > 0) {
      const float g = narrow_reduce<TILE, WAVE / TILE, 2, HAS_W, false>(
          grad_out, srow, sw, 0, width, s, e, wc.lane);
      if (wc.lane < TILE && wc.lane < width) {
        const int64_t o = row0 + wc.lane;
        apply_row_update<RULE>(&weight[o],
                               RULE != RULE_SGD ? &state[o] : nullptr, g, lr,
                               eps, sr, sr_group_hash(sr, o), o, ad);
      }
    } else {
      for (int col0 = tc.tl * VEC; col0 < width; col0 += tile_w * VEC) {
        float acc[VEC];
        wide_accumulate<VEC, HAS_W, false>(grad_out, srow, sw, 0, width, col0,
                                           s, e, acc);
        // VEC divides width and col0, so o0 is a multiple of VEC and its
        // VEC elements sit in one group of four: one hash for all
        const int64_t o0 = row0 + col0;
        if constexpr (RULE == RULE_ADAM) {
          // Each group goes whole into registers and whole back, with one
          // vector access per array; v_off is a multiple of VEC because
          // width is.  Left to per-element accesses the apply took 1696 us
          // on uniform ids (10M x 128 fp32, Adagrad 924 us), this way
          // 1100 us: m and v share one array a runtime distance apart, so
          // the compiler may not move a load of one across a store to the
          // other.
          float wv[VEC], mv[VEC], vv[VEC];
          pt_loadv<VEC>(weight + o0, wv);
          pt_loadv<VEC>(state + o0, mv);
          pt_loadv<VEC>(state + o0 + ad.v_off, vv);
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            wv[v] = adam_value(wv[v], mv[v], vv[v], acc[v], lr, eps, ad);
          pt_storev<VEC>(state + o0, mv);
          pt_storev<VEC>(state + o0 + ad.v_off, vv);
          pt_storev_sr<VEC>(weight + o0, wv, sr, o0);
        } else if constexpr (SR) {
          // One vector load and store per group.  The compiler makes these
          // of the nearest-even path's per-element ones, but not once each
          // store branches on finite / non-finite (measured: +24% on SGD,
          // +50% on Adagrad with four 2-byte loads and stores per lane).
          float wv[VEC];
          pt_loadv<VEC>(weight + o0, wv);
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            wv[v] = row_update_value<RULE>(
                wv[v], RULE != RULE_SGD ? &state[o0 + v] : nullptr, acc[v], lr,
                eps, true, ad);
          pt_storev_sr<VEC>(weight + o0, wv, sr, o0);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const int64_t o = o0 + v;
            apply_row_update<RULE>(&weight[o],
                                   RULE != RULE_SGD ? &state[o] : nullptr,
                                   acc[v], lr, eps, sr, 0, o, ad);
          }
        }
      }
    }
  }
}

// Row-wise Adagrad twin of sorted_opt_update.  A row's sum of squares has to
// be complete before its first column moves, so the wide path walks the
// columns twice: once for the squares, once for the update.  A row that fits
// one column pass (width <= tile_w * VEC) keeps its sums in registers in
// between; a wider one gathers them a second time.  The row loop and both
// column loops have wave-uniform trip counts, and a wide group with nothing
// to do stays in step with live == false, because the lanes of one wave
// shuffle together.
template <int TILE, int VEC, bool HAS_W, bool SR, typename PT, typename GT>
__global__ void sorted_opt_update_rowwise(
    PT* __restrict__ weight, float* __restrict__ state, float eps,
    const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ seg,
    const int64_t* __restrict__ srow, const float* __restrict__ sw,
    const GT* __restrict__ grad_out, const float* __restrict__ lr_ptr,
    const int32_t* __restrict__ nu_ptr, int64_t long_thresh, int width,
    int64_t* __restrict__ long_rows, int32_t* __restrict__ long_count,
    int tile_w, const int64_t* __restrict__ sr_ptr) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, TILE > 0 ? WAVE : tile_w);
  const float lr = *lr_ptr;
  const int64_t n_segs = *nu_ptr;
  const SrState sr = sr_load<SR>(sr_ptr);
  for (int64_t rbase = wc.wave_id * tc.rpw; rbase < n_segs;
       rbase += wc.n_waves * tc.rpw) {
    const int64_t r = rbase + tc.sub;
    int64_t s = 0, e = 0;
    if (r < n_segs) {
      s = seg[r];
      e = seg[r + 1];
    }
    bool live = s < e;
    if (live && e - s > long_thresh) {
      if (tc.tl == 0) long_rows[atomicAdd(long_count, 1)] = r;
      live = false;
    }
    const int64_t uid = live ? sorted_ids[s] : 0;
    PT* wrow = weight + uid * (int64_t)width;
    if constexpr (TILE > 0) {
      if (!live) continue;  // one segment per wave: the whole wave leaves
      const float g = narrow_reduce<TILE, WAVE / TILE, 2, HAS_W, false>(
          grad_out, srow, sw, 0, width, s, e, wc.lane);
      // the fold leaves partial sums on lanes >= TILE: they count as 0
      const bool mine = wc.lane < TILE && wc.lane < width;
      const float ssq = tile_sum(mine ? g * g : 0.f, WAVE);
      const float denom =
          rowwise_denom(&state[uid], ssq, width, wc.lane, WAVE, true, eps);
      if (mine) {
        const int64_t o = uid * (int64_t)width + wc.lane;
        pt_store_sr(&wrow[wc.lane], pt_load(&wrow[wc.lane]) - lr * g / denom,
                    sr, sr_group_hash(sr, o), o);
      }
    } else {
      const int pass_w = tile_w * VEC;
      const int n_pass = (width + pass_w - 1) / pass_w;
      float acc[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
      float ssq = 0.f;
      for (int p = 0; p < n_pass; ++p) {
        const int col0 = p * pass_w + tc.tl * VEC;
        if (live && col0 < width) {
          wide_accumulate<VEC, HAS_W, false>(grad_out, srow, sw, 0, width, col0,
                                             s, e, acc);
#pragma unroll
          for (int v = 0; v < VEC; ++v) ssq += acc[v] * acc[v];
        }
      }
      ssq = tile_sum(ssq, tile_w);
      const float denom =
          rowwise_denom(&state[uid], ssq, width, wc.lane, tile_w, live, eps);
      for (int p = 0; p < n_pass; ++p) {
        const int col0 = p * pass_w + tc.tl * VEC;
        if (live && col0 < width) {
          if (n_pass > 1)
            wide_accumulate<VEC, HAS_W, false>(grad_out, srow, sw, 0, width,
                                               col0, s, e, acc);
          float wv[VEC];
          pt_loadv<VEC>(wrow + col0, wv);
#pragma unroll
          for (int v = 0; v < VEC; ++v) wv[v] -= lr * acc[v] / denom;
          pt_storev_sr<VEC>(wrow + col0, wv, sr,
                            uid * (int64_t)width + col0);
        }
      }
    }
  }
}

// Long segments, fp32 SGD: chunk partials atomically into the weight
// (linear).  Otherwise: chunk partials into fp32 scratch rows, then finalize.
// DET (deterministic mode, TO_SCRATCH only): target is the slab and item
// `item` stores its partial to slab row `item` with plain stores; the
// fixed-order combine then completes the scratch rows (see csr_fwd_long).
template <int TILE, int VEC, bool HAS_W, bool TO_SCRATCH, bool DET,
          typename GT>
__global__ void sorted_opt_long(float* __restrict__ target,  // weight or scratch
                                const int64_t* __restrict__ sorted_ids,
                                const int64_t* __restrict__ seg,
                                const int64_t* __restrict__ srow,
                                const float* __restrict__ sw,
                                const GT* __restrict__ grad_out,
                                const float* __restrict__ lr_ptr, int width,
                                const int64_t* __restrict__ long_rows,
                                const int64_t* __restrict__ work_items,
                                const int32_t* __restrict__ n_work_ptr,
                                int tile_w) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, TILE > 0 ? WAVE : tile_w);
  const float lr = TO_SCRATCH ? 1.f : *lr_ptr;
  const int64_t n_items = *n_work_ptr;
  for (int64_t ibase = wc.wave_id * tc.rpw; ibase < n_items;
       ibase += wc.n_waves * tc.rpw) {
    const int64_t item = ibase + tc.sub;
    if (item >= n_items) continue;
    const LongChunk c = long_chunk(work_items, long_rows, seg, item);
    if (c.ks >= c.e) continue;
    static_assert(TO_SCRATCH || !DET, "the slab feeds the scratch rows");
    float* trow =
        target + (DET ? item : TO_SCRATCH ? c.li : sorted_ids[c.s]) *
                     (int64_t)width;
    if constexpr (TILE > 0) {
      const float g = narrow_reduce<TILE, WAVE / TILE, 2, HAS_W, false>(
          grad_out, srow, sw, 0, width, c.ks, c.ke, wc.lane);
      if (wc.lane < TILE && wc.lane < width) {
        if constexpr (DET) trow[wc.lane] = g;
        else atomicAdd(&trow[wc.lane], TO_SCRATCH ? g : -lr * g);
      }
    } else {
      for (int col0 = tc.tl * VEC; col0 < width; col0 += tile_w * VEC) {
        float acc[VEC];
        wide_accumulate<VEC, HAS_W, false>(grad_out, srow, sw, 0, width, col0,
                                           c.ks, c.ke, acc);
        if constexpr (DET) {
          pt_storev<VEC>(trow + col0, acc);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            atomicAdd(&trow[col0 + v], TO_SCRATCH ? acc[v] : -lr * acc[v]);
        }
      }
    }
  }
}

template <int RULE, bool SR, typename PT>
__global__ void sorted_long_finalize(
    PT* __restrict__ weight, float* __restrict__ state, float eps,
    const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ seg,
    const float* __restrict__ lr_ptr, int width,
    const int64_t* __restrict__ long_rows,
    const int32_t* __restrict__ long_count, const float* __restrict__ scratch,
    const int64_t* __restrict__ sr_ptr, AdamArgs ad) {
  const WaveCoord wc = wave_coord();
  const float lr = *lr_ptr;
  const int64_t n_long = *long_count;
  const SrState sr = sr_load<SR>(sr_ptr);
  for (int64_t li = wc.wave_id; li < n_long; li += wc.n_waves) {
    const int64_t uid = sorted_ids[seg[long_rows[li]]];
    for (int c = wc.lane; c < width; c += WAVE) {
      const int64_t o = uid * (int64_t)width + c;
      apply_row_update<RULE>(&weight[o],
                             RULE != RULE_SGD ? &state[o] : nullptr,
                             scratch[li * (int64_t)width + c], lr, eps, sr,
                             sr_group_hash(sr, o), o, ad);
    }
  }
}

// Row-wise Adagrad finalize: the chunk kernel has completed the scratch row.
template <bool SR, typename PT>
__global__ void sorted_long_finalize_rowwise(
    PT* __restrict__ weight, float* __restrict__ state, float eps,
    const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ seg,
    const float* __restrict__ lr_ptr, int width,
    const int64_t* __restrict__ long_rows,
    const int32_t* __restrict__ long_count, const float* __restrict__ scratch,
    const int64_t* __restrict__ sr_ptr) {
  const WaveCoord wc = wave_coord();
  const float lr = *lr_ptr;
  const int64_t n_long = *long_count;
  const SrState sr = sr_load<SR>(sr_ptr);
  for (int64_t li = wc.wave_id; li < n_long; li += wc.n_waves) {
    const int64_t uid = sorted_ids[seg[long_rows[li]]];
    rowwise_wave_update(weight + uid * (int64_t)width, &state[uid],
                        scratch + li * (int64_t)width, width, wc.lane, lr, eps,
                        sr, uid * (int64_t)width);
  }
}

// Ends an apply that rounded stochastically: every kernel before it on the
// stream has read sr[1], the next apply (or graph replay) reads the new one.
__global__ void sr_advance_step(int64_t* __restrict__ sr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) sr[1] = sr[1] + 1;
}

// Begins a lazy-Adam apply: t = ++step[0] and a_t[0] = lr * sqrt(1 - b2^t) /
// (1 - b1^t), the powers in double.  Every update kernel after it on the
// stream reads a_t where the other rules read lr, so all of one apply see the
// same t, and the next apply (or graph replay) the next one.
__global__ void adam_advance_step(int64_t* __restrict__ step,
                                  const float* __restrict__ lr_ptr,
                                  float* __restrict__ a_t, double b1,
                                  double b2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t t = step[0] + 1;
  step[0] = t;
  a_t[0] = (float)((double)*lr_ptr * sqrt(1.0 - pow(b2, (double)t)) /
                   (1.0 - pow(b1, (double)t)));
}

static AdamArgs adam_args(const AdamConfig* adam, int width) {
  if (!adam) return {0.f, 0.f, 0.f, 0.f, 0};
  return {(float)adam->b1, (float)adam->b2, (float)(1.0 - adam->b1),
          (float)(1.0 - adam->b2), adam->vocab * (int64_t)width};
}

template <bool SR, typename PT, typename GT>
static void launch_sorted_optimizer_update_t(
    PT* weight, float* state, float eps, const int64_t* sorted_ids,
    const int64_t* seg, const int64_t* srow, const float* sw,
    const GT* grad_out, const float* lr, const int32_t* nu_ptr,
    int64_t max_segs, int width, int64_t* long_rows, int32_t* long_count,
    int64_t* work_items, int32_t* n_work, float* long_scratch, int rule,
    bool rowwise, const int64_t* sr, AdamArgs ad, const DetBuffers& det,
    hipStream_t stream) {
  const dim3 block(256);
  const bool deterministic = det.slab != nullptr;
  // bf16 weights have no atomicAdd: their long-SGD path also goes through the
  // fp32 scratch + finalize pair.  So does every rule in deterministic mode,
  // where the combine completes the scratch rows.
  const bool use_scratch = deterministic || rule != RULE_SGD ||
                           !std::is_same<PT, float>::value;
  dispatch_width(width, [&](auto tile, auto vec) {
    constexpr int TILE = decltype(tile)::value, VEC = decltype(vec)::value;
    const RowTiling t = row_tiling<TILE, VEC>(width, max_segs);
    const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
    dispatch_bool(sw != nullptr, [&](auto has_w_t) {
      constexpr bool HAS_W = decltype(has_w_t)::value;
      if (rowwise) {
        hipLaunchKernelGGL(
            (sorted_opt_update_rowwise<TILE, VEC, HAS_W, SR, PT, GT>), grid,
            block, 0, stream, weight, state, eps, sorted_ids, seg, srow, sw,
            grad_out, lr, nu_ptr, (int64_t)LONG_T, width, long_rows,
            long_count, t.tile_w, sr);
      } else {
        dispatch_rule(rule, [&](auto rule_t) {
          hipLaunchKernelGGL(
              (sorted_opt_update<TILE, VEC, HAS_W, decltype(rule_t)::value, SR,
                                 PT, GT>),
              grid, block, 0, stream, weight, state, eps, sorted_ids, seg,
              srow, sw, grad_out, lr, nu_ptr, (int64_t)LONG_T, width,
              long_rows, long_count, t.tile_w, sr, ad);
        });
      }
      if (deterministic) {
        hipLaunchKernelGGL(expand_long_work<true>, dim3(512), block, 0, stream,
                           long_rows, long_count, seg, work_items, n_work,
                           det.work_base);
        hipLaunchKernelGGL(
            (sorted_opt_long<TILE, VEC, HAS_W, true, true, GT>), dim3(2048),
            block, 0, stream, det.slab, sorted_ids, seg, srow, sw, grad_out,
            lr, width, long_rows, work_items, n_work, t.tile_w);
        launch_slab_combine<true>(det, long_scratch, width, long_rows,
                                  long_count, seg, work_items, n_work, stream);
        return;
      }
      hipLaunchKernelGGL(expand_long_work<false>, dim3(512), block, 0, stream,
                         long_rows, long_count, seg, work_items, n_work,
                         (int32_t*)nullptr);
      dispatch_bool(use_scratch, [&](auto to_scratch) {
        constexpr bool TO_SCRATCH = decltype(to_scratch)::value;
        hipLaunchKernelGGL(
            (sorted_opt_long<TILE, VEC, HAS_W, TO_SCRATCH, false, GT>),
            dim3(2048), block, 0, stream,
            TO_SCRATCH ? long_scratch : (float*)weight, sorted_ids, seg, srow,
            sw, grad_out, lr, width, long_rows, work_items, n_work, t.tile_w);
      });
    });
    if (rowwise)
      hipLaunchKernelGGL((sorted_long_finalize_rowwise<SR, PT>), dim3(256),
                         block, 0, stream, weight, state, eps, sorted_ids, seg,
                         lr, width, long_rows, long_count, long_scratch, sr);
    else if (use_scratch)
      dispatch_rule(rule, [&](auto rule_t) {
        hipLaunchKernelGGL(
            (sorted_long_finalize<decltype(rule_t)::value, SR, PT>), dim3(256),
            block, 0, stream, weight, state, eps, sorted_ids, seg, lr, width,
            long_rows, long_count, long_scratch, sr, ad);
      });
  });
}

void launch_sorted_optimizer_update(void* weight, bool weight_bf16,
                                    float* state, float eps,
                                    const int64_t* sorted_ids,
                                    const int64_t* seg, const int64_t* srow,
                                    const float* sw, const void* grad_out,
                                    bool grad_bf16,
                                    const float* lr, const int32_t* nu_ptr,
                                    int64_t max_segs, int width,
                                    int64_t* long_rows, int32_t* long_count,
                                    int64_t* work_items, int32_t* n_work,
                                    float* long_scratch, int64_t scratch_rows,
                                    bool adagrad, bool rowwise, int64_t* sr,
                                    const AdamConfig* adam, float* det_slab,
                                    int32_t* det_work_base,
                                    hipStream_t stream) {
  if (!weight_bf16) sr = nullptr;  // fp32 tables do not round
  const int rule = adam ? RULE_ADAM : adagrad ? RULE_ADAGRAD : RULE_SGD;
  const DetBuffers det{det_slab, det_work_base};
  if (adam) {
    hipLaunchKernelGGL(adam_advance_step, dim3(1), dim3(WAVE), 0, stream,
                       adam->step, lr, adam->a_t, adam->b1, adam->b2);
    lr = adam->a_t;
  }
  hipMemsetAsync(long_count, 0, sizeof(int32_t), stream);
  hipMemsetAsync(n_work, 0, sizeof(int32_t), stream);
  // the deterministic combine stores whole scratch rows: nothing to zero
  if (long_scratch && !det.slab) {
    hipMemsetAsync(long_scratch, 0,
                   sizeof(float) * scratch_rows * (int64_t)width, stream);
  }
  dispatch_bool(weight_bf16, [&](auto w_bf16) {
    dispatch_bool(grad_bf16, [&](auto g_bf16) {
      using PT = storage_t<decltype(w_bf16)>;
      using GT = storage_t<decltype(g_bf16)>;
      dispatch_sr<PT>(sr, [&](auto sr_t) {
        launch_sorted_optimizer_update_t<decltype(sr_t)::value>(
            (PT*)weight, state, eps, sorted_ids, seg, srow, sw,
            (const GT*)grad_out, lr, nu_ptr, max_segs, width, long_rows,
            long_count, work_items, n_work, long_scratch, rule,
            rowwise && !adam, sr, adam_args(adam, width), det, stream);
      });
    });
  });
  if (sr)
    hipLaunchKernelGGL(sr_advance_step, dim3(1), dim3(WAVE), 0, stream, sr);
}

// ---------------------------------------------------------------------------
// Gradient of the per-id weights: dw[k] = c_r * <grad_out[r(k)], table[i_k]>,
// c_r = 1/len for MEAN and 1 otherwise; exactly 0 for an id outside
// [0, vocab).
// ---------------------------------------------------------------------------

// Id-parallel: one lane group per position k, so a long bag needs no long
// path and nothing is combined with atomics.  Tiling is the forward's: narrow
// (TILE > 0) gives TILE lanes to a position and 64/TILE positions to a wave;
// wide gives tile_w lanes x VEC columns and walks the row in n_pass column
// passes.  Each lane forms its partial dot product in fp32 and tile_sum folds
// the group in a fixed order, so two calls agree bitwise.  The position loop
// and the column loop have wave-uniform trip counts; a group past the end or
// with an out-of-range id stays in step with live == false, because the
// lanes of one wave shuffle together.  row_ids is launch_expand_row_ids'.
template <int TILE, int VEC, bool MEAN, typename PT, typename GT>
__global__ void csr_weight_grad(const PT* __restrict__ params,
                                const GT* __restrict__ grad_out,
                                const int64_t* __restrict__ values,
                                const int32_t* __restrict__ row_ids,
                                const int64_t* __restrict__ splits,
                                float* __restrict__ dw, int64_t nnz,
                                int64_t vocab, int width, int tile_w) {
  const WaveCoord wc = wave_coord();
  const TileCoord tc = tile_coord(wc.lane, TILE > 0 ? TILE : tile_w);
  for (int64_t base = wc.wave_id * tc.rpw; base < nnz;
       base += wc.n_waves * tc.rpw) {
    const int64_t k = base + tc.sub;
    int64_t id = -1, row = 0;
    if (k < nnz) {
      id = values[k];
      row = row_ids[k];
    }
    const bool live = id >= 0 && id < vocab;
    const PT* trow = params + (live ? id : 0) * (int64_t)width;
    const GT* grow = grad_out + row * (int64_t)width;
    float dot = 0.f;
    if constexpr (TILE > 0) {
      if (live && tc.tl < width)
        dot = pt_load(&grow[tc.tl]) * pt_load(&trow[tc.tl]);
      dot = tile_sum(dot, TILE);
    } else {
      const int pass_w = tile_w * VEC;
      const int n_pass = (width + pass_w - 1) / pass_w;
      for (int p = 0; p < n_pass; ++p) {
        const int col0 = p * pass_w + tc.tl * VEC;
        if (live && col0 < width) {
          float g[VEC], t[VEC];
          pt_loadv<VEC>(grow + col0, g);
          pt_loadv<VEC>(trow + col0, t);
#pragma unroll
          for (int v = 0; v < VEC; ++v) dot += g[v] * t[v];
        }
      }
      dot = tile_sum(dot, tile_w);
    }
    if (k < nnz && tc.tl == 0) {
      float c = 1.f;
      if (MEAN && live) c = 1.f / (float)(splits[row + 1] - splits[row]);
      dw[k] = live ? c * dot : 0.f;
    }
  }
}

void launch_csr_weight_grad(const void* params, bool params_bf16,
                            const void* grad_out, bool grad_bf16,
                            const int64_t* values, const int32_t* row_ids,
                            const int64_t* splits, bool mean, float* dw,
                            int64_t nnz, int64_t vocab, int width,
                            hipStream_t stream) {
  const dim3 block(256);
  dispatch_width(width, [&](auto tile, auto vec) {
    constexpr int TILE = decltype(tile)::value, VEC = decltype(vec)::value;
    const RowTiling t = row_tiling<TILE, VEC>(width, nnz);
    const dim3 grid(pick_grid(t.row_waves, block.x / WAVE));
    dispatch_bool(params_bf16, [&](auto p_bf16) {
      dispatch_bool(grad_bf16, [&](auto g_bf16) {
        dispatch_bool(mean, [&](auto mean_t) {
          using PT = storage_t<decltype(p_bf16)>;
          using GT = storage_t<decltype(g_bf16)>;
          hipLaunchKernelGGL(
              (csr_weight_grad<TILE, VEC, decltype(mean_t)::value, PT, GT>),
              grid, block, 0, stream, (const PT*)params, (const GT*)grad_out,
              values, row_ids, splits, dw, nnz, vocab, width, t.tile_w);
        });
      });
    });
  });
}

// ---------------------------------------------------------------------------
// Fused sparse optimizer steps: apply (unique_ids, unique_grad) rows directly
// to the table — no torch sparse re-coalesce, no dense grad materialization.
// One wave per row.
// ---------------------------------------------------------------------------

template <int RULE, bool SR, typename PT>
__global__ void sparse_row_update(PT* __restrict__ weight,
                                  float* __restrict__ state,
                                  const int64_t* __restrict__ ids,
                                  const float* __restrict__ grad,
                                  int64_t num_rows, int width, float lr,
                                  float eps,
                                  const int64_t* __restrict__ sr_ptr,
                                  AdamArgs ad) {
  const WaveCoord wc = wave_coord();
  const SrState sr = sr_load<SR>(sr_ptr);
  for (int64_t r = wc.wave_id; r < num_rows; r += wc.n_waves) {
    const int64_t row0 = ids[r] * (int64_t)width;
    for (int c = wc.lane; c < width; c += WAVE) {
      const int64_t o = row0 + c;
      apply_row_update<RULE>(&weight[o],
                             RULE != RULE_SGD ? &state[o] : nullptr,
                             grad[r * (int64_t)width + c], lr, eps, sr,
                             sr_group_hash(sr, o), o, ad);
    }
  }
}

// Row-wise Adagrad: state is [vocab], one float per row.
template <bool SR, typename PT>
__global__ void sparse_row_update_rowwise(PT* __restrict__ weight,
                                          float* __restrict__ state,
                                          const int64_t* __restrict__ ids,
                                          const float* __restrict__ grad,
                                          int64_t num_rows, int width,
                                          float lr, float eps,
                                          const int64_t* __restrict__ sr_ptr) {
  const WaveCoord wc = wave_coord();
  const SrState sr = sr_load<SR>(sr_ptr);
  for (int64_t r = wc.wave_id; r < num_rows; r += wc.n_waves) {
    const int64_t uid = ids[r];
    rowwise_wave_update(weight + uid * (int64_t)width, &state[uid],
                        grad + r * (int64_t)width, width, wc.lane, lr, eps, sr,
                        uid * (int64_t)width);
  }
}

void launch_sparse_row_update(void* weight, bool weight_bf16, float* state,
                              const int64_t* ids, const float* grad,
                              int64_t num_rows, int width, float lr, float eps,
                              bool adagrad, bool rowwise, int64_t* sr,
                              const AdamConfig* adam, hipStream_t stream) {
  const int block = 256;
  const int grid = pick_grid(num_rows, block / WAVE);
  if (!weight_bf16) sr = nullptr;  // fp32 tables do not round
  const int rule = adam ? RULE_ADAM : adagrad ? RULE_ADAGRAD : RULE_SGD;
  const AdamArgs ad = adam_args(adam, width);
  if (adam) rowwise = false;
  dispatch_bool(weight_bf16, [&](auto w_bf16) {
    using PT = storage_t<decltype(w_bf16)>;
    dispatch_sr<PT>(sr, [&](auto sr_t) {
      constexpr bool SR = decltype(sr_t)::value;
      if (rowwise) {
        hipLaunchKernelGGL((sparse_row_update_rowwise<SR, PT>), dim3(grid),
                           dim3(block), 0, stream, (PT*)weight, state, ids,
                           grad, num_rows, width, lr, eps, sr);
        return;
      }
      dispatch_rule(rule, [&](auto rule_t) {
        hipLaunchKernelGGL(
            (sparse_row_update<decltype(rule_t)::value, SR, PT>), dim3(grid),
            dim3(block), 0, stream, (PT*)weight, state, ids, grad, num_rows,
            width, lr, eps, sr, ad);
      });
    });
  });
  if (sr)
    hipLaunchKernelGGL(sr_advance_step, dim3(1), dim3(WAVE), 0, stream, sr);
}

// ---------------------------------------------------------------------------
// Stand-alone stochastic rounding: out[i] = SR(x[i]) with the bits of table
// offset base_offset + i.  Any n and any base_offset, so one hash per element.
// ---------------------------------------------------------------------------
__global__ void stochastic_round_bf16_kernel(const float* __restrict__ x,
                                             bf16_t* __restrict__ out,
                                             int64_t n, uint64_t seed,
                                             uint64_t step,
                                             int64_t base_offset) {
  const uint64_t key = sr_key(seed, step);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const int64_t o = base_offset + i;
    out[i].b = bf16_sr_bits(x[i], sr_pick(sr_hash(key, o), o));
  }
}

void launch_stochastic_round_bf16(const float* x, void* out, int64_t n,
                                  int64_t seed, int64_t step,
                                  int64_t base_offset, hipStream_t stream) {
  if (n <= 0) return;
  const int block = 256;
  int64_t grid = cdiv64(n, block);
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(stochastic_round_bf16_kernel, dim3((int)grid),
                     dim3(block), 0, stream, x, (bf16_t*)out, n,
                     (uint64_t)seed, (uint64_t)step, base_offset);
}

// ---------------------------------------------------------------------------
// IntegerLookup hash (open addressing, linear probe, device-scope atomics).
// Slots come from mix64 (top of the file).
// ---------------------------------------------------------------------------

// Pass 1: free values (counts[v]==0) -> avail list, ascending via scanned pos.
__global__ void mark_free_values(const int32_t* __restrict__ counts, int64_t n,
                                 int32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] = counts[i] == 0 ? 1 : 0;
}

__global__ void scatter_free_values(const int32_t* __restrict__ flags,
                                    const int32_t* __restrict__ pos, int64_t n,
                                    int64_t* __restrict__ avail,
                                    int32_t* __restrict__ navail) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) avail[pos[i] - 1] = i;
  if (i == n - 1) *navail = pos[i];
}

// Pass 2a: insert.  Claims key slots with 64-bit device-scope CAS
// (EMPTY = -1) and assigns fresh values; NO spin-waiting — a lane that loses
// the CAS to its own key simply stops (the winner's value write becomes
// visible at the kernel boundary, read by pass 2b).  An intra-wave
// winner/spinner pair would deadlock under wave64 branch serialization, so
// the insert/find split is load-bearing, not a style choice.
#define IL_EMPTY (-1ll)

__global__ void hash_insert(const int64_t* __restrict__ keys, int64_t n,
                            int64_t* __restrict__ tkeys,
                            int64_t* __restrict__ tvals, int64_t capacity,
                            const int64_t* __restrict__ avail,
                            const int32_t* __restrict__ navail,
                            int32_t* __restrict__ next_avail) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = keys[i];
  // key == EMPTY is the OOV token: no slot, no value (a CAS of EMPTY over
  // EMPTY would "claim" a slot that stays empty and still draw a value)
  if (key == IL_EMPTY) return;
  uint64_t slot = mix64((uint64_t)key) % (uint64_t)capacity;
  for (int64_t probe = 0; probe < capacity; ++probe) {
    int64_t prev = (int64_t)atomicCAS((unsigned long long*)&tkeys[slot],
                                      (unsigned long long)IL_EMPTY,
                                      (unsigned long long)key);
    if (prev == IL_EMPTY) {
      // claimed: draw the next free value (or 0 = OOV when full)
      const int32_t a = atomicAdd(next_avail, 1);
      tvals[slot] = (a < *navail) ? avail[a] : 0;
      return;
    }
    if (prev == key) return;  // someone else inserted this key
    slot = (slot + 1) % (uint64_t)capacity;
  }
}

// Pass 2b: find (all values final after the insert kernel) + frequency count.
__global__ void hash_find(const int64_t* __restrict__ keys, int64_t n,
                          const int64_t* __restrict__ tkeys,
                          const int64_t* __restrict__ tvals, int64_t capacity,
                          int32_t* __restrict__ counts,
                          int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = keys[i];
  uint64_t slot = mix64((uint64_t)key) % (uint64_t)capacity;
  int64_t value = 0;
  // the OOV token (key == EMPTY) is value 0 without probing: it would match
  // the first empty slot and read that slot's unowned tvals
  for (int64_t probe = 0; key != IL_EMPTY && probe < capacity; ++probe) {
    const int64_t k = tkeys[slot];
    if (k == key) {
      value = tvals[slot];
      break;
    }
    if (k == IL_EMPTY) break;  // absent (insert failed: table full)
    slot = (slot + 1) % (uint64_t)capacity;
  }
  atomicAdd(&counts[value], 1);
  out[i] = value;
}

// Rehash: re-insert every occupied (key, value) pair of the old table into a
// larger (sentinel-initialized) one, PRESERVING values.  Keys are unique in
// the old table, so CAS races are only slot contention between different
// keys — the loser probes on; no spin-waits (same wave64 deadlock rationale
// as hash_insert above).
__global__ void hash_reinsert(const int64_t* __restrict__ old_keys,
                              const int64_t* __restrict__ old_vals,
                              int64_t old_cap, int64_t* __restrict__ tkeys,
                              int64_t* __restrict__ tvals, int64_t capacity) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_cap) return;
  const int64_t key = old_keys[i];
  // drop value-0 entries: those are overflow keys hash_insert claimed while
  // the table was full — after growth they must re-insert with a REAL value
  // (keeping them would pin the key to OOV forever)
  if (key == IL_EMPTY || old_vals[i] == 0) return;
  uint64_t slot = mix64((uint64_t)key) % (uint64_t)capacity;
  for (int64_t probe = 0; probe < capacity; ++probe) {
    int64_t prev = (int64_t)atomicCAS((unsigned long long*)&tkeys[slot],
                                      (unsigned long long)IL_EMPTY,
                                      (unsigned long long)key);
    if (prev == IL_EMPTY) {
      tvals[slot] = old_vals[i];
      return;
    }
    slot = (slot + 1) % (uint64_t)capacity;
  }
}

void launch_hash_reinsert(const int64_t* old_keys, const int64_t* old_vals,
                          int64_t old_cap, int64_t* tkeys, int64_t* tvals,
                          int64_t capacity, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(hash_reinsert, dim3((int)cdiv64(old_cap, block)),
                     dim3(block), 0, stream, old_keys, old_vals, old_cap,
                     tkeys, tvals, capacity);
}

void launch_integer_lookup(const int64_t* keys, int64_t n, int64_t* tkeys,
                           int64_t* tvals, int64_t capacity, int32_t* counts,
                           int64_t max_tokens, void* temp, size_t temp_bytes,
                           int32_t* scratch_flags, int32_t* scratch_pos,
                           int64_t* avail, int32_t* navail, int32_t* next_avail,
                           int64_t* out, hipStream_t stream) {
  const int block = 256;
  const int64_t nvals = max_tokens + 1;
  hipLaunchKernelGGL(mark_free_values, dim3((int)cdiv64(nvals, block)),
                     dim3(block), 0, stream, counts, nvals, scratch_flags);
  rocprim::inclusive_scan(temp, temp_bytes, scratch_flags, scratch_pos,
                          (size_t)nvals, rocprim::plus<int32_t>(), stream);
  hipLaunchKernelGGL(scatter_free_values, dim3((int)cdiv64(nvals, block)),
                     dim3(block), 0, stream, scratch_flags, scratch_pos, nvals,
                     avail, navail);
  hipMemsetAsync(next_avail, 0, sizeof(int32_t), stream);
  hipLaunchKernelGGL(hash_insert, dim3((int)cdiv64(n, block)), dim3(block), 0,
                     stream, keys, n, tkeys, tvals, capacity, avail, navail,
                     next_avail);
  hipLaunchKernelGGL(hash_find, dim3((int)cdiv64(n, block)), dim3(block), 0,
                     stream, keys, n, tkeys, tvals, capacity, counts, out);
}

size_t integer_lookup_temp_bytes(int64_t max_tokens) {
  size_t scan_bytes = 0;
  rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr,
                          (int32_t*)nullptr, (size_t)(max_tokens + 1));
  return scan_bytes;
}
