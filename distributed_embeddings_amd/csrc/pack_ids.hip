// pack_ids: writes the flat id vector of one fused lookup group in one pass.
//
// A group's CSR values are the ids of all its (input, slice) pairs, one pair
// after the other, each shifted by the pair's row offset into the fused
// table.  Each pair is one *segment* of the launch:
//
//   copy    src [rows, h_out]   dst[dst_begin + r*h_out + k] = src[r, k] + offset
//   expand  src [rows]          dst[dst_begin + r*h_out + k] = bag(src[r])[k] + offset
//
// with bag() the multi-hot expansion of ops/embedding_lookup.py
// (multi_hot_expand), all arithmetic mod 2^64:
//
//   inner  = mix64(key_f + x)
//   bag[0] = x
//   bag[k] = mix64(inner + k) % vocab        k = 1 .. h_out-1, unsigned
//
// and an id outside [0, vocab) copied to every slot unhashed.
//
// Segment descriptors travel by value in the kernel argument block (no
// descriptor tensor, no host-to-device copy), so a launch is hipGraph
// capturable as it stands.  blockIdx.y selects the segment: the descriptor is
// wave-uniform and stays in scalar registers, and a block never straddles two
// segments.  Every thread writes two adjacent ids with one 16-byte store; a
// segment whose first destination element is not 16-byte aligned writes that
// element alone first, and an odd remainder goes out as one 8-byte store.
// wave64, plain vector stores, no LDS, no atomics.

#include <hip/hip_runtime.h>

#include "ops_api.h"

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t k) {
  // splitmix64 finalizer, as in embedding_ops.hip
  k += 0x9E3779B97F4A7C15ull;
  k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
  k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
  return k ^ (k >> 31);
}

struct PackIdsArgs {
  PackIdsSegment seg[kPackIdsMaxSegments];
};
static_assert(sizeof(PackIdsArgs) + 16 <= 4096,
              "pack_ids argument block must stay under 4 KB");

constexpr int kThreads = 256;

struct alignas(16) IdPair {
  int64_t a, b;
};

// element e of the segment: r = e / h, k = e % h.  `narrow` (uniform) means
// the segment has fewer than 2^32 elements and a 32-bit divide will do.
__device__ __forceinline__ void row_and_slot(int64_t e, uint32_t h, bool narrow,
                                             int64_t* r, uint32_t* k) {
  if (narrow) {
    const uint32_t e32 = (uint32_t)e;
    const uint32_t q = e32 / h;
    *r = q;
    *k = e32 - q * h;
  } else {
    const int64_t q = e / (int64_t)h;
    *r = q;
    *k = (uint32_t)(e - q * (int64_t)h);
  }
}

__device__ __forceinline__ int64_t expand_slot(int64_t x, uint32_t k,
                                               uint64_t vocab,
                                               uint64_t key_f) {
  if (k == 0 || (uint64_t)x >= vocab) return x;
  const uint64_t inner = mix64(key_f + (uint64_t)x);
  return (int64_t)(mix64(inner + k) % vocab);
}

__global__ void __launch_bounds__(kThreads)
pack_ids_kernel(PackIdsArgs args, int64_t* __restrict__ dst) {
  const PackIdsSegment& s = args.seg[blockIdx.y];
  const int64_t n = s.rows * (int64_t)s.h_out;
  if (n <= 0) return;
  const int64_t* __restrict__ src = s.src;
  int64_t* __restrict__ out = dst + s.dst_begin;
  const int64_t offset = s.offset;
  const uint32_t h = (uint32_t)s.h_out;
  const bool expand = s.mode == kPackIdsExpand;
  const uint64_t vocab = (uint64_t)s.vocab;
  const uint64_t key_f = s.key_f;
  const bool narrow = n < ((int64_t)1 << 32);

  // one leading element when out is 8- but not 16-byte aligned
  const int64_t head = (reinterpret_cast<uintptr_t>(out) >> 3) & 1;
  const int64_t npairs = (n - head) >> 1;
  const bool tail = ((n - head) & 1) != 0;

  auto value_at = [&](int64_t e) -> int64_t {
    if (!expand) return src[e] + offset;
    int64_t r;
    uint32_t k;
    row_and_slot(e, h, narrow, &r, &k);
    return expand_slot(src[r], k, vocab, key_f) + offset;
  };

  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) out[0] = value_at(0);
    if (tail) out[n - 1] = value_at(n - 1);
  }

  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (!expand) {
    const bool src16 =
        (reinterpret_cast<uintptr_t>(src + head) & 15) == 0;
    for (; p < npairs; p += stride) {
      const int64_t e = head + 2 * p;
      IdPair v;
      if (src16) {
        v = *reinterpret_cast<const IdPair*>(src + e);
      } else {
        v.a = src[e];
        v.b = src[e + 1];
      }
      v.a += offset;
      v.b += offset;
      *reinterpret_cast<IdPair*>(out + e) = v;
    }
    return;
  }
  for (; p < npairs; p += stride) {
    const int64_t e = head + 2 * p;
    int64_t r;
    uint32_t k;
    row_and_slot(e, h, narrow, &r, &k);
    const int64_t x0 = src[r];
    // the pair's second element is the next slot of the same row, or slot 0
    // of the next row (e + 1 < n, so that row exists)
    uint32_t k1 = k + 1;
    int64_t x1 = x0;
    if (k1 == h) {
      k1 = 0;
      x1 = src[r + 1];
    }
    IdPair v;
    v.a = expand_slot(x0, k, vocab, key_f) + offset;
    v.b = expand_slot(x1, k1, vocab, key_f) + offset;
    *reinterpret_cast<IdPair*>(out + e) = v;
  }
}

}  // namespace

void launch_pack_ids(const PackIdsSegment* segs, int nseg, int64_t* dst,
                     hipStream_t stream) {
  for (int first = 0; first < nseg; first += kPackIdsMaxSegments) {
    const int count = nseg - first < kPackIdsMaxSegments
                          ? nseg - first : kPackIdsMaxSegments;
    PackIdsArgs args{};
    int64_t max_n = 0;
    for (int i = 0; i < count; ++i) {
      args.seg[i] = segs[first + i];
      const int64_t n = segs[first + i].rows * (int64_t)segs[first + i].h_out;
      if (n > max_n) max_n = n;
    }
    if (max_n <= 0) continue;
    // four pairs per thread at most until the cap; blocks of a shorter
    // segment past its end return at once
    const int64_t per_block = (int64_t)kThreads * 2 * 4;
    int64_t bx = (max_n + per_block - 1) / per_block;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(pack_ids_kernel, dim3((unsigned)bx, (unsigned)count),
                       dim3(kThreads), 0, stream, args, dst);
  }
}
