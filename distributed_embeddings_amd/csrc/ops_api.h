// Internal launcher API between embedding_ops.hip (kernels) and bindings.cpp
// (torch glue).  gfx950-only; no CUDA-compat paths.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

void launch_csr_lookup_forward(const void* params, bool params_bf16,
                               const int64_t* values, const int64_t* splits,
                               const float* per_id_w, void* out, bool out_bf16,
                               int64_t num_rows, int64_t nnz, int64_t vocab,
                               int width, bool mean, int64_t* long_rows,
                               int32_t* long_count, int64_t* work_items,
                               int32_t* n_work, float* det_slab,
                               int32_t* det_work_base, hipStream_t stream);

// Deterministic mode (all forwards and launch_sorted_optimizer_update):
// det_slab, fp32 [work_items capacity, width], and det_work_base, int32
// [long_rows capacity], select it; both null keep the atomic long-row
// combine.  With them every long row's 128-id chunk partials go to the slab
// and are added in a fixed order (docs/KERNELS.md), bf16-out forwards split
// long rows like fp32-out ones, and no float atomic is issued.

// int8 row-wise quantized tables.  packed is [vocab, width + 8] bytes: per
// row width bytes q, fp32 scale, fp32 bias; the row stands for
// scale * q + bias.  width % 4 == 0, and the forward needs vocab > 0.
void launch_csr_lookup_forward_q8(const void* packed, const int64_t* values,
                                  const int64_t* splits, const float* per_id_w,
                                  void* out, bool out_bf16, int64_t num_rows,
                                  int64_t nnz, int64_t vocab, int width,
                                  bool mean, int64_t* long_rows,
                                  int32_t* long_count, int64_t* work_items,
                                  int32_t* n_work, float* det_slab,
                                  int32_t* det_work_base, hipStream_t stream);
// in: [n, width] fp32 or bf16, aligned to four elements; packed:
// [n, width + 8].
void launch_quantize_rows_q8(const void* in, bool in_bf16, void* packed,
                             int64_t n, int width, hipStream_t stream);
void launch_dequantize_rows_q8(const void* packed, float* out, int64_t n,
                               int width, hipStream_t stream);

// int4 row-wise quantized tables.  packed is [vocab, width / 2 + 4] bytes: per
// row width / 2 bytes of nibbles (column 2j low, 2j + 1 high), fp16 scale,
// fp16 bias; the row stands for scale * q + bias.  width % 8 == 0, and the
// forward needs vocab > 0.
void launch_csr_lookup_forward_q4(const void* packed, const int64_t* values,
                                  const int64_t* splits, const float* per_id_w,
                                  void* out, bool out_bf16, int64_t num_rows,
                                  int64_t nnz, int64_t vocab, int width,
                                  bool mean, int64_t* long_rows,
                                  int32_t* long_count, int64_t* work_items,
                                  int32_t* n_work, float* det_slab,
                                  int32_t* det_work_base, hipStream_t stream);
// in: [n, width] fp32 or bf16, aligned to four elements; packed:
// [n, width / 2 + 4].
void launch_quantize_rows_q4(const void* in, bool in_bf16, void* packed,
                             int64_t n, int width, hipStream_t stream);
void launch_dequantize_rows_q4(const void* packed, float* out, int64_t n,
                               int width, hipStream_t stream);

void launch_row_to_split(const int64_t* rows, int64_t nnz, int64_t num_rows,
                         int64_t* splits, hipStream_t stream);

size_t csr_backward_temp_bytes(int64_t nnz);

// Writes row_ids[k] and, when mean || user_w, w[k] = c_r * user_w[k] with
// c_r = 1/len for mean and 1 otherwise (user_w == nullptr counts as ones).
void launch_expand_row_ids(const int64_t* splits, int64_t num_rows,
                           int64_t nnz, int32_t* row_ids, float* w, bool mean,
                           const float* user_w, hipStream_t stream);

// dw[k] = c_r * <grad_out[row_ids[k]], params[values[k]]>, 0 for an id
// outside [0, vocab).  row_ids comes from launch_expand_row_ids.
void launch_csr_weight_grad(const void* params, bool params_bf16,
                            const void* grad_out, bool grad_bf16,
                            const int64_t* values, const int32_t* row_ids,
                            const int64_t* splits, bool mean, float* dw,
                            int64_t nnz, int64_t vocab, int width,
                            hipStream_t stream);

hipError_t run_inclusive_scan_i32(void* temp, size_t temp_bytes,
                                  const int32_t* in, int32_t* out, int64_t n,
                                  hipStream_t stream);

void launch_mark_heads(const int64_t* sorted_ids, int64_t n, int64_t vocab,
                       int32_t* head, hipStream_t stream);

void launch_scatter_unique(const int64_t* sorted_ids, const int32_t* head,
                           const int32_t* pos, int64_t n, int64_t* unique_ids,
                           int64_t* seg_offsets, int32_t* num_unique,
                           hipStream_t stream);

void launch_gather_sorted(const int32_t* perm, const int32_t* row_ids,
                          const float* w, int64_t n, int64_t* srow, float* sw,
                          hipStream_t stream);

// *valid_end = first sorted position holding an out-of-vocabulary id.
void launch_find_valid_bounds(const int64_t* sorted_ids, int64_t n,
                              int64_t vocab, int64_t* valid_end,
                              hipStream_t stream);

void launch_set_seg_end(int64_t* seg_offsets, const int32_t* num_unique,
                        const int64_t* valid_end, hipStream_t stream);

void launch_integer_lookup(const int64_t* keys, int64_t n, int64_t* tkeys,
                           int64_t* tvals, int64_t capacity, int32_t* counts,
                           int64_t max_tokens, void* temp, size_t temp_bytes,
                           int32_t* scratch_flags, int32_t* scratch_pos,
                           int64_t* avail, int32_t* navail, int32_t* next_avail,
                           int64_t* out, hipStream_t stream);

size_t integer_lookup_temp_bytes(int64_t max_tokens);

void launch_hash_reinsert(const int64_t* old_keys, const int64_t* old_vals,
                          int64_t old_cap, int64_t* tkeys, int64_t* tvals,
                          int64_t capacity, hipStream_t stream);

void launch_pad_seg_offsets(int64_t* seg, int64_t n, const int32_t* num_unique,
                            const int64_t* valid_end, hipStream_t stream);

// Lazy Adam.  state is then fp32 [2, vocab, width], m first, and adagrad and
// rowwise are ignored.  launch_sorted_optimizer_update: a leading one-thread
// kernel sets t = ++step[0] and a_t[0] = lr * sqrt(1 - b2^t) / (1 - b1^t) on
// the device (step: int64 [1], a_t: one float of scratch) and the update
// kernels read a_t in place of lr.  launch_sparse_row_update leaves step and
// a_t alone: its caller passes a_t as lr.
struct AdamConfig {
  double b1, b2;
  int64_t vocab;
  int64_t* step;
  float* a_t;
};

// adam == nullptr selects SGD or Adagrad by the flags.
// rowwise (row-wise Adagrad) takes state as [vocab] fp32, one float per row,
// in place of Adagrad's [vocab, width]; it implies adagrad.
// sr: device pointer to {seed, step}, or nullptr.  With a bf16 weight it
// selects stochastic rounding of the weight stores; every kernel of the call
// reads the same step and a trailing one-thread kernel adds 1 to it, which is
// why the pointer is not const.  nullptr (and any fp32 weight) keeps
// round-to-nearest-even and launches nothing extra.
// det_slab / det_work_base: deterministic mode, see above.  long_scratch is
// then needed for every rule, fp32 SGD included.
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
                                    hipStream_t stream);

void launch_sparse_row_update(void* weight, bool weight_bf16, float* state,
                              const int64_t* ids, const float* grad,
                              int64_t num_rows, int width, float lr, float eps,
                              bool adagrad, bool rowwise, int64_t* sr,
                              const AdamConfig* adam, hipStream_t stream);

// out[i] = bf16 of x[i], stochastically rounded with the bits of table offset
// base_offset + i at (seed, step); out is bf16 [n].
void launch_stochastic_round_bf16(const float* x, void* out, int64_t n,
                                  int64_t seed, int64_t step,
                                  int64_t base_offset, hipStream_t stream);

// pack_ids.hip.  One segment of a pack_ids launch: the ids of one (input,
// slice) pair of a fused lookup group.  copy: src is [rows, h_out] and
// dst[dst_begin + r * h_out + k] = src[r, k] + offset.  expand: src is [rows]
// and the k-th id of row r is the multi-hot expansion of src[r] (see
// pack_ids.hip) + offset.  h_out >= 1; expand needs vocab >= 1.
constexpr int kPackIdsCopy = 0;
constexpr int kPackIdsExpand = 1;
constexpr int kPackIdsMaxSegments = 64;  // per launch: 56 bytes each, < 4 KB
struct PackIdsSegment {
  const int64_t* src;
  int64_t rows;
  int64_t dst_begin;
  int64_t vocab;
  uint64_t key_f;
  int64_t offset;
  int32_t h_out;
  int32_t mode;
};
// The segments go by value in the kernel arguments, kPackIdsMaxSegments per
// launch, so nseg above that takes several launches over consecutive
// segments.  Segments with rows == 0 are legal, and a call whose segments are
// all empty launches nothing.  dst must be 8-byte aligned.
void launch_pack_ids(const PackIdsSegment* segs, int nseg, int64_t* dst,
                     hipStream_t stream);

void launch_dot_interact_fwd_packed(const void* bottom, const void* packed,
                                    const int* perm, void* out, int64_t B,
                                    int F, int D, int out_w, int tri_n,
                                    int64_t sb, int64_t sp,
                                    hipStream_t stream);
void launch_dot_interact_bwd_packed(const void* gout, const void* bottom,
                                    const void* packed, const int* perm,
                                    void* gbottom, void* gpacked, int64_t B,
                                    int F, int D, int out_w, int tri_n,
                                    int64_t sb, int64_t sp,
                                    hipStream_t stream);
void launch_dot_interact_fwd(const void* feats, void* out, int64_t B, int F,
                             int D, int out_w, int tri_n, hipStream_t stream);
void launch_dot_interact_bwd(const void* gout, const void* feats, void* gfeats,
                             int64_t B, int F, int D, int out_w, int tri_n,
                             hipStream_t stream);
// The launchers above serve F <= 32 (D % 32 == 0); these serve 33 <= F <= 64
// with D % 32 == 0 and D <= 256, and throw std::invalid_argument outside that.
void launch_dot_interact_fwd_packed64(const void* bottom, const void* packed,
                                      const int* perm, void* out, int64_t B,
                                      int F, int D, int out_w, int tri_n,
                                      int64_t sb, int64_t sp,
                                      hipStream_t stream);
void launch_dot_interact_bwd_packed64(const void* gout, const void* bottom,
                                      const void* packed, const int* perm,
                                      void* gbottom, void* gpacked, int64_t B,
                                      int F, int D, int out_w, int tri_n,
                                      int64_t sb, int64_t sp,
                                      hipStream_t stream);
void launch_dot_interact_fwd64(const void* feats, void* out, int64_t B, int F,
                               int D, int out_w, int tri_n, hipStream_t stream);
void launch_dot_interact_bwd64(const void* gout, const void* feats,
                               void* gfeats, int64_t B, int F, int D,
                               int out_w, int tri_n, hipStream_t stream);

// mlp_ops.hip.  relu_bwd_bias_grad: grad_in = (y <= 0) ? 0 : grad_out and
// bias_grad = bf16(column sums of grad_in), bf16 [B, N] with N % 8 == 0.
// The plan gives the slab shape [num_chunks, N] fp32 the launcher needs.
void relu_bwd_bias_grad_plan(int64_t B, int N, int64_t* rows_per_chunk,
                             int64_t* num_chunks);
void launch_relu_bwd_bias_grad(const void* grad_out, const void* y,
                               void* grad_in, float* slab, void* bias_grad,
                               int64_t B, int N, int64_t rows_per_chunk,
                               int64_t num_chunks, hipStream_t stream);

// mlp_ops.hip.  cross_bwd, the elementwise backward of one low-rank cross
// layer x_{l+1} = x0 * u + x_l, all bf16 [B, N] with N % 8 == 0 and 16-byte
// aligned: gu = bf16(gout * x0), bias_grad = bf16(column sums of gu) and, in
// place, acc = bf16((init ? 0 : acc) + gout * u) formed in fp32.  init never
// reads acc.  Slab [num_chunks, N] fp32 from relu_bwd_bias_grad_plan.
void launch_cross_bwd(const void* gout, const void* x0, const void* u,
                      void* acc, bool init, void* gu, float* slab,
                      void* bias_grad, int64_t B, int N,
                      int64_t rows_per_chunk, int64_t num_chunks,
                      hipStream_t stream);

// cross_ops.hip.  x0 [B, (P+1)*D] = [bottom | packed rows in perm order]:
// x0[b, 0:D] = bottom[b], x0[b, f*D:(f+1)*D] = packed row perm[f-1] of sample
// b, at element offset (b*sb + perm[f-1]*sp)*D as in the packed dot
// interaction.  bf16, D % 8 == 0, 16-byte aligned.  The backward splits gx0
// into gbottom and gpacked; perm has to be a permutation of [0, P) for it to
// cover gpacked, and an entry outside [0, P) is skipped (zeros in x0).
void launch_cross_concat_fwd(const void* bottom, const void* packed,
                             const int* perm, void* x0, int64_t B, int P,
                             int D, int64_t sb, int64_t sp,
                             hipStream_t stream);
void launch_cross_concat_bwd(const void* gx0, const int* perm, void* gbottom,
                             void* gpacked, int64_t B, int P, int D,
                             int64_t sb, int64_t sp, hipStream_t stream);

// wgrad_splitk.hip.  gw [M, N] = bf16(g^T x) for bf16 g [K, M], x [K, N], fp32
// accumulation, one rounding: split-K partial products into the fp32 slab
// [splitk, M, np], then a fixed-order sum.  M % 8 == 0; N % 8 == 0 or N <= 16.
struct WgradSplitkPlan {
  int cfg;         // tile geometry
  int splitk;      // K-slices, none empty
  int64_t kslice;  // rows of g and x per slice
  int np;          // slab row length: N rounded up to 4
  bool use;        // route the MLP's weight gradient of this shape here
};
// false: the kernels do not take this shape
bool wgrad_splitk_plan(int64_t K, int64_t M, int64_t N, WgradSplitkPlan* plan);
// splitk >= 1 (capped at ceil(K / 64)) and tile >= 0 replace the plan's
// choices (tests, tuning)
bool wgrad_splitk_plan_with(int64_t K, int64_t M, int64_t N, int64_t splitk,
                            int tile, WgradSplitkPlan* plan);
void launch_wgrad_splitk(const void* g, const void* x, float* slab, void* gw,
                         int64_t K, int M, int N, const WgradSplitkPlan& plan,
                         hipStream_t stream);

size_t custom_radix_sort_hist_elems(int64_t n);
int custom_radix_sort_num_variants();
// keys per block of tile geometry `variant` in [0, num_variants)
int custom_radix_sort_variant_tile(int variant);

// variant -1: DE_SORT_VARIANT, then dispatch on n (production); a value in
// [0, num_variants) forces that tile geometry.  The caller rejects the rest.
void custom_radix_sort_keys(const uint64_t* keys_in, uint64_t* keys_out,
                            uint64_t* keys_tmp, int32_t* hist,
                            int32_t* scan_sums, int64_t n, int begin_bit,
                            int end_bit, int variant, hipStream_t stream);

void launch_mask_oob_pack(const int64_t* ids, int64_t n, int64_t vocab,
                          uint64_t* packed, hipStream_t stream);
void launch_unpack_sorted(const uint64_t* packed, int64_t n,
                          int64_t* sorted_ids, int32_t* sorted_pos,
                          hipStream_t stream);
hipError_t run_sort_keys_u64(void* temp, size_t temp_bytes,
                             const uint64_t* keys_in, uint64_t* keys_out,
                             int64_t n, int begin_bit, int end_bit,
                             hipStream_t stream);
size_t rocprim_sort_keys_temp_bytes(int64_t n);
