// Torch bindings for the gfx950 HIP kernels (in-tree extension
// distributed_embeddings_amd._hip_ops).  Host-side orchestration of the
// backward pipeline lives here (the one deliberate D2H sync: num_unique —
// parity with the reference GradFunctor, embedding_lookup_kernels.cu:663-667).

#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include "ops_api.h"

namespace {

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")

inline hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

int log2_ceil(int64_t v) {
  int b = 0;
  while ((int64_t(1) << b) < v) ++b;
  return b;
}


// Sort dispatch: hand-written LSD radix sort (csrc/radix_sort.hip) by
// default; DE_USE_ROCPRIM_SORT=1 switches to the rocPRIM bring-up path for
// comparison.
bool use_rocprim_sort() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("DE_USE_ROCPRIM_SORT");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}

// Which sort runs: production passes kDefault (the env switch decides); the
// debug bindings can force either implementation.
enum class SortChoice { kDefault, kCustom, kRocprim };

// Sorts ids (masking OOB to the `vocab` sentinel) by packing
// (id << 32 | position) into one u64 array; returns sorted_ids + the sorted
// original positions.  Hand-written sort by default, rocPRIM via env.
// variant is custom_radix_sort_keys' (-1: production dispatch).
void sort_ids_dispatch(torch::Tensor values, int64_t vocab, int64_t nnz,
                       int end_bit, torch::Tensor sorted_ids,
                       torch::Tensor sorted_pos, hipStream_t stream,
                       int variant = -1,
                       SortChoice sort = SortChoice::kDefault) {
  TORCH_CHECK(end_bit <= 32, "fused table vocab must fit 32 bits");
  TORCH_CHECK(nnz < (int64_t(1) << 32),
              "sort packs positions into 32 bits: nnz must be < 2^32");
  TORCH_CHECK(variant >= -1 && variant < custom_radix_sort_num_variants(),
              "sort variant must be -1 or in [0, ",
              custom_radix_sort_num_variants(), "), got ", variant);
  const bool rocprim = sort == SortChoice::kRocprim ||
                       (sort == SortChoice::kDefault && use_rocprim_sort());
  auto u64 = values.options().dtype(torch::kUInt64);
  auto i32 = values.options().dtype(torch::kInt32);
  auto packed = torch::empty({nnz}, u64);
  launch_mask_oob_pack(values.data_ptr<int64_t>(), nnz, vocab,
                       (uint64_t*)packed.data_ptr(), stream);
  auto packed_out = torch::empty({nnz}, u64);
  if (rocprim) {
    size_t temp_bytes = rocprim_sort_keys_temp_bytes(nnz);
    auto temp = torch::empty({(int64_t)temp_bytes},
                             values.options().dtype(torch::kUInt8));
    // rocPRIM's merge-sort path (mid-sized n) masks a bit range with
    // T(1) << end_bit, which is undefined at end_bit == 64 and then compares
    // the positions only.  A range ending at bit 64 (vocab >= 2^31) sorts the
    // whole key instead: the low words are the distinct ascending positions,
    // so the order is the stable order on the ids.
    const int begin_bit = end_bit == 32 ? 0 : 32;
    auto err = run_sort_keys_u64(temp.data_ptr(), temp_bytes,
                                 (const uint64_t*)packed.data_ptr(),
                                 (uint64_t*)packed_out.data_ptr(), nnz,
                                 begin_bit, 32 + end_bit, stream);
    TORCH_CHECK(err == hipSuccess, "radix_sort_keys failed");
  } else {
    auto keys_tmp = torch::empty({nnz}, u64);
    const int64_t hist_elems = (int64_t)custom_radix_sort_hist_elems(nnz);
    auto hist = torch::empty({hist_elems}, i32);
    auto scan_sums = torch::empty({4096}, i32);
    custom_radix_sort_keys((const uint64_t*)packed.data_ptr(),
                           (uint64_t*)packed_out.data_ptr(),
                           (uint64_t*)keys_tmp.data_ptr(),
                           hist.data_ptr<int32_t>(),
                           scan_sums.data_ptr<int32_t>(), nnz, 32,
                           32 + end_bit, variant, stream);
  }
  launch_unpack_sorted((const uint64_t*)packed_out.data_ptr(), nnz,
                       sorted_ids.data_ptr<int64_t>(),
                       sorted_pos.data_ptr<int32_t>(), stream);
}

// Optional per-id weights of a weighted lookup: fp32 [nnz] on the GPU, or
// nullptr when the caller gave none.
const float* per_id_w_ptr(const std::optional<torch::Tensor>& per_id_w,
                          const torch::Tensor& values) {
  if (!per_id_w.has_value()) return nullptr;
  const torch::Tensor& w = *per_id_w;
  CHECK_CUDA(w); CHECK_CONTIG(w);
  TORCH_CHECK(w.dtype() == torch::kFloat32, "per_id_w must be fp32");
  TORCH_CHECK(w.numel() == values.numel(),
              "per_id_w must have one weight per id: got ", w.numel(),
              " for ", values.numel(), " ids");
  return w.data_ptr<float>();
}

// Deterministic mode's buffers, allocated only when the mode is on and sized
// from host-known shapes (no sync): the slab holds one fp32 partial row per
// work item and has the work list's capacity, nnz / 64 + 64 rows -- a long
// row has len > 128 ids, so its ceil(len / 128) items number fewer than
// len / 64 -- and work_base one int32 per possible long row.
struct DetAlloc {
  torch::Tensor slab, work_base;
  DetAlloc(bool deterministic, int64_t nnz, int64_t max_long_rows, int width,
             const torch::TensorOptions& like) {
    if (!deterministic) return;
    slab = torch::empty({nnz / 64 + 64, (int64_t)width},
                        like.dtype(torch::kFloat32));
    work_base = torch::empty({max_long_rows}, like.dtype(torch::kInt32));
  }
  float* slab_ptr() const {
    return slab.defined() ? slab.data_ptr<float>() : nullptr;
  }
  int32_t* work_base_ptr() const {
    return work_base.defined() ? work_base.data_ptr<int32_t>() : nullptr;
  }
};

torch::Tensor csr_lookup_forward(torch::Tensor params, torch::Tensor values,
                                 torch::Tensor row_splits, bool mean,
                                 bool out_bf16,
                                 std::optional<torch::Tensor> per_id_w,
                                 bool deterministic) {
  CHECK_CUDA(params); CHECK_CUDA(values); CHECK_CUDA(row_splits);
  CHECK_CONTIG(params); CHECK_CONTIG(values); CHECK_CONTIG(row_splits);
  TORCH_CHECK(params.dtype() == torch::kFloat32 ||
                  params.dtype() == torch::kBFloat16,
              "params must be fp32 or bf16");
  TORCH_CHECK(values.dtype() == torch::kInt64, "values must be int64");
  TORCH_CHECK(row_splits.dtype() == torch::kInt64, "row_splits must be int64");
  const float* w_ptr = per_id_w_ptr(per_id_w, values);
  const int64_t num_rows = row_splits.numel() - 1;
  const int64_t vocab = params.size(0);
  const int width = (int)params.size(1);
  // accumulation is fp32 regardless of table/output storage dtype; bf16 out
  // stores RNE-rounded results directly (no separate cast kernel).  The
  // long-segment split needs fp32 atomics, so bf16-out launches reduce
  // every row in-register instead (fine for bounded forward hotness);
  // deterministic mode combines without atomics and splits them too.
  auto out = torch::empty({num_rows, width},
                          params.options().dtype(
                              out_bf16 ? torch::kBFloat16 : torch::kFloat32));
  if (num_rows > 0) {
    const int64_t nnz_in = values.numel();
    auto long_rows = torch::empty({num_rows}, values.options());
    auto long_count = torch::empty({1}, values.options().dtype(torch::kInt32));
    auto work_items = torch::empty({nnz_in / 64 + 64}, values.options());
    auto n_work = torch::empty({1}, values.options().dtype(torch::kInt32));
    const DetAlloc det(deterministic, nnz_in, num_rows, width,
                         params.options());
    launch_csr_lookup_forward(params.data_ptr(),
                              params.dtype() == torch::kBFloat16,
                              values.data_ptr<int64_t>(),
                              row_splits.data_ptr<int64_t>(), w_ptr,
                              out.data_ptr(), out_bf16, num_rows, nnz_in,
                              vocab, width, mean,
                              long_rows.data_ptr<int64_t>(),
                              long_count.data_ptr<int32_t>(),
                              work_items.data_ptr<int64_t>(),
                              n_work.data_ptr<int32_t>(), det.slab_ptr(),
                              det.work_base_ptr(), current_stream());
  }
  return out;
}

// int8 row-wise quantized table: uint8 [vocab, width + 8] (width bytes q,
// fp32 scale, fp32 bias per row), width a positive multiple of 4.
#define CHECK_Q8_PACKED(x)                                                   \
  CHECK_CUDA(x); CHECK_CONTIG(x);                                            \
  TORCH_CHECK((x).dtype() == torch::kUInt8, #x " must be uint8");            \
  TORCH_CHECK((x).dim() == 2 && (x).size(1) >= 12 &&                         \
                  ((x).size(1) - 8) % 4 == 0,                                \
              #x " must be [vocab, width + 8] with width a positive "        \
                 "multiple of 4");                                           \
  TORCH_CHECK(reinterpret_cast<uintptr_t>((x).data_ptr()) % 4 == 0,          \
              #x " must be 4-byte aligned")

// int4 row-wise quantized table: uint8 [vocab, width / 2 + 4] (width / 2
// bytes of nibbles, fp16 scale, fp16 bias per row), width a positive
// multiple of 8.
#define CHECK_Q4_PACKED(x)                                                   \
  CHECK_CUDA(x); CHECK_CONTIG(x);                                            \
  TORCH_CHECK((x).dtype() == torch::kUInt8, #x " must be uint8");            \
  TORCH_CHECK((x).dim() == 2 && (x).size(1) >= 8 &&                          \
                  ((x).size(1) - 4) % 4 == 0,                                \
              #x " must be [vocab, width / 2 + 4] with width a positive "    \
                 "multiple of 8");                                           \
  TORCH_CHECK(reinterpret_cast<uintptr_t>((x).data_ptr()) % 4 == 0,          \
              #x " must be 4-byte aligned")

using PackedForwardLauncher = decltype(&launch_csr_lookup_forward_q8);

// The forward from a checked packed table of logical width `width`.
torch::Tensor packed_lookup_forward(PackedForwardLauncher launch,
                                    const torch::Tensor& packed, int width,
                                    const torch::Tensor& values,
                                    const torch::Tensor& row_splits, bool mean,
                                    bool out_bf16,
                                    const std::optional<torch::Tensor>& per_id_w,
                                    bool deterministic) {
  CHECK_CUDA(values); CHECK_CUDA(row_splits);
  CHECK_CONTIG(values); CHECK_CONTIG(row_splits);
  TORCH_CHECK(values.dtype() == torch::kInt64, "values must be int64");
  TORCH_CHECK(row_splits.dtype() == torch::kInt64, "row_splits must be int64");
  TORCH_CHECK(values.device() == packed.device() &&
                  row_splits.device() == packed.device(),
              "packed, values and row_splits must be on one device");
  const float* w_ptr = per_id_w_ptr(per_id_w, values);
  const int64_t num_rows = row_splits.numel() - 1;
  const int64_t vocab = packed.size(0);
  const auto opts = packed.options().dtype(out_bf16 ? torch::kBFloat16
                                                    : torch::kFloat32);
  // an empty table has no row to read: every id is out of range
  if (vocab == 0) return torch::zeros({num_rows, width}, opts);
  // fp32 accumulation; bf16 out is stored directly and, as for the fp32 and
  // bf16 tables, reduces every row in-register (no long-row split) unless
  // the call is deterministic
  auto out = torch::empty({num_rows, width}, opts);
  if (num_rows > 0) {
    const int64_t nnz_in = values.numel();
    auto long_rows = torch::empty({num_rows}, values.options());
    auto long_count = torch::empty({1}, values.options().dtype(torch::kInt32));
    auto work_items = torch::empty({nnz_in / 64 + 64}, values.options());
    auto n_work = torch::empty({1}, values.options().dtype(torch::kInt32));
    const DetAlloc det(deterministic, nnz_in, num_rows, width,
                         packed.options());
    launch(packed.data_ptr(), values.data_ptr<int64_t>(),
           row_splits.data_ptr<int64_t>(), w_ptr, out.data_ptr(), out_bf16,
           num_rows, nnz_in, vocab, width, mean,
           long_rows.data_ptr<int64_t>(), long_count.data_ptr<int32_t>(),
           work_items.data_ptr<int64_t>(), n_work.data_ptr<int32_t>(),
           det.slab_ptr(), det.work_base_ptr(), current_stream());
  }
  return out;
}

torch::Tensor csr_lookup_forward_q8(torch::Tensor packed, torch::Tensor values,
                                    torch::Tensor row_splits, bool mean,
                                    bool out_bf16,
                                    std::optional<torch::Tensor> per_id_w,
                                    bool deterministic) {
  CHECK_Q8_PACKED(packed);
  return packed_lookup_forward(&launch_csr_lookup_forward_q8, packed,
                               (int)packed.size(1) - 8, values, row_splits,
                               mean, out_bf16, per_id_w, deterministic);
}

torch::Tensor csr_lookup_forward_q4(torch::Tensor packed, torch::Tensor values,
                                    torch::Tensor row_splits, bool mean,
                                    bool out_bf16,
                                    std::optional<torch::Tensor> per_id_w,
                                    bool deterministic) {
  CHECK_Q4_PACKED(packed);
  return packed_lookup_forward(&launch_csr_lookup_forward_q4, packed,
                               2 * ((int)packed.size(1) - 4), values,
                               row_splits, mean, out_bf16, per_id_w,
                               deterministic);
}

torch::Tensor quantize_rows_q8(torch::Tensor weight) {
  CHECK_CUDA(weight); CHECK_CONTIG(weight);
  TORCH_CHECK(weight.dtype() == torch::kFloat32 ||
                  weight.dtype() == torch::kBFloat16,
              "weight must be fp32 or bf16");
  TORCH_CHECK(weight.dim() == 2 && weight.size(1) >= 4 &&
                  weight.size(1) % 4 == 0,
              "weight must be [n, width] with width a positive multiple of "
              "4, got width ", weight.dim() == 2 ? weight.size(1) : -1);
  // a lane loads four columns at once: 16 bytes of fp32, 8 of bf16
  TORCH_CHECK(reinterpret_cast<uintptr_t>(weight.data_ptr()) %
                      (4 * weight.element_size()) == 0,
              "weight must be aligned to four of its elements");
  const int64_t n = weight.size(0);
  const int width = (int)weight.size(1);
  auto packed = torch::empty({n, width + 8},
                             weight.options().dtype(torch::kUInt8));
  launch_quantize_rows_q8(weight.data_ptr(),
                          weight.dtype() == torch::kBFloat16,
                          packed.data_ptr(), n, width, current_stream());
  return packed;
}

torch::Tensor dequantize_rows_q8(torch::Tensor packed) {
  CHECK_Q8_PACKED(packed);
  const int64_t n = packed.size(0);
  const int width = (int)packed.size(1) - 8;
  auto out = torch::empty({n, width},
                          packed.options().dtype(torch::kFloat32));
  launch_dequantize_rows_q8(packed.data_ptr(), out.data_ptr<float>(), n, width,
                            current_stream());
  return out;
}

torch::Tensor quantize_rows_q4(torch::Tensor weight) {
  CHECK_CUDA(weight); CHECK_CONTIG(weight);
  TORCH_CHECK(weight.dtype() == torch::kFloat32 ||
                  weight.dtype() == torch::kBFloat16,
              "weight must be fp32 or bf16");
  TORCH_CHECK(weight.dim() == 2 && weight.size(1) >= 8 &&
                  weight.size(1) % 8 == 0,
              "weight must be [n, width] with width a positive multiple of "
              "8 (the 4-bit layout itself only needs an even width), got "
              "width ", weight.dim() == 2 ? weight.size(1) : -1);
  // a lane loads its eight columns four at a time: 16 bytes of fp32, 8 of bf16
  TORCH_CHECK(reinterpret_cast<uintptr_t>(weight.data_ptr()) %
                      (4 * weight.element_size()) == 0,
              "weight must be aligned to four of its elements");
  const int64_t n = weight.size(0);
  const int width = (int)weight.size(1);
  auto packed = torch::empty({n, width / 2 + 4},
                             weight.options().dtype(torch::kUInt8));
  launch_quantize_rows_q4(weight.data_ptr(),
                          weight.dtype() == torch::kBFloat16,
                          packed.data_ptr(), n, width, current_stream());
  return packed;
}

torch::Tensor dequantize_rows_q4(torch::Tensor packed) {
  CHECK_Q4_PACKED(packed);
  const int64_t n = packed.size(0);
  const int width = 2 * ((int)packed.size(1) - 4);
  auto out = torch::empty({n, width},
                          packed.options().dtype(torch::kFloat32));
  launch_dequantize_rows_q4(packed.data_ptr(), out.data_ptr<float>(), n, width,
                            current_stream());
  return out;
}

torch::Tensor row_to_split(torch::Tensor rows, int64_t num_rows) {
  CHECK_CUDA(rows); CHECK_CONTIG(rows);
  TORCH_CHECK(rows.dtype() == torch::kInt64);
  auto splits = torch::empty({num_rows + 1}, rows.options());
  launch_row_to_split(rows.data_ptr<int64_t>(), rows.numel(), num_rows,
                      splits.data_ptr<int64_t>(), current_stream());
  return splits;
}

// Sorted-segment view of a CSR batch, shared by the sparse backward and the
// fused update: the ids sorted ascending (OOB masked to the `vocab` sentinel,
// so last), the source row and mean weight of each sorted position, and one
// segment per unique valid id.  With user_w (per-id weights of a weighted
// lookup, or nullptr) sw holds c_r * user_w instead.  seg holds num_unique segment starts; each
// caller finishes seg[num_unique...] from bounds in its own way.
struct SortedSegments {
  torch::Tensor sorted_ids;  // [nnz] i64
  torch::Tensor srow;        // [nnz] i64: row of each sorted id
  torch::Tensor sw;          // [nnz] f32: 1/len of that row (mean) times
                             // the id's weight (weighted); else undefined
  torch::Tensor seg;         // [nnz + 1] i64: first num_unique are set
  torch::Tensor unique_ids;  // [nnz] i64: first num_unique are set
  torch::Tensor num_unique;  // [1] i32, on the device
  torch::Tensor bounds;      // [1] i64, on the device: first OOB position
  float* sw_ptr() const { return sw.defined() ? sw.data_ptr<float>() : nullptr; }
};

SortedSegments build_sorted_segments(torch::Tensor values,
                                     torch::Tensor row_splits, int64_t vocab,
                                     bool mean, const float* user_w,
                                     hipStream_t stream, int variant = -1,
                                     SortChoice sort = SortChoice::kDefault) {
  const int64_t nnz = values.numel();
  const int64_t num_rows = row_splits.numel() - 1;
  auto i64 = values.options();
  auto i32 = values.options().dtype(torch::kInt32);
  auto f32 = values.options().dtype(torch::kFloat32);
  SortedSegments ss;

  // 1. per-id row ids (+ mean and user weights keyed by original position).
  const bool has_w = mean || user_w != nullptr;
  auto row_ids = torch::empty({nnz}, i32);
  torch::Tensor w;
  if (has_w) w = torch::empty({nnz}, f32);
  float* w_ptr = has_w ? w.data_ptr<float>() : nullptr;
  launch_expand_row_ids(row_splits.data_ptr<int64_t>(), num_rows, nnz,
                        row_ids.data_ptr<int32_t>(), w_ptr, mean, user_w,
                        stream);

  // 2. mask OOB -> sentinel and radix sort packed (id, position); end_bit
  // covers [0, vocab] inclusive.
  ss.sorted_ids = torch::empty({nnz}, i64);
  auto sorted_pos = torch::empty({nnz}, i32);
  sort_ids_dispatch(values, vocab, nnz, log2_ceil(vocab + 1), ss.sorted_ids,
                    sorted_pos, stream, variant, sort);
  size_t temp_bytes = csr_backward_temp_bytes(nnz);
  auto temp = torch::empty({(int64_t)temp_bytes}, i64.dtype(torch::kUInt8));

  // 3. permute row ids (+ weights) into sorted order, widened to i64.
  ss.srow = torch::empty({nnz}, i64);
  if (has_w) ss.sw = torch::empty({nnz}, f32);
  launch_gather_sorted(sorted_pos.data_ptr<int32_t>(),
                       row_ids.data_ptr<int32_t>(), w_ptr, nnz,
                       ss.srow.data_ptr<int64_t>(), ss.sw_ptr(), stream);

  // 4. unique-by-key via head flags + scan.
  auto head = torch::empty({nnz}, i32);
  auto pos = torch::empty({nnz}, i32);
  launch_mark_heads(ss.sorted_ids.data_ptr<int64_t>(), nnz, vocab,
                    head.data_ptr<int32_t>(), stream);
  auto err = run_inclusive_scan_i32(temp.data_ptr(), temp_bytes,
                                    head.data_ptr<int32_t>(),
                                    pos.data_ptr<int32_t>(), nnz, stream);
  TORCH_CHECK(err == hipSuccess, "inclusive_scan failed");
  ss.unique_ids = torch::empty({nnz}, i64);
  ss.seg = torch::empty({nnz + 1}, i64);
  ss.num_unique = torch::zeros({1}, i32);
  launch_scatter_unique(ss.sorted_ids.data_ptr<int64_t>(),
                        head.data_ptr<int32_t>(), pos.data_ptr<int32_t>(), nnz,
                        ss.unique_ids.data_ptr<int64_t>(),
                        ss.seg.data_ptr<int64_t>(),
                        ss.num_unique.data_ptr<int32_t>(), stream);
  ss.bounds = torch::empty({1}, i64);
  launch_find_valid_bounds(ss.sorted_ids.data_ptr<int64_t>(), nnz, vocab,
                           ss.bounds.data_ptr<int64_t>(), stream);
  return ss;
}

std::vector<torch::Tensor> csr_lookup_backward(torch::Tensor grad_out,
                                               torch::Tensor values,
                                               torch::Tensor row_splits,
                                               int64_t vocab, bool mean,
                                               std::optional<torch::Tensor>
                                                   per_id_w,
                                               bool deterministic) {
  CHECK_CUDA(grad_out); CHECK_CUDA(values); CHECK_CUDA(row_splits);
  CHECK_CONTIG(grad_out); CHECK_CONTIG(values); CHECK_CONTIG(row_splits);
  TORCH_CHECK(grad_out.dtype() == torch::kFloat32 ||
                  grad_out.dtype() == torch::kBFloat16,
              "grad_out must be fp32 or bf16");
  const float* user_w = per_id_w_ptr(per_id_w, values);
  const int64_t nnz = values.numel();
  const int width = (int)grad_out.size(1);
  auto stream = current_stream();
  auto i64 = values.options();
  auto i32 = values.options().dtype(torch::kInt32);
  auto f32 = grad_out.options().dtype(torch::kFloat32);

  if (nnz == 0) {
    return {torch::empty({0}, i64), torch::empty({0, width}, f32)};
  }

  auto ss = build_sorted_segments(values, row_splits, vocab, mean, user_w,
                                  stream);
  launch_set_seg_end(ss.seg.data_ptr<int64_t>(),
                     ss.num_unique.data_ptr<int32_t>(),
                     ss.bounds.data_ptr<int64_t>(), stream);

  // the one host sync: number of unique ids (output allocation).
  const int64_t nu = ss.num_unique.to(torch::kCPU).item<int32_t>();

  auto unique_ids = ss.unique_ids.narrow(0, 0, nu).contiguous();
  auto unique_grad = torch::empty({nu, width}, f32);
  if (nu > 0) {
    // segmented sum == forward gather-reduce over grad_out rows.
    auto long_rows = torch::empty({nu}, i64);
    auto long_count = torch::empty({1}, i32);
    auto work_items = torch::empty({nnz / 64 + 64}, i64);
    auto n_work = torch::empty({1}, i32);
    const DetAlloc det(deterministic, nnz, nu, width, f32);
    launch_csr_lookup_forward(grad_out.data_ptr(),
                              grad_out.dtype() == torch::kBFloat16,
                              ss.srow.data_ptr<int64_t>(),
                              ss.seg.data_ptr<int64_t>(), ss.sw_ptr(),
                              unique_grad.data_ptr<float>(), false, nu, nnz,
                              grad_out.size(0), width, /*mean=*/false,
                              long_rows.data_ptr<int64_t>(),
                              long_count.data_ptr<int32_t>(),
                              work_items.data_ptr<int64_t>(),
                              n_work.data_ptr<int32_t>(), det.slab_ptr(),
                              det.work_base_ptr(), stream);
  }
  return {unique_ids, unique_grad};
}

// --- test-only windows into the sort pipeline (not public API) -------------

SortChoice parse_sort_choice(const std::string& sort) {
  if (sort == "default") return SortChoice::kDefault;
  if (sort == "custom") return SortChoice::kCustom;
  if (sort == "rocprim") return SortChoice::kRocprim;
  TORCH_CHECK(false, "sort must be 'default', 'custom' or 'rocprim', got '",
              sort, "'");
}

void check_debug_ids(const torch::Tensor& values, int64_t vocab,
                     int64_t variant) {
  CHECK_CUDA(values); CHECK_CONTIG(values);
  TORCH_CHECK(values.dtype() == torch::kInt64, "values must be int64");
  TORCH_CHECK(vocab >= 1 && vocab < (int64_t(1) << 32),
              "vocab must be in [1, 2^32), got ", vocab);
  TORCH_CHECK(variant >= -1 && variant < custom_radix_sort_num_variants(),
              "sort variant must be -1 or in [0, ",
              custom_radix_sort_num_variants(), "), got ", variant);
}

std::vector<int64_t> debug_sort_variant_tiles() {
  std::vector<int64_t> tiles;
  for (int v = 0; v < custom_radix_sort_num_variants(); ++v)
    tiles.push_back(custom_radix_sort_variant_tile(v));
  return tiles;
}

// Exactly what sort_ids_dispatch produces: (sorted_ids i64, sorted_pos i32).
std::tuple<torch::Tensor, torch::Tensor> debug_sort_ids(
    torch::Tensor values, int64_t vocab, int64_t variant,
    const std::string& sort) {
  check_debug_ids(values, vocab, variant);
  const SortChoice choice = parse_sort_choice(sort);
  const int64_t nnz = values.numel();
  auto sorted_ids = torch::empty({nnz}, values.options());
  auto sorted_pos =
      torch::empty({nnz}, values.options().dtype(torch::kInt32));
  if (nnz == 0) return {sorted_ids, sorted_pos};
  sort_ids_dispatch(values, vocab, nnz, log2_ceil(vocab + 1), sorted_ids,
                    sorted_pos, current_stream(), (int)variant, choice);
  return {sorted_ids, sorted_pos};
}

// build_sorted_segments plus the caller's finish of seg: set_seg_end (the
// sparse backward) or, with padded, pad_seg_offsets (the fused update).
// Returns (sorted_ids, srow, sw or None, seg, unique_ids, num_unique, bounds).
std::tuple<torch::Tensor, torch::Tensor, std::optional<torch::Tensor>,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
debug_sorted_segments(torch::Tensor values, torch::Tensor row_splits,
                      int64_t vocab, bool mean,
                      std::optional<torch::Tensor> per_id_w, bool padded,
                      int64_t variant, const std::string& sort) {
  check_debug_ids(values, vocab, variant);
  CHECK_CUDA(row_splits); CHECK_CONTIG(row_splits);
  TORCH_CHECK(row_splits.dtype() == torch::kInt64, "row_splits must be int64");
  const SortChoice choice = parse_sort_choice(sort);
  const float* user_w = per_id_w_ptr(per_id_w, values);
  const int64_t nnz = values.numel();
  // a debug entry point can afford the sync: rows must cover [0, nnz)
  TORCH_CHECK(row_splits.numel() >= 1, "row_splits must not be empty");
  TORCH_CHECK(row_splits[0].item<int64_t>() == 0 &&
                  row_splits[-1].item<int64_t>() == nnz,
              "row_splits must run from 0 to nnz");
  auto i64 = values.options();
  auto i32 = values.options().dtype(torch::kInt32);
  if (nnz == 0) {
    std::optional<torch::Tensor> sw;
    if (mean || user_w)
      sw = torch::empty({0}, values.options().dtype(torch::kFloat32));
    return {torch::empty({0}, i64), torch::empty({0}, i64), sw,
            torch::zeros({1}, i64), torch::empty({0}, i64),
            torch::zeros({1}, i32), torch::zeros({1}, i64)};
  }
  auto stream = current_stream();
  auto ss = build_sorted_segments(values, row_splits, vocab, mean, user_w,
                                  stream, (int)variant, choice);
  if (padded) {
    launch_pad_seg_offsets(ss.seg.data_ptr<int64_t>(), nnz,
                           ss.num_unique.data_ptr<int32_t>(),
                           ss.bounds.data_ptr<int64_t>(), stream);
  } else {
    launch_set_seg_end(ss.seg.data_ptr<int64_t>(),
                       ss.num_unique.data_ptr<int32_t>(),
                       ss.bounds.data_ptr<int64_t>(), stream);
  }
  std::optional<torch::Tensor> sw;
  if (ss.sw.defined()) sw = ss.sw;
  return {ss.sorted_ids, ss.srow, sw, ss.seg, ss.unique_ids, ss.num_unique,
          ss.bounds};
}

// Gradient of the per-id weights of a weighted lookup, fp32 [nnz]:
// dw[k] = c_r * <grad_out[r(k)], params[values[k]]>, 0 for an out-of-range
// id.  No host sync and torch-allocated buffers only, so it can be captured.
torch::Tensor csr_lookup_weight_grad(torch::Tensor grad_out,
                                     torch::Tensor params,
                                     torch::Tensor values,
                                     torch::Tensor row_splits, bool mean) {
  CHECK_CUDA(grad_out); CHECK_CUDA(params); CHECK_CUDA(values);
  CHECK_CUDA(row_splits);
  CHECK_CONTIG(grad_out); CHECK_CONTIG(params); CHECK_CONTIG(values);
  CHECK_CONTIG(row_splits);
  TORCH_CHECK(grad_out.dtype() == torch::kFloat32 ||
                  grad_out.dtype() == torch::kBFloat16,
              "grad_out must be fp32 or bf16");
  TORCH_CHECK(params.dtype() == torch::kFloat32 ||
                  params.dtype() == torch::kBFloat16,
              "params must be fp32 or bf16");
  TORCH_CHECK(values.dtype() == torch::kInt64, "values must be int64");
  TORCH_CHECK(row_splits.dtype() == torch::kInt64, "row_splits must be int64");
  const int64_t nnz = values.numel();
  const int64_t num_rows = row_splits.numel() - 1;
  TORCH_CHECK(grad_out.dim() == 2 && params.dim() == 2 &&
                  grad_out.size(0) == num_rows &&
                  grad_out.size(1) == params.size(1),
              "grad_out must be [num_rows, width]");
  auto stream = current_stream();
  auto dw = torch::zeros({nnz}, grad_out.options().dtype(torch::kFloat32));
  if (nnz == 0 || num_rows <= 0) return dw;
  // zero-filled: a position no row covers reads row 0 and stays in bounds
  auto row_ids = torch::zeros({nnz}, values.options().dtype(torch::kInt32));
  launch_expand_row_ids(row_splits.data_ptr<int64_t>(), num_rows, nnz,
                        row_ids.data_ptr<int32_t>(), nullptr, false, nullptr,
                        stream);
  launch_csr_weight_grad(params.data_ptr(),
                         params.dtype() == torch::kBFloat16,
                         grad_out.data_ptr(),
                         grad_out.dtype() == torch::kBFloat16,
                         values.data_ptr<int64_t>(),
                         row_ids.data_ptr<int32_t>(),
                         row_splits.data_ptr<int64_t>(), mean,
                         dw.data_ptr<float>(), nnz, params.size(0),
                         (int)params.size(1), stream);
  return dw;
}

torch::Tensor integer_lookup(torch::Tensor keys, torch::Tensor table_keys,
                             torch::Tensor table_values, torch::Tensor counts,
                             int64_t max_tokens) {
  CHECK_CUDA(keys); CHECK_CUDA(table_keys); CHECK_CUDA(table_values);
  CHECK_CUDA(counts);
  CHECK_CONTIG(keys); CHECK_CONTIG(table_keys); CHECK_CONTIG(table_values);
  CHECK_CONTIG(counts);
  const int64_t n = keys.numel();
  const int64_t capacity = table_keys.numel();
  auto i32 = keys.options().dtype(torch::kInt32);
  auto i64 = keys.options();
  auto out = torch::empty({n}, i64);
  if (n == 0) return out;
  const int64_t nvals = max_tokens + 1;
  size_t temp_bytes = integer_lookup_temp_bytes(max_tokens);
  auto temp = torch::empty({(int64_t)temp_bytes}, i32.dtype(torch::kUInt8));
  auto flags = torch::empty({nvals}, i32);
  auto pos = torch::empty({nvals}, i32);
  auto avail = torch::empty({nvals}, i64);
  auto navail = torch::zeros({1}, i32);
  auto next_avail = torch::zeros({1}, i32);
  launch_integer_lookup(keys.data_ptr<int64_t>(), n,
                        table_keys.data_ptr<int64_t>(),
                        table_values.data_ptr<int64_t>(), capacity,
                        counts.data_ptr<int32_t>(), max_tokens,
                        temp.data_ptr(), temp_bytes, flags.data_ptr<int32_t>(),
                        pos.data_ptr<int32_t>(), avail.data_ptr<int64_t>(),
                        navail.data_ptr<int32_t>(),
                        next_avail.data_ptr<int32_t>(),
                        out.data_ptr<int64_t>(), current_stream());
  return out;
}

void hash_rehash(torch::Tensor old_keys, torch::Tensor old_values,
                 torch::Tensor new_keys, torch::Tensor new_values) {
  CHECK_CUDA(old_keys); CHECK_CUDA(old_values);
  CHECK_CUDA(new_keys); CHECK_CUDA(new_values);
  CHECK_CONTIG(old_keys); CHECK_CONTIG(old_values);
  CHECK_CONTIG(new_keys); CHECK_CONTIG(new_values);
  TORCH_CHECK(new_keys.numel() >= old_keys.numel(),
              "rehash target must not be smaller");
  launch_hash_reinsert(old_keys.data_ptr<int64_t>(),
                       old_values.data_ptr<int64_t>(), old_keys.numel(),
                       new_keys.data_ptr<int64_t>(),
                       new_values.data_ptr<int64_t>(), new_keys.numel(),
                       current_stream());
}

// Adagrad state is fp32 [vocab, width]; a 1-D fp32 [vocab] state selects
// row-wise Adagrad (one accumulator per row).  Returns true for row-wise.
static bool check_adagrad_state(const torch::Tensor& state,
                                const torch::Tensor& weight) {
  CHECK_CUDA(state); CHECK_CONTIG(state);
  const bool rowwise = state.dim() == 1 && state.size(0) == weight.size(0);
  TORCH_CHECK(rowwise || state.sizes() == weight.sizes(),
              "adagrad state shape mismatch: expected [vocab, width] "
              "(element-wise) or [vocab] (row-wise), got ", state.sizes(),
              " for weight ", weight.sizes());
  TORCH_CHECK(state.dtype() == torch::kFloat32, "adagrad state must be fp32");
  return rowwise;
}

// The {seed, step} pair of stochastic rounding: int64 [2] on the weight's
// device, bf16 weights only.  Returns its pointer, nullptr without one.
static int64_t* sr_ptr(const std::optional<torch::Tensor>& sr,
                       const torch::Tensor& weight) {
  if (!sr.has_value()) return nullptr;
  const torch::Tensor& t = *sr;
  CHECK_CUDA(t); CHECK_CONTIG(t);
  TORCH_CHECK(t.dtype() == torch::kInt64 && t.dim() == 1 && t.numel() == 2,
              "sr must be an int64 [2] tensor {seed, step}");
  TORCH_CHECK(t.device() == weight.device(),
              "sr must be on the weight's device");
  TORCH_CHECK(weight.dtype() == torch::kBFloat16,
              "stochastic rounding needs a bf16 weight: an fp32 weight has "
              "nothing to round");
  return t.data_ptr<int64_t>();
}

// Adam's moments, fp32 on the weight's device; both betas in [0, 1).  The
// shape selects the rule: [2, vocab, width], m first, is lazy Adam, and a 1-D
// state of vocab * (width + 1) elements, m [vocab, width] then the rows' v
// [vocab], is partial row-wise Adam.  Returns true for the latter.
static bool check_adam_state(const torch::Tensor& state,
                             const torch::Tensor& weight, double beta1,
                             double beta2) {
  CHECK_CUDA(state); CHECK_CONTIG(state);
  TORCH_CHECK(state.dtype() == torch::kFloat32, "adam state must be fp32");
  const bool lazy = state.dim() == 3 && state.size(0) == 2 &&
                    state.size(1) == weight.size(0) &&
                    state.size(2) == weight.size(1);
  const bool rowwise =
      state.dim() == 1 &&
      state.size(0) == weight.size(0) * (weight.size(1) + 1);
  TORCH_CHECK(lazy || rowwise,
              "adam state shape mismatch: expected [2, vocab, width] (lazy "
              "Adam) or [vocab * (width + 1)] (partial row-wise Adam), got ",
              state.sizes(), " for weight ", weight.sizes());
  TORCH_CHECK(state.device() == weight.device(),
              "adam state must be on the weight's device");
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
              "adam betas must lie in [0, 1), got (", beta1, ", ", beta2, ")");
  return rowwise;
}

// adam_step > 0 selects Adam at step t = adam_step (the host counts on this
// path): adagrad has to be false, and state is [2, vocab, width] for lazy
// Adam or [vocab * (width + 1)] for partial row-wise Adam.
void sparse_row_update(torch::Tensor weight, torch::Tensor state,
                       torch::Tensor ids, torch::Tensor grad, double lr,
                       double eps, bool adagrad,
                       std::optional<torch::Tensor> sr, int64_t adam_step,
                       double beta1, double beta2) {
  CHECK_CUDA(weight); CHECK_CUDA(ids); CHECK_CUDA(grad);
  CHECK_CONTIG(weight); CHECK_CONTIG(ids); CHECK_CONTIG(grad);
  TORCH_CHECK(weight.dtype() == torch::kFloat32 ||
              weight.dtype() == torch::kBFloat16);
  TORCH_CHECK(grad.dtype() == torch::kFloat32);
  TORCH_CHECK(ids.dtype() == torch::kInt64);
  int64_t* sr_p = sr_ptr(sr, weight);
  TORCH_CHECK(adam_step >= 0, "adam_step must not be negative");
  const bool adam = adam_step > 0;
  TORCH_CHECK(!(adam && adagrad), "adam_step and adagrad exclude each other");
  bool rowwise = adam && check_adam_state(state, weight, beta1, beta2);
  const int64_t n = ids.numel();
  if (n == 0) return;
  float* state_ptr = nullptr;
  if (adagrad) {
    rowwise = check_adagrad_state(state, weight);
    state_ptr = state.data_ptr<float>();
  }
  AdamConfig cfg{beta1, beta2, weight.size(0), nullptr, nullptr};
  if (adam) {
    state_ptr = state.data_ptr<float>();
    const double t = (double)adam_step;
    lr = lr * std::sqrt(1.0 - std::pow(beta2, t)) / (1.0 - std::pow(beta1, t));
  }
  launch_sparse_row_update(weight.data_ptr(),
                           weight.dtype() == torch::kBFloat16, state_ptr,
                           ids.data_ptr<int64_t>(), grad.data_ptr<float>(), n,
                           (int)weight.size(1), (float)lr, (float)eps, adagrad,
                           rowwise, sr_p, adam ? &cfg : nullptr,
                           current_stream());
}

// The id-only half of the fused update: build_sorted_segments with seg padded
// (launch_pad_seg_offsets), plus the sizes the apply checks its arguments
// against.  It depends on the ids, the row lengths and the per-id weights
// alone, so it can be built as soon as the forward lookup is launched.  An
// empty plan (no ids or no rows) holds no tensors and applies as a no-op.
struct SortPlan {
  SortedSegments ss;
  int64_t nnz = 0;
  int64_t num_rows = 0;
  int64_t vocab = 0;
  bool empty() const { return num_rows <= 0 || nnz <= 0; }
};

// All on the device, no host sync; the same kernels and sort dispatch
// (DE_USE_ROCPRIM_SORT included) as the one-shot csr_fused_optimizer_apply.
SortPlan csr_sort_plan(torch::Tensor values, torch::Tensor row_splits,
                       int64_t vocab, bool mean,
                       std::optional<torch::Tensor> per_id_w) {
  CHECK_CUDA(values); CHECK_CUDA(row_splits);
  CHECK_CONTIG(values); CHECK_CONTIG(row_splits);
  TORCH_CHECK(vocab >= 0, "vocab must not be negative, got ", vocab);
  const float* user_w = per_id_w_ptr(per_id_w, values);
  SortPlan plan;
  plan.nnz = values.numel();
  plan.num_rows = row_splits.numel() - 1;
  plan.vocab = vocab;
  if (plan.empty()) return plan;
  auto stream = current_stream();
  plan.ss = build_sorted_segments(values, row_splits, vocab, mean, user_w,
                                  stream);
  launch_pad_seg_offsets(plan.ss.seg.data_ptr<int64_t>(), plan.nnz,
                         plan.ss.num_unique.data_ptr<int32_t>(),
                         plan.ss.bounds.data_ptr<int64_t>(), stream);
  return plan;
}

// What the apply has checked about its arguments.
struct FusedApplyArgs {
  int64_t* sr_p;  // {seed, step} of stochastic rounding, or nullptr
  bool rowwise;   // row-wise Adagrad or partial row-wise Adam state
};

// The one copy of the apply's argument checks; launches nothing.  nnz and
// num_rows are the plan's (or, for the one-shot call, those of the ids the
// plan will be built from): without ids or rows the apply is a no-op, and the
// Adagrad state and the shape of grad_out are not looked at.
static FusedApplyArgs check_fused_apply(
    const torch::Tensor& weight, const torch::Tensor& state,
    const torch::Tensor& grad_out, const torch::Tensor& lr, bool adagrad,
    const std::optional<torch::Tensor>& sr,
    const std::optional<torch::Tensor>& adam_step, double beta1, double beta2,
    int64_t nnz, int64_t num_rows) {
  CHECK_CUDA(weight); CHECK_CUDA(grad_out); CHECK_CUDA(lr);
  CHECK_CONTIG(weight); CHECK_CONTIG(grad_out);
  TORCH_CHECK(weight.dim() == 2, "weight must be [vocab, width]");
  TORCH_CHECK(weight.dtype() == torch::kFloat32 ||
              weight.dtype() == torch::kBFloat16);
  TORCH_CHECK((grad_out.dtype() == torch::kFloat32 ||
               grad_out.dtype() == torch::kBFloat16) &&
              lr.dtype() == torch::kFloat32);
  FusedApplyArgs args{sr_ptr(sr, weight), false};
  if (adam_step.has_value()) {
    TORCH_CHECK(!adagrad, "adam_step and adagrad exclude each other");
    args.rowwise = check_adam_state(state, weight, beta1, beta2);
    const torch::Tensor& t = *adam_step;
    CHECK_CUDA(t); CHECK_CONTIG(t);
    TORCH_CHECK(t.dtype() == torch::kInt64 && t.dim() == 1 && t.numel() == 1,
                "adam_step must be an int64 [1] tensor");
    TORCH_CHECK(t.device() == weight.device(),
                "adam_step must be on the weight's device");
  }
  if (num_rows <= 0 || nnz <= 0) return args;
  // srow indexes rows of grad_out
  TORCH_CHECK(grad_out.numel() == num_rows * weight.size(1),
              "grad_out must be [num_rows, width] = [", num_rows, ", ",
              weight.size(1), "], got ", grad_out.sizes());
  if (adagrad) args.rowwise = check_adagrad_state(state, weight);
  return args;
}

// The gradient half on checked arguments: one direct update per unique row of
// the plan (long segments chunked with one atomic per partial, or,
// deterministic, one slab row per partial and a fixed-order combine).
static void apply_sort_plan(torch::Tensor weight, torch::Tensor state,
                            const SortPlan& plan, torch::Tensor grad_out,
                            torch::Tensor lr, bool adagrad, double eps,
                            const FusedApplyArgs& args,
                            std::optional<torch::Tensor> adam_step,
                            double beta1, double beta2, bool deterministic) {
  if (plan.empty()) return;
  const SortedSegments& ss = plan.ss;
  const bool wbf16 = weight.dtype() == torch::kBFloat16;
  const int64_t nnz = plan.nnz;
  const int64_t vocab = weight.size(0);
  const int width = (int)weight.size(1);
  const bool adam = adam_step.has_value();
  auto stream = current_stream();
  auto i64 = ss.sorted_ids.options();
  auto i32 = i64.dtype(torch::kInt32);
  auto f32 = grad_out.options().dtype(torch::kFloat32);

  auto long_rows = torch::empty({nnz}, i64);
  auto long_count = torch::empty({1}, i32);
  auto work_items = torch::empty({nnz / 64 + 64}, i64);
  auto n_work = torch::empty({1}, i32);
  float* state_ptr = nullptr;
  torch::Tensor scratch;
  float* scratch_ptr = nullptr;
  int64_t scratch_rows = 0;
  if (adagrad) state_ptr = state.data_ptr<float>();
  AdamConfig cfg{beta1, beta2, vocab, nullptr, nullptr};
  torch::Tensor a_t;
  if (adam) {
    state_ptr = state.data_ptr<float>();
    a_t = torch::empty({1}, f32);
    cfg.step = adam_step->data_ptr<int64_t>();
    cfg.a_t = a_t.data_ptr<float>();
  }
  if (adagrad || adam || wbf16 || deterministic) {
    scratch_rows = nnz / (128 + 1) + 1;  // max possible long segments
    scratch = torch::empty({scratch_rows, (int64_t)width}, f32);
    scratch_ptr = scratch.data_ptr<float>();
  }
  // a long segment has more than 128 ids: at most scratch_rows of them
  const DetAlloc det(deterministic, nnz, nnz / (128 + 1) + 1, width, f32);
  launch_sorted_optimizer_update(weight.data_ptr(), wbf16, state_ptr,
                                 (float)eps, ss.sorted_ids.data_ptr<int64_t>(),
                                 ss.seg.data_ptr<int64_t>(),
                                 ss.srow.data_ptr<int64_t>(), ss.sw_ptr(),
                                 grad_out.data_ptr(),
                                 grad_out.dtype() == torch::kBFloat16,
                                 lr.data_ptr<float>(),
                                 ss.num_unique.data_ptr<int32_t>(), nnz, width,
                                 long_rows.data_ptr<int64_t>(),
                                 long_count.data_ptr<int32_t>(),
                                 work_items.data_ptr<int64_t>(),
                                 n_work.data_ptr<int32_t>(), scratch_ptr,
                                 scratch_rows, adagrad, args.rowwise,
                                 args.sr_p, adam ? &cfg : nullptr,
                                 det.slab_ptr(), det.work_base_ptr(), stream);
}

// The gradient half of the fused update on a csr_sort_plan.  Reads the plan's
// tensors only and leaves them as they are, so one plan can be applied more
// than once.  adam_step (int64 [1] on the device) selects Adam: state is
// [2, vocab, width] (lazy Adam) or [vocab * (width + 1)] (partial row-wise
// Adam), adagrad has to be false, and an apply that launches adds 1 to the
// step on the device.
void csr_fused_optimizer_apply_planned(torch::Tensor weight,
                                       torch::Tensor state,
                                       const SortPlan& plan,
                                       torch::Tensor grad_out,
                                       torch::Tensor lr, bool adagrad,
                                       double eps,
                                       std::optional<torch::Tensor> sr,
                                       std::optional<torch::Tensor> adam_step,
                                       double beta1, double beta2,
                                       bool deterministic) {
  const FusedApplyArgs args =
      check_fused_apply(weight, state, grad_out, lr, adagrad, sr, adam_step,
                        beta1, beta2, plan.nnz, plan.num_rows);
  TORCH_CHECK(plan.vocab == weight.size(0),
              "the sort plan was built for vocab ", plan.vocab,
              ", the weight has ", weight.size(0), " rows");
  TORCH_CHECK(plan.empty() || plan.ss.sorted_ids.device() == weight.device(),
              "the sort plan must be on the weight's device");
  apply_sort_plan(weight, state, plan, grad_out, lr, adagrad, eps, args,
                  adam_step, beta1, beta2, deterministic);
}

// Plan and planned apply in one call: the all-device sorted pipeline (no host
// sync; hipGraph-capturable) sort (id, pos) -> permute row-ids -> head-flag
// unique -> segment pad -> update.  Replaces both torch sparse grads and the
// naive atomic scatter (hot-row same-address chains).  Every argument is
// checked before the first launch.
void csr_fused_optimizer_apply(torch::Tensor weight, torch::Tensor state,
                               torch::Tensor values, torch::Tensor row_splits,
                               torch::Tensor grad_out, torch::Tensor lr,
                               bool mean, bool adagrad, double eps,
                               std::optional<torch::Tensor> per_id_w,
                               std::optional<torch::Tensor> sr,
                               std::optional<torch::Tensor> adam_step,
                               double beta1, double beta2,
                               bool deterministic) {
  const FusedApplyArgs args =
      check_fused_apply(weight, state, grad_out, lr, adagrad, sr, adam_step,
                        beta1, beta2, values.numel(), row_splits.numel() - 1);
  // the plan's own checks of the ids come before its first launch
  const SortPlan plan =
      csr_sort_plan(values, row_splits, weight.size(0), mean, per_id_w);
  apply_sort_plan(weight, state, plan, grad_out, lr, adagrad, eps, args,
                  adam_step, beta1, beta2, deterministic);
}

// fp32 [n] -> bf16 [n], stochastically rounded with the bits the fused
// optimizers use for table offsets base_offset .. base_offset + n - 1.
torch::Tensor stochastic_round_bf16(torch::Tensor x, int64_t seed,
                                    int64_t step, int64_t base_offset) {
  CHECK_CUDA(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.dtype() == torch::kFloat32, "x must be fp32");
  TORCH_CHECK(base_offset >= 0, "base_offset must not be negative");
  auto out = torch::empty(x.sizes(), x.options().dtype(torch::kBFloat16));
  launch_stochastic_round_bf16(x.data_ptr<float>(), out.data_ptr(), x.numel(),
                               seed, step, base_offset, current_stream());
  return out;
}

// The flat id vector of one fused lookup group, one segment per list entry in
// order (csrc/pack_ids.hip).  expand[i] false: srcs[i] holds rows * h_out[i]
// ids that are copied; true: srcs[i] holds one id per row and each is expanded
// to h_out[i] ids with (vocab[i], key_f[i]).  offset[i] is added to every id
// of the segment.  key_f carries a uint64 bit pattern.
torch::Tensor pack_ids(std::vector<torch::Tensor> srcs,
                       std::vector<int64_t> h_out, std::vector<bool> expand,
                       std::vector<int64_t> vocab, std::vector<int64_t> key_f,
                       std::vector<int64_t> offset) {
  const size_t nseg = srcs.size();
  TORCH_CHECK(nseg >= 1, "pack_ids needs at least one segment");
  TORCH_CHECK(h_out.size() == nseg && expand.size() == nseg &&
                  vocab.size() == nseg && key_f.size() == nseg &&
                  offset.size() == nseg,
              "pack_ids: every list must have one entry per segment");
  TORCH_CHECK(nseg <= (size_t)INT32_MAX, "pack_ids: too many segments");
  std::vector<PackIdsSegment> segs(nseg);
  int64_t total = 0;
  for (size_t i = 0; i < nseg; ++i) {
    const auto& src = srcs[i];
    TORCH_CHECK(src.is_cuda(), "pack_ids: segment ", i, " must be on GPU");
    TORCH_CHECK(src.device() == srcs[0].device(),
                "pack_ids: all segments must be on the same device");
    TORCH_CHECK(src.dtype() == torch::kInt64,
                "pack_ids: segment ", i, " must be int64");
    TORCH_CHECK(src.is_contiguous(),
                "pack_ids: segment ", i, " must be contiguous");
    TORCH_CHECK(h_out[i] >= 1 && h_out[i] <= INT32_MAX,
                "pack_ids: h_out must be >= 1 (segment ", i, ")");
    PackIdsSegment& s = segs[i];
    s.src = src.data_ptr<int64_t>();
    s.h_out = (int32_t)h_out[i];
    if (expand[i]) {
      TORCH_CHECK(vocab[i] >= 1,
                  "pack_ids: an expand segment needs vocab >= 1");
      s.mode = kPackIdsExpand;
      s.rows = src.numel();
    } else {
      TORCH_CHECK(src.numel() % h_out[i] == 0, "pack_ids: segment ", i,
                  " does not hold whole rows of ", h_out[i], " ids");
      s.mode = kPackIdsCopy;
      s.rows = src.numel() / h_out[i];
    }
    s.vocab = vocab[i];
    s.key_f = (uint64_t)key_f[i];
    s.offset = offset[i];
    s.dst_begin = total;
    total += s.rows * h_out[i];
  }
  auto out = torch::empty({total}, srcs[0].options());
  if (total > 0) {
    launch_pack_ids(segs.data(), (int)nseg, out.data_ptr<int64_t>(),
                    current_stream());
  }
  return out;
}

// Shapes the interaction kernels take: the 32-row kernels serve F <= 32, the
// 64-row kernels 33 <= F <= 64 at D <= 256 (their LDS block).
static void check_dot_interact_shape(int64_t F, int64_t D) {
  TORCH_CHECK(F >= 1 && D >= 32 && D % 32 == 0 &&
                  (F <= 32 || (F <= 64 && D <= 256)),
              "F<=32 and D%32==0, or F<=64, D%32==0 and D<=256 required "
              "(got F=", F, ", D=", D, ")");
}

torch::Tensor dot_interact_fwd(torch::Tensor feats, int64_t out_w) {
  CHECK_CUDA(feats); CHECK_CONTIG(feats);
  TORCH_CHECK(feats.dtype() == torch::kBFloat16, "feats must be bf16");
  TORCH_CHECK(feats.dim() == 3, "feats must be [B, F, D]");
  const int64_t B = feats.size(0);
  check_dot_interact_shape(feats.size(1), feats.size(2));
  const int F = (int)feats.size(1), D = (int)feats.size(2);
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(out_w >= tri_n + D, "out width too small");
  auto out = torch::empty({B, out_w}, feats.options());
  (F <= 32 ? launch_dot_interact_fwd : launch_dot_interact_fwd64)(
      feats.data_ptr(), out.data_ptr(), B, F, D, (int)out_w, tri_n,
      current_stream());
  return out;
}

// sample_major=false: packed is [P, B, D] (a2a recv layout, world>1);
// sample_major=true: packed is [B, P, D] (world==1 zero-copy lookup output —
// each sample's feature rows are adjacent, so reads/writes stay local).
torch::Tensor dot_interact_fwd_packed(torch::Tensor bottom,
                                      torch::Tensor packed, torch::Tensor perm,
                                      int64_t out_w, bool sample_major) {
  CHECK_CUDA(bottom); CHECK_CUDA(packed); CHECK_CUDA(perm);
  CHECK_CONTIG(bottom); CHECK_CONTIG(packed); CHECK_CONTIG(perm);
  TORCH_CHECK(bottom.dtype() == torch::kBFloat16 &&
              packed.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(bottom.dim() == 2 && packed.dim() == 3, "bottom [B,D], packed 3-D");
  const int64_t B = bottom.size(0);
  const int D = (int)bottom.size(1);
  const int P = (int)(sample_major ? packed.size(1) : packed.size(0));
  TORCH_CHECK(packed.size(sample_major ? 0 : 1) == B && packed.size(2) == D,
              "shape mismatch");
  TORCH_CHECK(perm.numel() == P, "perm must have P entries");
  check_dot_interact_shape((int64_t)P + 1, bottom.size(1));
  const int F = P + 1;
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(out_w >= tri_n + D, "out width too small");
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto out = torch::empty({B, out_w}, bottom.options());
  (F <= 32 ? launch_dot_interact_fwd_packed : launch_dot_interact_fwd_packed64)(
      bottom.data_ptr(), packed.data_ptr(), perm.data_ptr<int>(),
      out.data_ptr(), B, F, D, (int)out_w, tri_n, sb, sp, current_stream());
  return out;
}

std::vector<torch::Tensor> dot_interact_bwd_packed(torch::Tensor gout,
                                                   torch::Tensor bottom,
                                                   torch::Tensor packed,
                                                   torch::Tensor perm,
                                                   bool sample_major) {
  CHECK_CUDA(gout); CHECK_CUDA(bottom); CHECK_CUDA(packed); CHECK_CUDA(perm);
  CHECK_CONTIG(gout); CHECK_CONTIG(bottom); CHECK_CONTIG(packed);
  CHECK_CONTIG(perm);
  TORCH_CHECK(gout.dtype() == torch::kBFloat16 &&
              bottom.dtype() == torch::kBFloat16 &&
              packed.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(gout.dim() == 2 && bottom.dim() == 2 && packed.dim() == 3,
              "gout [B,W], bottom [B,D], packed 3-D");
  const int64_t B = bottom.size(0);
  const int D = (int)bottom.size(1);
  const int P = (int)(sample_major ? packed.size(1) : packed.size(0));
  TORCH_CHECK(perm.numel() == P, "perm must have P entries");
  TORCH_CHECK(packed.size(sample_major ? 0 : 1) == B && packed.size(2) == D,
              "shape mismatch");
  check_dot_interact_shape((int64_t)P + 1, bottom.size(1));
  const int F = P + 1;
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(gout.size(0) == B && gout.size(1) >= tri_n + D,
              "gout must be [B, >= F(F-1)/2 + D]");
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto gbottom = torch::empty_like(bottom);
  auto gpacked = torch::empty_like(packed);
  (F <= 32 ? launch_dot_interact_bwd_packed : launch_dot_interact_bwd_packed64)(
      gout.data_ptr(), bottom.data_ptr(), packed.data_ptr(),
      perm.data_ptr<int>(), gbottom.data_ptr(), gpacked.data_ptr(), B, F, D,
      (int)gout.size(1), tri_n, sb, sp, current_stream());
  return {gbottom, gpacked};
}

torch::Tensor dot_interact_bwd(torch::Tensor gout, torch::Tensor feats) {
  CHECK_CUDA(gout); CHECK_CUDA(feats);
  CHECK_CONTIG(gout); CHECK_CONTIG(feats);
  TORCH_CHECK(gout.dtype() == torch::kBFloat16 &&
              feats.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(gout.dim() == 2 && feats.dim() == 3,
              "gout [B,W], feats [B,F,D]");
  const int64_t B = feats.size(0);
  check_dot_interact_shape(feats.size(1), feats.size(2));
  const int F = (int)feats.size(1), D = (int)feats.size(2);
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(gout.size(0) == B && gout.size(1) >= tri_n + D,
              "gout must be [B, >= F(F-1)/2 + D]");
  auto gfeats = torch::empty_like(feats);
  (F <= 32 ? launch_dot_interact_bwd : launch_dot_interact_bwd64)(
      gout.data_ptr(), feats.data_ptr(), gfeats.data_ptr(), B, F, D,
      (int)gout.size(1), tri_n, current_stream());
  return gfeats;
}

// Narrow widths (D = 8, 16, 24; F <= 32): bindings of their own, so that the
// four above keep rejecting these shapes.  The kernels move every feature row
// as 16-B vectors, so the feature tensors must start on a 16-B boundary (rows
// of 16, 32 or 48 bytes then do too); out / gout rows are 2-byte aligned.
// As for the siblings, perm must be a permutation of [0, P): the backward
// writes the rows of gpacked that perm names and leaves any other as
// allocated.
static void check_dot_interact_narrow_shape(int64_t F, int64_t D) {
  TORCH_CHECK((D == 8 || D == 16 || D == 24) && F >= 1 && F <= 32,
              "D in {8, 16, 24} and 1 <= F <= 32 required (got F=", F,
              ", D=", D, ")");
}

static void check_align16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}

torch::Tensor dot_interact_narrow_fwd(torch::Tensor feats, int64_t out_w) {
  CHECK_CUDA(feats); CHECK_CONTIG(feats);
  TORCH_CHECK(feats.dtype() == torch::kBFloat16, "feats must be bf16");
  TORCH_CHECK(feats.dim() == 3, "feats must be [B, F, D]");
  const int64_t B = feats.size(0);
  check_dot_interact_narrow_shape(feats.size(1), feats.size(2));
  check_align16(feats, "feats");
  const int F = (int)feats.size(1), D = (int)feats.size(2);
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(out_w >= tri_n + D, "out width too small");
  auto out = torch::empty({B, out_w}, feats.options());
  launch_dot_interact_fwd_narrow(feats.data_ptr(), out.data_ptr(), B, F, D,
                                 (int)out_w, tri_n, current_stream());
  return out;
}

torch::Tensor dot_interact_narrow_bwd(torch::Tensor gout, torch::Tensor feats) {
  CHECK_CUDA(gout); CHECK_CUDA(feats);
  CHECK_CONTIG(gout); CHECK_CONTIG(feats);
  TORCH_CHECK(gout.dtype() == torch::kBFloat16 &&
              feats.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(gout.dim() == 2 && feats.dim() == 3,
              "gout [B,W], feats [B,F,D]");
  const int64_t B = feats.size(0);
  check_dot_interact_narrow_shape(feats.size(1), feats.size(2));
  check_align16(feats, "feats");
  const int F = (int)feats.size(1), D = (int)feats.size(2);
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(gout.size(0) == B && gout.size(1) >= tri_n + D,
              "gout must be [B, >= F(F-1)/2 + D]");
  auto gfeats = torch::empty_like(feats);
  launch_dot_interact_bwd_narrow(gout.data_ptr(), feats.data_ptr(),
                                 gfeats.data_ptr(), B, F, D, (int)gout.size(1),
                                 tri_n, current_stream());
  return gfeats;
}

torch::Tensor dot_interact_narrow_fwd_packed(torch::Tensor bottom,
                                             torch::Tensor packed,
                                             torch::Tensor perm, int64_t out_w,
                                             bool sample_major) {
  CHECK_CUDA(bottom); CHECK_CUDA(packed); CHECK_CUDA(perm);
  CHECK_CONTIG(bottom); CHECK_CONTIG(packed); CHECK_CONTIG(perm);
  TORCH_CHECK(bottom.dtype() == torch::kBFloat16 &&
              packed.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(bottom.dim() == 2 && packed.dim() == 3, "bottom [B,D], packed 3-D");
  const int64_t B = bottom.size(0);
  const int D = (int)bottom.size(1);
  const int P = (int)(sample_major ? packed.size(1) : packed.size(0));
  TORCH_CHECK(packed.size(sample_major ? 0 : 1) == B && packed.size(2) == D,
              "shape mismatch");
  TORCH_CHECK(perm.numel() == P, "perm must have P entries");
  check_dot_interact_narrow_shape((int64_t)P + 1, bottom.size(1));
  check_align16(bottom, "bottom");
  check_align16(packed, "packed");
  const int F = P + 1;
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(out_w >= tri_n + D, "out width too small");
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto out = torch::empty({B, out_w}, bottom.options());
  launch_dot_interact_fwd_narrow_packed(
      bottom.data_ptr(), packed.data_ptr(), perm.data_ptr<int>(),
      out.data_ptr(), B, F, D, (int)out_w, tri_n, sb, sp, current_stream());
  return out;
}

std::vector<torch::Tensor> dot_interact_narrow_bwd_packed(torch::Tensor gout,
                                                          torch::Tensor bottom,
                                                          torch::Tensor packed,
                                                          torch::Tensor perm,
                                                          bool sample_major) {
  CHECK_CUDA(gout); CHECK_CUDA(bottom); CHECK_CUDA(packed); CHECK_CUDA(perm);
  CHECK_CONTIG(gout); CHECK_CONTIG(bottom); CHECK_CONTIG(packed);
  CHECK_CONTIG(perm);
  TORCH_CHECK(gout.dtype() == torch::kBFloat16 &&
              bottom.dtype() == torch::kBFloat16 &&
              packed.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(gout.dim() == 2 && bottom.dim() == 2 && packed.dim() == 3,
              "gout [B,W], bottom [B,D], packed 3-D");
  const int64_t B = bottom.size(0);
  const int D = (int)bottom.size(1);
  const int P = (int)(sample_major ? packed.size(1) : packed.size(0));
  TORCH_CHECK(perm.numel() == P, "perm must have P entries");
  TORCH_CHECK(packed.size(sample_major ? 0 : 1) == B && packed.size(2) == D,
              "shape mismatch");
  check_dot_interact_narrow_shape((int64_t)P + 1, bottom.size(1));
  check_align16(bottom, "bottom");
  check_align16(packed, "packed");
  const int F = P + 1;
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(gout.size(0) == B && gout.size(1) >= tri_n + D,
              "gout must be [B, >= F(F-1)/2 + D]");
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto gbottom = torch::empty_like(bottom);
  auto gpacked = torch::empty_like(packed);
  launch_dot_interact_bwd_narrow_packed(
      gout.data_ptr(), bottom.data_ptr(), packed.data_ptr(),
      perm.data_ptr<int>(), gbottom.data_ptr(), gpacked.data_ptr(), B, F, D,
      (int)gout.size(1), tri_n, sb, sp, current_stream());
  return {gbottom, gpacked};
}

// fp32 inputs (dot_interact_f32.hip): 1 <= F <= 32, D % 8 == 0, 8 <= D <= 256,
// fp32 in and out.  Feature rows move as 16-B vectors, so the feature tensors
// must start on a 16-B boundary; out / gout rows are 4-byte aligned.  perm as
// for the narrow bindings.
static void check_dot_interact_f32_shape(int64_t F, int64_t D) {
  TORCH_CHECK(F >= 1 && F <= 32 && D >= 8 && D <= 256 && D % 8 == 0,
              "1 <= F <= 32, D % 8 == 0 and 8 <= D <= 256 required (got F=", F,
              ", D=", D, ")");
}

static void check_f32(const torch::Tensor& t, const char* name) {
  CHECK_CUDA(t); CHECK_CONTIG(t);
  TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be float32");
}

// (F, D, sb, sp) of a checked (bottom, packed, perm) triple
struct F32Packed {
  int64_t B, sb, sp;
  int F, D, tri_n;
};

static F32Packed check_f32_packed(const torch::Tensor& bottom,
                                  const torch::Tensor& packed,
                                  const torch::Tensor& perm,
                                  bool sample_major) {
  check_f32(bottom, "bottom");
  check_f32(packed, "packed");
  CHECK_CUDA(perm); CHECK_CONTIG(perm);
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(packed.device() == bottom.device() &&
              perm.device() == bottom.device(), "tensors on one device");
  TORCH_CHECK(bottom.dim() == 2 && packed.dim() == 3, "bottom [B,D], packed 3-D");
  const int64_t B = bottom.size(0), D = bottom.size(1);
  const int64_t P = sample_major ? packed.size(1) : packed.size(0);
  TORCH_CHECK(packed.size(sample_major ? 0 : 1) == B && packed.size(2) == D,
              "shape mismatch");
  TORCH_CHECK(perm.numel() == P, "perm must have P entries");
  check_dot_interact_f32_shape(P + 1, D);
  check_align16(bottom, "bottom");
  check_align16(packed, "packed");
  const int F = (int)P + 1;
  return {B, sample_major ? P : 1, sample_major ? 1 : B, F, (int)D,
          F * (F - 1) / 2};
}

torch::Tensor dot_interact_f32_fwd(torch::Tensor feats, int64_t out_w) {
  check_f32(feats, "feats");
  TORCH_CHECK(feats.dim() == 3, "feats must be [B, F, D]");
  check_dot_interact_f32_shape(feats.size(1), feats.size(2));
  check_align16(feats, "feats");
  const int64_t B = feats.size(0);
  const int F = (int)feats.size(1), D = (int)feats.size(2);
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(out_w >= tri_n + D && out_w <= INT32_MAX, "out width too small");
  auto out = torch::empty({B, out_w}, feats.options());
  launch_dot_interact_f32_fwd(feats.data_ptr(), out.data_ptr(), B, F, D,
                              (int)out_w, tri_n, current_stream());
  return out;
}

torch::Tensor dot_interact_f32_bwd(torch::Tensor gout, torch::Tensor feats) {
  check_f32(gout, "gout");
  check_f32(feats, "feats");
  TORCH_CHECK(gout.device() == feats.device(), "tensors on one device");
  TORCH_CHECK(gout.dim() == 2 && feats.dim() == 3, "gout [B,W], feats [B,F,D]");
  check_dot_interact_f32_shape(feats.size(1), feats.size(2));
  check_align16(feats, "feats");
  const int64_t B = feats.size(0);
  const int F = (int)feats.size(1), D = (int)feats.size(2);
  const int tri_n = F * (F - 1) / 2;
  TORCH_CHECK(gout.size(0) == B && gout.size(1) >= tri_n + D &&
              gout.size(1) <= INT32_MAX, "gout must be [B, >= F(F-1)/2 + D]");
  auto gfeats = torch::empty_like(feats);
  launch_dot_interact_f32_bwd(gout.data_ptr(), feats.data_ptr(),
                              gfeats.data_ptr(), B, F, D, (int)gout.size(1),
                              tri_n, current_stream());
  return gfeats;
}

torch::Tensor dot_interact_f32_fwd_packed(torch::Tensor bottom,
                                          torch::Tensor packed,
                                          torch::Tensor perm, int64_t out_w,
                                          bool sample_major) {
  const F32Packed s = check_f32_packed(bottom, packed, perm, sample_major);
  TORCH_CHECK(out_w >= s.tri_n + s.D && out_w <= INT32_MAX,
              "out width too small");
  auto out = torch::empty({s.B, out_w}, bottom.options());
  launch_dot_interact_f32_fwd_packed(
      bottom.data_ptr(), packed.data_ptr(), perm.data_ptr<int>(),
      out.data_ptr(), s.B, s.F, s.D, (int)out_w, s.tri_n, s.sb, s.sp,
      current_stream());
  return out;
}

std::vector<torch::Tensor> dot_interact_f32_bwd_packed(torch::Tensor gout,
                                                       torch::Tensor bottom,
                                                       torch::Tensor packed,
                                                       torch::Tensor perm,
                                                       bool sample_major) {
  check_f32(gout, "gout");
  const F32Packed s = check_f32_packed(bottom, packed, perm, sample_major);
  TORCH_CHECK(gout.device() == bottom.device(), "tensors on one device");
  TORCH_CHECK(gout.dim() == 2 && gout.size(0) == s.B &&
              gout.size(1) >= s.tri_n + s.D && gout.size(1) <= INT32_MAX,
              "gout must be [B, >= F(F-1)/2 + D]");
  auto gbottom = torch::empty_like(bottom);
  auto gpacked = torch::empty_like(packed);
  launch_dot_interact_f32_bwd_packed(
      gout.data_ptr(), bottom.data_ptr(), packed.data_ptr(),
      perm.data_ptr<int>(), gbottom.data_ptr(), gpacked.data_ptr(), s.B, s.F,
      s.D, (int)gout.size(1), s.tri_n, s.sb, s.sp, current_stream());
  return {gbottom, gpacked};
}

// ReLU backward fused with the bias gradient: one pass over grad_out and y
// (mlp_ops.hip).  Outputs and the fp32 partial slab come from the torch
// allocator, so the op can be captured in a hipGraph.
std::vector<torch::Tensor> relu_bwd_bias_grad(torch::Tensor grad_out,
                                              torch::Tensor y) {
  CHECK_CUDA(grad_out); CHECK_CUDA(y);
  CHECK_CONTIG(grad_out); CHECK_CONTIG(y);
  TORCH_CHECK(grad_out.dtype() == torch::kBFloat16 &&
              y.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(grad_out.dim() == 2 && grad_out.sizes() == y.sizes(),
              "grad_out and y must be [B, N]");
  const int64_t B = grad_out.size(0);
  const int64_t N = grad_out.size(1);
  TORCH_CHECK(N % 8 == 0 && N < (int64_t(1) << 31), "N % 8 == 0 required");
  auto grad_in = torch::empty_like(grad_out);
  if (B == 0 || N == 0) {
    return {grad_in, torch::zeros({N}, grad_out.options())};
  }
  auto bias_grad = torch::empty({N}, grad_out.options());
  int64_t rows_per_chunk = 0, num_chunks = 0;
  relu_bwd_bias_grad_plan(B, (int)N, &rows_per_chunk, &num_chunks);
  auto slab = torch::empty({num_chunks, N},
                           grad_out.options().dtype(torch::kFloat32));
  launch_relu_bwd_bias_grad(grad_out.data_ptr(), y.data_ptr(),
                            grad_in.data_ptr(), slab.data_ptr<float>(),
                            bias_grad.data_ptr(), B, (int)N, rows_per_chunk,
                            num_chunks, current_stream());
  return {grad_in, bias_grad};
}

#define CHECK_ALIGN16(x)                                                     \
  TORCH_CHECK(reinterpret_cast<uintptr_t>((x).data_ptr()) % 16 == 0,         \
              #x " must be 16-byte aligned")

// Elementwise backward of one low-rank cross layer x_{l+1} = x0 * u + x_l
// (mlp_ops.hip): gu = G * x0, gb = column sums of gu and, in place,
// acc = (init ? 0 : acc) + G * u, from one pass.  Returns (gu, gb).  Outputs
// and the fp32 partial slab come from the torch allocator and both launches
// go on the current stream, so the op can be captured in a hipGraph.
// f32: fp32 tensors with N % 4 == 0 (cross_bwd_f32), else bf16 with N % 8.
static std::vector<torch::Tensor> cross_bwd_impl(torch::Tensor G,
                                                 torch::Tensor x0,
                                                 torch::Tensor u,
                                                 torch::Tensor acc, bool init,
                                                 bool f32) {
  CHECK_CUDA(G); CHECK_CUDA(x0); CHECK_CUDA(u); CHECK_CUDA(acc);
  CHECK_CONTIG(G); CHECK_CONTIG(x0); CHECK_CONTIG(u); CHECK_CONTIG(acc);
  const auto dtype = f32 ? torch::kFloat32 : torch::kBFloat16;
  TORCH_CHECK(G.dtype() == dtype && x0.dtype() == dtype &&
              u.dtype() == dtype && acc.dtype() == dtype,
              f32 ? "fp32 required" : "bf16 required");
  TORCH_CHECK(G.dim() == 2 && G.sizes() == x0.sizes() &&
              G.sizes() == u.sizes() && G.sizes() == acc.sizes(),
              "G, x0, u and acc must be [B, N]");
  TORCH_CHECK(G.device() == x0.device() && G.device() == u.device() &&
              G.device() == acc.device(), "operands must share a device");
  const int64_t B = G.size(0);
  const int64_t N = G.size(1);
  TORCH_CHECK(N % (f32 ? 4 : 8) == 0 && N < (int64_t(1) << 31),
              f32 ? "N % 4 == 0 required" : "N % 8 == 0 required");
  CHECK_ALIGN16(G); CHECK_ALIGN16(x0); CHECK_ALIGN16(u); CHECK_ALIGN16(acc);
  auto gu = torch::empty_like(G);
  if (B == 0 || N == 0) {
    return {gu, torch::zeros({N}, G.options())};
  }
  TORCH_CHECK(acc.data_ptr() != G.data_ptr() &&
              acc.data_ptr() != x0.data_ptr() &&
              acc.data_ptr() != u.data_ptr(),
              "acc is written in place and must not alias an input");
  auto gb = torch::empty({N}, G.options());
  int64_t rows_per_chunk = 0, num_chunks = 0;
  relu_bwd_bias_grad_plan(B, (int)N, &rows_per_chunk, &num_chunks);
  auto slab = torch::empty({num_chunks, N},
                           G.options().dtype(torch::kFloat32));
  (f32 ? launch_cross_bwd_f32 : launch_cross_bwd)(
      G.data_ptr(), x0.data_ptr(), u.data_ptr(), acc.data_ptr(), init,
      gu.data_ptr(), slab.data_ptr<float>(), gb.data_ptr(), B, (int)N,
      rows_per_chunk, num_chunks, current_stream());
  return {gu, gb};
}

std::vector<torch::Tensor> cross_bwd(torch::Tensor G, torch::Tensor x0,
                                     torch::Tensor u, torch::Tensor acc,
                                     bool init) {
  return cross_bwd_impl(G, x0, u, acc, init, false);
}

std::vector<torch::Tensor> cross_bwd_f32(torch::Tensor G, torch::Tensor x0,
                                         torch::Tensor u, torch::Tensor acc,
                                         bool init) {
  return cross_bwd_impl(G, x0, u, acc, init, true);
}

// Shapes of the cross interaction's input assembly: bottom [B, D], packed
// [P, B, D] (feature-major) or [B, P, D] (sample-major), x0 [B, (P+1)*D].
// vec is the elements of a 16-byte chunk: 8 for bf16, 4 for fp32.
static void check_cross_concat_shape(int64_t B, int64_t P, int64_t D,
                                     int64_t vec) {
  TORCH_CHECK(P >= 1 && D >= vec && D % vec == 0,
              "P >= 1 and D % ", vec, " == 0 required (got P=", P, ", D=", D,
              ")");
  // a block walks 16 rows of x0 with 32-bit indices: 2^27 bf16, 2^26 fp32
  TORCH_CHECK((P + 1) * D < (int64_t(1) << 24) * vec, "row of x0 too wide");
  TORCH_CHECK(B >= 0, "negative batch");
}

static torch::Tensor cross_concat_fwd_impl(torch::Tensor bottom,
                                           torch::Tensor packed,
                                           torch::Tensor perm,
                                           bool sample_major, bool f32) {
  CHECK_CUDA(bottom); CHECK_CUDA(packed); CHECK_CUDA(perm);
  CHECK_CONTIG(bottom); CHECK_CONTIG(packed); CHECK_CONTIG(perm);
  const auto dtype = f32 ? torch::kFloat32 : torch::kBFloat16;
  TORCH_CHECK(bottom.dtype() == dtype && packed.dtype() == dtype,
              f32 ? "fp32 required" : "bf16 required");
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(bottom.dim() == 2 && packed.dim() == 3,
              "bottom [B,D], packed 3-D");
  TORCH_CHECK(bottom.device() == packed.device() &&
              bottom.device() == perm.device(),
              "operands must share a device");
  const int64_t B = bottom.size(0);
  const int64_t D = bottom.size(1);
  const int64_t P = sample_major ? packed.size(1) : packed.size(0);
  TORCH_CHECK(packed.size(sample_major ? 0 : 1) == B && packed.size(2) == D,
              "shape mismatch");
  TORCH_CHECK(perm.numel() == P, "perm must have P entries");
  check_cross_concat_shape(B, P, D, f32 ? 4 : 8);
  CHECK_ALIGN16(bottom); CHECK_ALIGN16(packed);
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto x0 = torch::empty({B, (P + 1) * D}, bottom.options());
  (f32 ? launch_cross_concat_f32_fwd : launch_cross_concat_fwd)(
      bottom.data_ptr(), packed.data_ptr(), perm.data_ptr<int>(),
      x0.data_ptr(), B, (int)P, (int)D, sb, sp, current_stream());
  return x0;
}

torch::Tensor cross_concat_fwd(torch::Tensor bottom, torch::Tensor packed,
                               torch::Tensor perm, bool sample_major) {
  return cross_concat_fwd_impl(bottom, packed, perm, sample_major, false);
}

torch::Tensor cross_concat_f32_fwd(torch::Tensor bottom, torch::Tensor packed,
                                   torch::Tensor perm, bool sample_major) {
  return cross_concat_fwd_impl(bottom, packed, perm, sample_major, true);
}

// (gbottom [B, D], gpacked in packed's layout) from gx0 [B, (P+1)*D]; perm
// has to be a permutation of [0, P).
static std::vector<torch::Tensor> cross_concat_bwd_impl(torch::Tensor gx0,
                                                        torch::Tensor perm,
                                                        bool sample_major,
                                                        bool f32) {
  CHECK_CUDA(gx0); CHECK_CUDA(perm);
  CHECK_CONTIG(gx0); CHECK_CONTIG(perm);
  TORCH_CHECK(gx0.dtype() == (f32 ? torch::kFloat32 : torch::kBFloat16),
              f32 ? "fp32 required" : "bf16 required");
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(gx0.dim() == 2 && perm.dim() == 1 && perm.numel() >= 1,
              "gx0 [B, (P+1)*D], perm [P]");
  TORCH_CHECK(gx0.device() == perm.device(), "operands must share a device");
  const int64_t B = gx0.size(0);
  const int64_t P = perm.numel();
  TORCH_CHECK(gx0.size(1) % (P + 1) == 0,
              "gx0 width must be a multiple of P + 1");
  const int64_t D = gx0.size(1) / (P + 1);
  check_cross_concat_shape(B, P, D, f32 ? 4 : 8);
  CHECK_ALIGN16(gx0);
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto gbottom = torch::empty({B, D}, gx0.options());
  auto gpacked = sample_major ? torch::empty({B, P, D}, gx0.options())
                              : torch::empty({P, B, D}, gx0.options());
  (f32 ? launch_cross_concat_f32_bwd : launch_cross_concat_bwd)(
      gx0.data_ptr(), perm.data_ptr<int>(), gbottom.data_ptr(),
      gpacked.data_ptr(), B, (int)P, (int)D, sb, sp, current_stream());
  return {gbottom, gpacked};
}

std::vector<torch::Tensor> cross_concat_bwd(torch::Tensor gx0,
                                            torch::Tensor perm,
                                            bool sample_major) {
  return cross_concat_bwd_impl(gx0, perm, sample_major, false);
}

std::vector<torch::Tensor> cross_concat_f32_bwd(torch::Tensor gx0,
                                                torch::Tensor perm,
                                                bool sample_major) {
  return cross_concat_bwd_impl(gx0, perm, sample_major, true);
}

// Concat + average pool (csrc/concat_pool.hip).  The kernels take bf16 and
// fp32 only, on both sides.
static bool concat_pool_is_bf16(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.dtype() == torch::kBFloat16 || t.dtype() == torch::kFloat32,
              "concat_pool: ", what, " must be bf16 or fp32");
  return t.dtype() == torch::kBFloat16;
}

static void check_concat_pool_shape(int64_t B, int64_t W, int64_t Nn,
                                    int64_t stride) {
  TORCH_CHECK(stride >= 1 && stride <= kConcatPoolMaxStride,
              "concat_pool: stride must be in [1, ", kConcatPoolMaxStride, "]");
  // columns and the rows of one tile are indexed in 32 bits
  TORCH_CHECK(W >= 1 && W + Nn < (int64_t(1) << 25),
              "concat_pool: row too wide");
  TORCH_CHECK(B >= 0, "negative batch");
}

// out [B, ceil(W / stride) + Nn] from inputs[t] [B, w_t] and numerical
// [B, Nn]: no sync, one allocation, launches on the current stream.
torch::Tensor concat_pool_fwd(std::vector<torch::Tensor> inputs,
                              std::optional<torch::Tensor> numerical,
                              int64_t stride, bool out_bf16) {
  TORCH_CHECK(!inputs.empty(), "concat_pool: needs at least one input");
  const auto& first = inputs[0];
  CHECK_CUDA(first);
  TORCH_CHECK(first.dim() == 2, "concat_pool: inputs must be [B, w]");
  const bool in_bf16 = concat_pool_is_bf16(first, "inputs");
  const int64_t ch = in_bf16 ? 8 : 4;
  const int64_t B = first.size(0);
  std::vector<ConcatPoolInput> descs(inputs.size());
  int64_t W = 0;
  for (size_t t = 0; t < inputs.size(); ++t) {
    const auto& x = inputs[t];
    TORCH_CHECK(x.is_cuda() && x.device() == first.device() &&
                x.dtype() == first.dtype() && x.dim() == 2 && x.size(0) == B,
                "concat_pool: input ", t, " must match input 0 in device, "
                "dtype and batch");
    TORCH_CHECK(x.is_contiguous(), "concat_pool: input ", t,
                " must be contiguous");
    TORCH_CHECK(x.size(1) >= ch && x.size(1) % ch == 0, "concat_pool: input ",
                t, " must have a width that is a multiple of ", ch);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
                "concat_pool: input ", t, " must be 16-byte aligned");
    TORCH_CHECK(W + x.size(1) < (int64_t(1) << 25), "concat_pool: row too wide");
    descs[t] = {x.data_ptr(), (int32_t)W, (int32_t)x.size(1)};
    W += x.size(1);
  }
  int64_t Nn = 0;
  bool num_bf16 = false;
  const void* num_ptr = nullptr;
  if (numerical.has_value()) {
    const auto& num = *numerical;
    CHECK_CUDA(num); CHECK_CONTIG(num);
    TORCH_CHECK(num.dim() == 2 && num.size(0) == B &&
                num.device() == first.device(),
                "concat_pool: numerical must be [B, Nn] on the inputs' device");
    num_bf16 = concat_pool_is_bf16(num, "numerical");
    Nn = num.size(1);
    num_ptr = num.data_ptr();
  }
  check_concat_pool_shape(B, W, Nn, stride);
  const int64_t Wp = (W + stride - 1) / stride;
  auto out = torch::empty(
      {B, Wp + Nn},
      first.options().dtype(out_bf16 ? torch::kBFloat16 : torch::kFloat32));
  launch_concat_pool_fwd(descs.data(), (int)descs.size(), in_bf16, num_ptr,
                         num_bf16, (int)Nn, out.data_ptr(), out_bf16, B,
                         (int)W, (int)stride, current_stream());
  return out;
}

// The inputs' gradients from gout [B, ceil(W / stride) + Nn]: contiguous
// [B, widths[t]] views, in input order, of one flat allocation.
std::vector<torch::Tensor> concat_pool_bwd(torch::Tensor gout,
                                           std::vector<int64_t> widths,
                                           int64_t stride, int64_t Nn,
                                           bool in_bf16) {
  CHECK_CUDA(gout); CHECK_CONTIG(gout);
  TORCH_CHECK(gout.dim() == 2 && !widths.empty() && Nn >= 0,
              "concat_pool: gout must be [B, Wp + Nn]");
  const bool gout_bf16 = concat_pool_is_bf16(gout, "gout");
  const int64_t ch = in_bf16 ? 8 : 4;
  const int64_t B = gout.size(0);
  int64_t W = 0;
  for (int64_t w : widths) {
    TORCH_CHECK(w >= ch && w % ch == 0,
                "concat_pool: widths must be multiples of ", ch);
    W += w;
    TORCH_CHECK(W < (int64_t(1) << 25), "concat_pool: row too wide");
  }
  check_concat_pool_shape(B, W, Nn, stride);
  TORCH_CHECK(gout.size(1) == (W + stride - 1) / stride + Nn,
              "concat_pool: gout has the wrong width");
  auto flat = torch::empty(
      {B * W},
      gout.options().dtype(in_bf16 ? torch::kBFloat16 : torch::kFloat32));
  std::vector<torch::Tensor> gins(widths.size());
  std::vector<ConcatPoolInput> descs(widths.size());
  int64_t begin = 0;
  for (size_t t = 0; t < widths.size(); ++t) {
    // B * begin elements: a multiple of 16 bytes, as begin is one of ch
    gins[t] = flat.narrow(0, B * begin, B * widths[t]).view({B, widths[t]});
    descs[t] = {gins[t].data_ptr(), (int32_t)begin, (int32_t)widths[t]};
    begin += widths[t];
  }
  launch_concat_pool_bwd(gout.data_ptr(), gout_bf16, descs.data(),
                         (int)descs.size(), in_bf16, (int)Nn, B, (int)W,
                         (int)stride, current_stream());
  return gins;
}

// Weight gradient of a Linear layer, gw = bf16(g^T x) with fp32 accumulation
// (wgrad_splitk.hip).  The slab comes from the torch allocator and both
// launches go on the current stream: capturable.  splitk > 0 and tile >= 0
// replace the plan's number of K-slices and tile geometry.
torch::Tensor wgrad_splitk(torch::Tensor g, torch::Tensor x, int64_t splitk,
                           int64_t tile) {
  CHECK_CUDA(g); CHECK_CUDA(x);
  CHECK_CONTIG(g); CHECK_CONTIG(x);
  TORCH_CHECK(g.dtype() == torch::kBFloat16 && x.dtype() == torch::kBFloat16,
              "bf16 required");
  TORCH_CHECK(g.dim() == 2 && x.dim() == 2 && g.size(0) == x.size(0),
              "g must be [K, M] and x [K, N]");
  const int64_t K = g.size(0), M = g.size(1), N = x.size(1);
  TORCH_CHECK(splitk >= 0, "splitk must not be negative");
  TORCH_CHECK(tile >= -1 && tile <= 2, "tile must be -1 (plan), 0, 1 or 2");
  WgradSplitkPlan plan;
  TORCH_CHECK(wgrad_splitk_plan_with(K, M, N, splitk, (int)tile, &plan),
              "wgrad_splitk takes K >= 1, M % 8 == 0 and N % 8 == 0 or "
              "N <= 16 (tile 2 for N <= 16 only); got K=", K, " M=", M,
              " N=", N, " tile=", tile);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "operands must be 16-byte aligned");
  auto gw = torch::empty({M, N}, g.options());
  auto slab = torch::empty({plan.splitk, M, plan.np},
                           g.options().dtype(torch::kFloat32));
  launch_wgrad_splitk(g.data_ptr(), x.data_ptr(), slab.data_ptr<float>(),
                      gw.data_ptr(), K, (int)M, (int)N, plan,
                      current_stream());
  return gw;
}

// (use, splitk, tile geometry) of the plan; use == false also for shapes the
// kernels do not take
std::vector<int64_t> wgrad_splitk_plan_py(int64_t K, int64_t M, int64_t N) {
  WgradSplitkPlan plan;
  if (!wgrad_splitk_plan(K, M, N, &plan)) return {0, 0, -1};
  return {plan.use ? 1 : 0, plan.splitk, plan.cfg};
}

// Weight and bias gradient of a Linear with one output feature
// (wgrad_splitk.hip): (gw [1, N], gb [1]) = (bf16(g^T x), bf16(sum g)) for
// g [K, 1], x [K, N].  Slab from the torch allocator, both launches on the
// current stream: capturable.
std::vector<torch::Tensor> wgrad_gemv(torch::Tensor g, torch::Tensor x) {
  CHECK_CUDA(g); CHECK_CUDA(x);
  CHECK_CONTIG(g); CHECK_CONTIG(x);
  TORCH_CHECK(g.dtype() == torch::kBFloat16 && x.dtype() == torch::kBFloat16,
              "bf16 required");
  TORCH_CHECK(g.dim() == 2 && x.dim() == 2 && g.size(1) == 1 &&
              g.size(0) == x.size(0), "g must be [K, 1] and x [K, N]");
  TORCH_CHECK(g.device() == x.device(), "operands must share a device");
  const int64_t K = g.size(0), N = x.size(1);
  WgradGemvPlan plan;
  TORCH_CHECK(wgrad_gemv_plan(K, N, &plan),
              "wgrad_gemv takes K >= 1 and N % 8 == 0; got K=", K, " N=", N);
  CHECK_ALIGN16(x);
  auto gw = torch::empty({1, N}, g.options());
  auto gb = torch::empty({1}, g.options());
  auto slab = torch::empty({plan.num_chunks, N + 1},
                           g.options().dtype(torch::kFloat32));
  launch_wgrad_gemv(g.data_ptr(), x.data_ptr(), slab.data_ptr<float>(),
                    gw.data_ptr(), gb.data_ptr(), K, (int)N, plan,
                    current_stream());
  return {gw, gb};
}

// (use, row chunks) of the plan; use == false also for shapes the kernels do
// not take
std::vector<int64_t> wgrad_gemv_plan_py(int64_t K, int64_t N) {
  WgradGemvPlan plan;
  if (!wgrad_gemv_plan(K, N, &plan)) return {0, 0};
  return {plan.use ? 1 : 0, plan.num_chunks};
}

// The fp32 forms of the four ops above (mlp_ops.hip, wgrad_splitk_f32.hip):
// fp32 operands and fp32 results, the same checks, allocator and stream, so
// they capture into a hipGraph as well.
std::vector<torch::Tensor> relu_bwd_bias_grad_f32(torch::Tensor grad_out,
                                                  torch::Tensor y) {
  CHECK_CUDA(grad_out); CHECK_CUDA(y);
  CHECK_CONTIG(grad_out); CHECK_CONTIG(y);
  TORCH_CHECK(grad_out.dtype() == torch::kFloat32 &&
              y.dtype() == torch::kFloat32, "fp32 required");
  TORCH_CHECK(grad_out.dim() == 2 && grad_out.sizes() == y.sizes(),
              "grad_out and y must be [B, N]");
  TORCH_CHECK(grad_out.device() == y.device(), "operands must share a device");
  const int64_t B = grad_out.size(0);
  const int64_t N = grad_out.size(1);
  TORCH_CHECK(N % 4 == 0 && N < (int64_t(1) << 31), "N % 4 == 0 required");
  CHECK_ALIGN16(grad_out); CHECK_ALIGN16(y);
  auto grad_in = torch::empty_like(grad_out);
  if (B == 0 || N == 0) {
    return {grad_in, torch::zeros({N}, grad_out.options())};
  }
  auto bias_grad = torch::empty({N}, grad_out.options());
  int64_t rows_per_chunk = 0, num_chunks = 0;
  relu_bwd_bias_grad_plan(B, (int)N, &rows_per_chunk, &num_chunks);
  auto slab = torch::empty({num_chunks, N}, grad_out.options());
  launch_relu_bwd_bias_grad_f32(grad_out.data_ptr(), y.data_ptr(),
                                grad_in.data_ptr(), slab.data_ptr<float>(),
                                bias_grad.data_ptr(), B, (int)N,
                                rows_per_chunk, num_chunks, current_stream());
  return {grad_in, bias_grad};
}

torch::Tensor wgrad_splitk_f32(torch::Tensor g, torch::Tensor x,
                               int64_t splitk, int64_t tile) {
  CHECK_CUDA(g); CHECK_CUDA(x);
  CHECK_CONTIG(g); CHECK_CONTIG(x);
  TORCH_CHECK(g.dtype() == torch::kFloat32 && x.dtype() == torch::kFloat32,
              "fp32 required");
  TORCH_CHECK(g.dim() == 2 && x.dim() == 2 && g.size(0) == x.size(0),
              "g must be [K, M] and x [K, N]");
  TORCH_CHECK(g.device() == x.device(), "operands must share a device");
  const int64_t K = g.size(0), M = g.size(1), N = x.size(1);
  TORCH_CHECK(splitk >= 0, "splitk must not be negative");
  TORCH_CHECK(tile >= -1 && tile <= 2, "tile must be -1 (plan), 0, 1 or 2");
  WgradSplitkPlan plan;
  TORCH_CHECK(wgrad_splitk_f32_plan_with(K, M, N, splitk, (int)tile, &plan),
              "wgrad_splitk_f32 takes K >= 1, M % 4 == 0 and N % 4 == 0 or "
              "N <= 16 (tile 2 for N <= 16 only); got K=", K, " M=", M,
              " N=", N, " tile=", tile);
  CHECK_ALIGN16(g); CHECK_ALIGN16(x);
  auto gw = torch::empty({M, N}, g.options());
  auto slab = torch::empty({plan.splitk, M, plan.np}, g.options());
  launch_wgrad_splitk_f32(g.data_ptr(), x.data_ptr(), slab.data_ptr<float>(),
                          gw.data_ptr(), K, (int)M, (int)N, plan,
                          current_stream());
  return gw;
}

std::vector<int64_t> wgrad_splitk_f32_plan_py(int64_t K, int64_t M,
                                              int64_t N) {
  WgradSplitkPlan plan;
  if (!wgrad_splitk_f32_plan(K, M, N, &plan)) return {0, 0, -1};
  return {plan.use ? 1 : 0, plan.splitk, plan.cfg};
}

std::vector<torch::Tensor> wgrad_gemv_f32(torch::Tensor g, torch::Tensor x) {
  CHECK_CUDA(g); CHECK_CUDA(x);
  CHECK_CONTIG(g); CHECK_CONTIG(x);
  TORCH_CHECK(g.dtype() == torch::kFloat32 && x.dtype() == torch::kFloat32,
              "fp32 required");
  TORCH_CHECK(g.dim() == 2 && x.dim() == 2 && g.size(1) == 1 &&
              g.size(0) == x.size(0), "g must be [K, 1] and x [K, N]");
  TORCH_CHECK(g.device() == x.device(), "operands must share a device");
  const int64_t K = g.size(0), N = x.size(1);
  WgradGemvPlan plan;
  TORCH_CHECK(wgrad_gemv_f32_plan(K, N, &plan),
              "wgrad_gemv_f32 takes K >= 1 and N % 4 == 0; got K=", K,
              " N=", N);
  CHECK_ALIGN16(x);
  auto gw = torch::empty({1, N}, g.options());
  auto gb = torch::empty({1}, g.options());
  auto slab = torch::empty({plan.num_chunks, N + 1}, g.options());
  launch_wgrad_gemv_f32(g.data_ptr(), x.data_ptr(), slab.data_ptr<float>(),
                        gw.data_ptr(), gb.data_ptr(), K, (int)N, plan,
                        current_stream());
  return {gw, gb};
}

std::vector<int64_t> wgrad_gemv_f32_plan_py(int64_t K, int64_t N) {
  WgradGemvPlan plan;
  if (!wgrad_gemv_f32_plan(K, N, &plan)) return {0, 0};
  return {plan.use ? 1 : 0, plan.num_chunks};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("csr_lookup_forward", &csr_lookup_forward,
        "CSR segmented gather-reduce forward (gfx950)",
        pybind11::arg("params"), pybind11::arg("values"),
        pybind11::arg("row_splits"), pybind11::arg("mean"),
        pybind11::arg("out_bf16") = false,
        pybind11::arg("per_id_w") = pybind11::none(),
        pybind11::arg("deterministic") = false);
  m.def("csr_lookup_forward_q8", &csr_lookup_forward_q8,
        "CSR gather-reduce from an int8 row-wise quantized table (gfx950)",
        pybind11::arg("packed"), pybind11::arg("values"),
        pybind11::arg("row_splits"), pybind11::arg("mean"),
        pybind11::arg("out_bf16") = false,
        pybind11::arg("per_id_w") = pybind11::none(),
        pybind11::arg("deterministic") = false);
  m.def("quantize_rows_q8", &quantize_rows_q8,
        "fp32/bf16 [n, width] -> int8 row-wise packed [n, width + 8] (gfx950)",
        pybind11::arg("weight"));
  m.def("dequantize_rows_q8", &dequantize_rows_q8,
        "int8 row-wise packed [n, width + 8] -> fp32 [n, width] (gfx950)",
        pybind11::arg("packed"));
  m.def("csr_lookup_forward_q4", &csr_lookup_forward_q4,
        "CSR gather-reduce from an int4 row-wise quantized table (gfx950)",
        pybind11::arg("packed"), pybind11::arg("values"),
        pybind11::arg("row_splits"), pybind11::arg("mean"),
        pybind11::arg("out_bf16") = false,
        pybind11::arg("per_id_w") = pybind11::none(),
        pybind11::arg("deterministic") = false);
  m.def("quantize_rows_q4", &quantize_rows_q4,
        "fp32/bf16 [n, width] -> int4 row-wise packed [n, width / 2 + 4] "
        "(gfx950)",
        pybind11::arg("weight"));
  m.def("dequantize_rows_q4", &dequantize_rows_q4,
        "int4 row-wise packed [n, width / 2 + 4] -> fp32 [n, width] (gfx950)",
        pybind11::arg("packed"));
  m.def("csr_lookup_backward", &csr_lookup_backward,
        "sparse backward: sort + unique + segmented sum (gfx950)",
        pybind11::arg("grad_out"), pybind11::arg("values"),
        pybind11::arg("row_splits"), pybind11::arg("vocab"),
        pybind11::arg("mean"), pybind11::arg("per_id_w") = pybind11::none(),
        pybind11::arg("deterministic") = false);
  m.def("csr_lookup_weight_grad", &csr_lookup_weight_grad,
        "gradient of the per-id weights of a weighted lookup (gfx950)",
        pybind11::arg("grad_out"), pybind11::arg("params"),
        pybind11::arg("values"), pybind11::arg("row_splits"),
        pybind11::arg("mean"));
  m.def("debug_sort_ids", &debug_sort_ids,
        "TESTS ONLY: the backward's id sort -> (sorted_ids, sorted_pos)",
        pybind11::arg("values"), pybind11::arg("vocab"),
        pybind11::arg("variant") = -1, pybind11::arg("sort") = "default");
  m.def("debug_sorted_segments", &debug_sorted_segments,
        "TESTS ONLY: the backward's sorted-segment view -> (sorted_ids, "
        "srow, sw or None, seg, unique_ids, num_unique, bounds)",
        pybind11::arg("values"), pybind11::arg("row_splits"),
        pybind11::arg("vocab"), pybind11::arg("mean"),
        pybind11::arg("per_id_w") = pybind11::none(),
        pybind11::arg("padded") = false, pybind11::arg("variant") = -1,
        pybind11::arg("sort") = "default");
  m.def("debug_sort_variant_tiles", &debug_sort_variant_tiles,
        "TESTS ONLY: keys per block of each radix-sort tile variant");
  m.def("row_to_split", &row_to_split, "COO rows -> CSR splits (gfx950)");
  m.def("hash_rehash", &hash_rehash,
        "re-insert occupied (key,value) pairs into a larger hash (gfx950)");
  m.def("integer_lookup", &integer_lookup,
        "open-addressing hash vocab build + lookup (gfx950)");
  m.def("sparse_row_update", &sparse_row_update,
        "fused sparse SGD/Adagrad/row-wise Adagrad/lazy Adam row update "
        "(gfx950)",
        pybind11::arg("weight"), pybind11::arg("state"), pybind11::arg("ids"),
        pybind11::arg("grad"), pybind11::arg("lr"), pybind11::arg("eps"),
        pybind11::arg("adagrad"), pybind11::arg("sr") = pybind11::none(),
        pybind11::arg("adam_step") = 0, pybind11::arg("beta1") = 0.9,
        pybind11::arg("beta2") = 0.999);
  {
    // an empty plan holds no tensors: its tensor attributes read as None
    auto opt = [](const torch::Tensor& t) {
      return t.defined() ? std::optional<torch::Tensor>(t) : std::nullopt;
    };
    pybind11::class_<SortPlan>(m, "SortPlan",
                               "id-only half of the fused update, padded seg")
        .def_readonly("nnz", &SortPlan::nnz)
        .def_readonly("num_rows", &SortPlan::num_rows)
        .def_readonly("vocab", &SortPlan::vocab)
        .def_property_readonly(
            "sorted_ids",
            [opt](const SortPlan& p) { return opt(p.ss.sorted_ids); })
        .def_property_readonly(
            "srow", [opt](const SortPlan& p) { return opt(p.ss.srow); })
        .def_property_readonly(
            "sw", [opt](const SortPlan& p) { return opt(p.ss.sw); })
        .def_property_readonly(
            "seg", [opt](const SortPlan& p) { return opt(p.ss.seg); })
        .def_property_readonly(
            "unique_ids",
            [opt](const SortPlan& p) { return opt(p.ss.unique_ids); })
        .def_property_readonly(
            "num_unique",
            [opt](const SortPlan& p) { return opt(p.ss.num_unique); })
        .def_property_readonly(
            "bounds", [opt](const SortPlan& p) { return opt(p.ss.bounds); });
  }
  m.def("csr_sort_plan", &csr_sort_plan,
        "id-only half of the fused update: sorted segments of a CSR batch, "
        "seg padded (gfx950)",
        pybind11::arg("values"), pybind11::arg("row_splits"),
        pybind11::arg("vocab"), pybind11::arg("mean"),
        pybind11::arg("per_id_w") = pybind11::none());
  m.def("csr_fused_optimizer_apply_planned",
        &csr_fused_optimizer_apply_planned,
        "gradient half of the fused update on a csr_sort_plan (gfx950)",
        pybind11::arg("weight"), pybind11::arg("state"), pybind11::arg("plan"),
        pybind11::arg("grad_out"), pybind11::arg("lr"),
        pybind11::arg("adagrad"), pybind11::arg("eps"),
        pybind11::arg("sr") = pybind11::none(),
        pybind11::arg("adam_step") = pybind11::none(),
        pybind11::arg("beta1") = 0.9, pybind11::arg("beta2") = 0.999,
        pybind11::arg("deterministic") = false);
  m.def("csr_fused_optimizer_apply", &csr_fused_optimizer_apply,
        "in-backward fused SGD/Adagrad/row-wise Adagrad/lazy Adam update "
        "(gfx950)",
        pybind11::arg("weight"), pybind11::arg("state"),
        pybind11::arg("values"), pybind11::arg("row_splits"),
        pybind11::arg("grad_out"), pybind11::arg("lr"), pybind11::arg("mean"),
        pybind11::arg("adagrad"), pybind11::arg("eps"),
        pybind11::arg("per_id_w") = pybind11::none(),
        pybind11::arg("sr") = pybind11::none(),
        pybind11::arg("adam_step") = pybind11::none(),
        pybind11::arg("beta1") = 0.9, pybind11::arg("beta2") = 0.999,
        pybind11::arg("deterministic") = false);
  m.def("stochastic_round_bf16", &stochastic_round_bf16,
        "fp32 -> bf16 with the fused optimizers' stochastic rounding (gfx950)",
        pybind11::arg("x"), pybind11::arg("seed"), pybind11::arg("step") = 0,
        pybind11::arg("base_offset") = 0);
  m.def("pack_ids", &pack_ids,
        "flat id vector of a fused lookup group from copy / multi-hot expand "
        "segments, one pass (gfx950)",
        pybind11::arg("srcs"), pybind11::arg("h_out"), pybind11::arg("expand"),
        pybind11::arg("vocab"), pybind11::arg("key_f"),
        pybind11::arg("offset"));
  m.def("dot_interact_fwd_packed", &dot_interact_fwd_packed,
        "pairwise-dot interaction on (bottom, packed, perm) (MFMA, gfx950)");
  m.def("dot_interact_bwd_packed", &dot_interact_bwd_packed,
        "packed interaction backward -> (gbottom, gpacked) (MFMA, gfx950)");
  m.def("dot_interact_fwd", &dot_interact_fwd,
        "fused DLRM pairwise-dot interaction forward (MFMA bf16, gfx950)");
  m.def("dot_interact_bwd", &dot_interact_bwd,
        "fused DLRM pairwise-dot interaction backward (MFMA bf16, gfx950)");
  m.def("dot_interact_narrow_fwd", &dot_interact_narrow_fwd,
        "interaction forward, D in {8, 16, 24}, F <= 32 (MFMA bf16, gfx950)");
  m.def("dot_interact_narrow_bwd", &dot_interact_narrow_bwd,
        "interaction backward, D in {8, 16, 24}, F <= 32 (MFMA bf16, gfx950)");
  m.def("dot_interact_narrow_fwd_packed", &dot_interact_narrow_fwd_packed,
        "narrow interaction on (bottom, packed, perm) (MFMA, gfx950)");
  m.def("dot_interact_narrow_bwd_packed", &dot_interact_narrow_bwd_packed,
        "narrow packed interaction backward -> (gbottom, gpacked) (gfx950)");
  m.def("dot_interact_f32_fwd", &dot_interact_f32_fwd,
        "interaction forward on fp32, F <= 32, D % 8 == 0 (MFMA f32, gfx950)");
  m.def("dot_interact_f32_bwd", &dot_interact_f32_bwd,
        "interaction backward on fp32, F <= 32, D % 8 == 0 (MFMA f32, gfx950)");
  m.def("dot_interact_f32_fwd_packed", &dot_interact_f32_fwd_packed,
        "fp32 interaction on (bottom, packed, perm) (MFMA f32, gfx950)");
  m.def("dot_interact_f32_bwd_packed", &dot_interact_f32_bwd_packed,
        "fp32 packed interaction backward -> (gbottom, gpacked) (gfx950)");
  m.def("relu_bwd_bias_grad", &relu_bwd_bias_grad,
        "ReLU backward + bias gradient in one pass -> (grad_in, bias_grad) "
        "(gfx950)");
  m.def("cross_bwd", &cross_bwd,
        "low-rank cross layer backward: gu = G * x0, its column sum, and "
        "acc (+)= G * u in place, one pass -> (gu, gb) (gfx950)",
        pybind11::arg("G"), pybind11::arg("x0"), pybind11::arg("u"),
        pybind11::arg("acc"), pybind11::arg("init"));
  m.def("cross_concat_fwd", &cross_concat_fwd,
        "x0 = [bottom | packed rows in perm order] (gfx950)",
        pybind11::arg("bottom"), pybind11::arg("packed"),
        pybind11::arg("perm"), pybind11::arg("sample_major"));
  m.def("cross_concat_bwd", &cross_concat_bwd,
        "gradient of x0 -> (gbottom, gpacked) (gfx950)",
        pybind11::arg("gx0"), pybind11::arg("perm"),
        pybind11::arg("sample_major"));
  m.def("cross_bwd_f32", &cross_bwd_f32,
        "fp32 low-rank cross layer backward: gu = G * x0, its column sum, "
        "and acc (+)= G * u in place, one pass -> (gu, gb) (gfx950)",
        pybind11::arg("G"), pybind11::arg("x0"), pybind11::arg("u"),
        pybind11::arg("acc"), pybind11::arg("init"));
  m.def("cross_concat_f32_fwd", &cross_concat_f32_fwd,
        "fp32 x0 = [bottom | packed rows in perm order] (gfx950)",
        pybind11::arg("bottom"), pybind11::arg("packed"),
        pybind11::arg("perm"), pybind11::arg("sample_major"));
  m.def("cross_concat_f32_bwd", &cross_concat_f32_bwd,
        "fp32 gradient of x0 -> (gbottom, gpacked) (gfx950)",
        pybind11::arg("gx0"), pybind11::arg("perm"),
        pybind11::arg("sample_major"));
  m.def("concat_pool_fwd", &concat_pool_fwd,
        "[average pool of the concatenated inputs | numerical] (gfx950)",
        pybind11::arg("inputs"), pybind11::arg("numerical"),
        pybind11::arg("stride"), pybind11::arg("out_bf16"));
  m.def("concat_pool_bwd", &concat_pool_bwd,
        "gradient of concat_pool_fwd's output -> the inputs' gradients "
        "(gfx950)",
        pybind11::arg("gout"), pybind11::arg("widths"),
        pybind11::arg("stride"), pybind11::arg("num_numerical"),
        pybind11::arg("in_bf16"));
  m.def("wgrad_splitk", &wgrad_splitk,
        "Linear weight gradient bf16(g^T x), split-K (MFMA bf16, gfx950)",
        pybind11::arg("g"), pybind11::arg("x"), pybind11::arg("splitk") = 0,
        pybind11::arg("tile") = -1);
  m.def("wgrad_splitk_plan", &wgrad_splitk_plan_py,
        "(use, splitk, tile geometry) for g [K, M], x [K, N]");
  m.def("wgrad_gemv", &wgrad_gemv,
        "Linear(N, 1) weight and bias gradient -> (gw [1, N], gb [1]) (gfx950)",
        pybind11::arg("g"), pybind11::arg("x"));
  m.def("wgrad_gemv_plan", &wgrad_gemv_plan_py,
        "(use, row chunks) for g [K, 1], x [K, N]");
  m.def("relu_bwd_bias_grad_f32", &relu_bwd_bias_grad_f32,
        "fp32 ReLU backward + bias gradient in one pass -> (grad_in, "
        "bias_grad) (gfx950)");
  m.def("wgrad_splitk_f32", &wgrad_splitk_f32,
        "fp32 Linear weight gradient g^T x, split-K (MFMA f32, gfx950)",
        pybind11::arg("g"), pybind11::arg("x"), pybind11::arg("splitk") = 0,
        pybind11::arg("tile") = -1);
  m.def("wgrad_splitk_f32_plan", &wgrad_splitk_f32_plan_py,
        "(use, splitk, tile geometry) for fp32 g [K, M], x [K, N]");
  m.def("wgrad_gemv_f32", &wgrad_gemv_f32,
        "fp32 Linear(N, 1) weight and bias gradient -> (gw [1, N], gb [1]) "
        "(gfx950)",
        pybind11::arg("g"), pybind11::arg("x"));
  m.def("wgrad_gemv_f32_plan", &wgrad_gemv_f32_plan_py,
        "(use, row chunks) for fp32 g [K, 1], x [K, N]");
}
