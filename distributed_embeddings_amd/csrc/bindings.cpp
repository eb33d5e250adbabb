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

// Lazy Adam's moments: fp32 [2, vocab, width], m first, on the weight's
// device; both betas in [0, 1).
static void check_adam_state(const torch::Tensor& state,
                             const torch::Tensor& weight, double beta1,
                             double beta2) {
  CHECK_CUDA(state); CHECK_CONTIG(state);
  TORCH_CHECK(state.dtype() == torch::kFloat32, "adam state must be fp32");
  TORCH_CHECK(state.dim() == 3 && state.size(0) == 2 &&
              state.size(1) == weight.size(0) &&
              state.size(2) == weight.size(1),
              "adam state shape mismatch: expected [2, vocab, width], got ",
              state.sizes(), " for weight ", weight.sizes());
  TORCH_CHECK(state.device() == weight.device(),
              "adam state must be on the weight's device");
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
              "adam betas must lie in [0, 1), got (", beta1, ", ", beta2, ")");
}

// adam_step > 0 selects lazy Adam at step t = adam_step (the host counts on
// this path): state is [2, vocab, width] and adagrad has to be false.
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
  if (adam) check_adam_state(state, weight, beta1, beta2);
  const int64_t n = ids.numel();
  if (n == 0) return;
  float* state_ptr = nullptr;
  bool rowwise = false;
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

void csr_fused_optimizer_apply(torch::Tensor weight, torch::Tensor state,
                               torch::Tensor values, torch::Tensor row_splits,
                               torch::Tensor grad_out, torch::Tensor lr,
                               bool mean, bool adagrad, double eps,
                               std::optional<torch::Tensor> per_id_w,
                               std::optional<torch::Tensor> sr,
                               std::optional<torch::Tensor> adam_step,
                               double beta1, double beta2,
                               bool deterministic) {
  // adam_step (int64 [1] on the device) selects lazy Adam: state is
  // [2, vocab, width], adagrad has to be false, and an apply that launches
  // adds 1 to the step on the device.
  // All-device sorted pipeline (no host sync; hipGraph-capturable):
  // sort (id, pos) -> permute row-ids -> head-flag unique -> segment pad ->
  // one direct update per unique row (long segments chunked with one atomic
  // per partial, or, deterministic, one slab row per partial and a
  // fixed-order combine).  Replaces both torch sparse grads and the naive
  // atomic scatter (hot-row same-address chains).
  CHECK_CUDA(weight); CHECK_CUDA(values); CHECK_CUDA(row_splits);
  CHECK_CUDA(grad_out); CHECK_CUDA(lr);
  CHECK_CONTIG(weight); CHECK_CONTIG(values); CHECK_CONTIG(row_splits);
  CHECK_CONTIG(grad_out);
  TORCH_CHECK(weight.dtype() == torch::kFloat32 ||
              weight.dtype() == torch::kBFloat16);
  TORCH_CHECK((grad_out.dtype() == torch::kFloat32 ||
               grad_out.dtype() == torch::kBFloat16) &&
              lr.dtype() == torch::kFloat32);
  const float* user_w = per_id_w_ptr(per_id_w, values);
  int64_t* sr_p = sr_ptr(sr, weight);
  const bool wbf16 = weight.dtype() == torch::kBFloat16;
  const int64_t num_rows = row_splits.numel() - 1;
  const int64_t nnz = values.numel();
  const int64_t vocab = weight.size(0);
  const int width = (int)weight.size(1);
  const bool adam = adam_step.has_value();
  if (adam) {
    TORCH_CHECK(!adagrad, "adam_step and adagrad exclude each other");
    check_adam_state(state, weight, beta1, beta2);
    const torch::Tensor& t = *adam_step;
    CHECK_CUDA(t); CHECK_CONTIG(t);
    TORCH_CHECK(t.dtype() == torch::kInt64 && t.dim() == 1 && t.numel() == 1,
                "adam_step must be an int64 [1] tensor");
    TORCH_CHECK(t.device() == weight.device(),
                "adam_step must be on the weight's device");
  }
  if (num_rows <= 0 || nnz <= 0) return;
  auto stream = current_stream();
  auto i64 = values.options();
  auto i32 = values.options().dtype(torch::kInt32);
  auto f32 = grad_out.options().dtype(torch::kFloat32);

  auto ss = build_sorted_segments(values, row_splits, vocab, mean, user_w,
                                  stream);
  launch_pad_seg_offsets(ss.seg.data_ptr<int64_t>(), nnz,
                         ss.num_unique.data_ptr<int32_t>(),
                         ss.bounds.data_ptr<int64_t>(), stream);
  auto long_rows = torch::empty({nnz}, i64);
  auto long_count = torch::empty({1}, i32);
  auto work_items = torch::empty({nnz / 64 + 64}, i64);
  auto n_work = torch::empty({1}, i32);
  float* state_ptr = nullptr;
  torch::Tensor scratch;
  float* scratch_ptr = nullptr;
  int64_t scratch_rows = 0;
  bool rowwise = false;
  if (adagrad) {
    rowwise = check_adagrad_state(state, weight);
    state_ptr = state.data_ptr<float>();
  }
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
                                 scratch_rows, adagrad, rowwise, sr_p,
                                 adam ? &cfg : nullptr, det.slab_ptr(),
                                 det.work_base_ptr(), stream);
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
std::vector<torch::Tensor> cross_bwd(torch::Tensor G, torch::Tensor x0,
                                     torch::Tensor u, torch::Tensor acc,
                                     bool init) {
  CHECK_CUDA(G); CHECK_CUDA(x0); CHECK_CUDA(u); CHECK_CUDA(acc);
  CHECK_CONTIG(G); CHECK_CONTIG(x0); CHECK_CONTIG(u); CHECK_CONTIG(acc);
  TORCH_CHECK(G.dtype() == torch::kBFloat16 &&
              x0.dtype() == torch::kBFloat16 &&
              u.dtype() == torch::kBFloat16 &&
              acc.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(G.dim() == 2 && G.sizes() == x0.sizes() &&
              G.sizes() == u.sizes() && G.sizes() == acc.sizes(),
              "G, x0, u and acc must be [B, N]");
  TORCH_CHECK(G.device() == x0.device() && G.device() == u.device() &&
              G.device() == acc.device(), "operands must share a device");
  const int64_t B = G.size(0);
  const int64_t N = G.size(1);
  TORCH_CHECK(N % 8 == 0 && N < (int64_t(1) << 31), "N % 8 == 0 required");
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
  launch_cross_bwd(G.data_ptr(), x0.data_ptr(), u.data_ptr(), acc.data_ptr(),
                   init, gu.data_ptr(), slab.data_ptr<float>(), gb.data_ptr(),
                   B, (int)N, rows_per_chunk, num_chunks, current_stream());
  return {gu, gb};
}

// Shapes of the cross interaction's input assembly: bottom [B, D], packed
// [P, B, D] (feature-major) or [B, P, D] (sample-major), x0 [B, (P+1)*D].
static void check_cross_concat_shape(int64_t B, int64_t P, int64_t D) {
  TORCH_CHECK(P >= 1 && D >= 8 && D % 8 == 0,
              "P >= 1 and D % 8 == 0 required (got P=", P, ", D=", D, ")");
  // a block walks 16 rows of x0 with 32-bit indices
  TORCH_CHECK((P + 1) * D < (int64_t(1) << 27), "row of x0 too wide");
  TORCH_CHECK(B >= 0, "negative batch");
}

torch::Tensor cross_concat_fwd(torch::Tensor bottom, torch::Tensor packed,
                               torch::Tensor perm, bool sample_major) {
  CHECK_CUDA(bottom); CHECK_CUDA(packed); CHECK_CUDA(perm);
  CHECK_CONTIG(bottom); CHECK_CONTIG(packed); CHECK_CONTIG(perm);
  TORCH_CHECK(bottom.dtype() == torch::kBFloat16 &&
              packed.dtype() == torch::kBFloat16, "bf16 required");
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
  check_cross_concat_shape(B, P, D);
  CHECK_ALIGN16(bottom); CHECK_ALIGN16(packed);
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto x0 = torch::empty({B, (P + 1) * D}, bottom.options());
  launch_cross_concat_fwd(bottom.data_ptr(), packed.data_ptr(),
                          perm.data_ptr<int>(), x0.data_ptr(), B, (int)P,
                          (int)D, sb, sp, current_stream());
  return x0;
}

// (gbottom [B, D], gpacked in packed's layout) from gx0 [B, (P+1)*D]; perm
// has to be a permutation of [0, P).
std::vector<torch::Tensor> cross_concat_bwd(torch::Tensor gx0,
                                            torch::Tensor perm,
                                            bool sample_major) {
  CHECK_CUDA(gx0); CHECK_CUDA(perm);
  CHECK_CONTIG(gx0); CHECK_CONTIG(perm);
  TORCH_CHECK(gx0.dtype() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(perm.dtype() == torch::kInt32, "perm must be int32");
  TORCH_CHECK(gx0.dim() == 2 && perm.dim() == 1 && perm.numel() >= 1,
              "gx0 [B, (P+1)*D], perm [P]");
  TORCH_CHECK(gx0.device() == perm.device(), "operands must share a device");
  const int64_t B = gx0.size(0);
  const int64_t P = perm.numel();
  TORCH_CHECK(gx0.size(1) % (P + 1) == 0,
              "gx0 width must be a multiple of P + 1");
  const int64_t D = gx0.size(1) / (P + 1);
  check_cross_concat_shape(B, P, D);
  CHECK_ALIGN16(gx0);
  const int64_t sb = sample_major ? P : 1;
  const int64_t sp = sample_major ? 1 : B;
  auto gbottom = torch::empty({B, D}, gx0.options());
  auto gpacked = sample_major ? torch::empty({B, P, D}, gx0.options())
                              : torch::empty({P, B, D}, gx0.options());
  launch_cross_concat_bwd(gx0.data_ptr(), perm.data_ptr<int>(),
                          gbottom.data_ptr(), gpacked.data_ptr(), B, (int)P,
                          (int)D, sb, sp, current_stream());
  return {gbottom, gpacked};
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
  m.def("wgrad_splitk", &wgrad_splitk,
        "Linear weight gradient bf16(g^T x), split-K (MFMA bf16, gfx950)",
        pybind11::arg("g"), pybind11::arg("x"), pybind11::arg("splitk") = 0,
        pybind11::arg("tile") = -1);
  m.def("wgrad_splitk_plan", &wgrad_splitk_plan_py,
        "(use, splitk, tile geometry) for g [K, M], x [K, N]");
}
