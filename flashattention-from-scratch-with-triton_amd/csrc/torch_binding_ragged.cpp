// Host-side binding of fa_fwd_kvcache_ragged (include/mi355fa_ragged.h) for PyTorch-ROCm: decoding attention over a paged KV
// cache with packed variable-length queries, for ragged_kvcache.py.  A module of its own, _mi355fa_ragged_torch.so, beside
// _mi355fa_paged_torch.so (torch_binding_paged.cpp), which it follows: O (unless the caller gives one), LSE and the
// workspace come from the caching allocator, q / out and the pools are addressed in place through their strides, the launch
// goes to the current stream, and nothing here synchronises or reads cu_seqlens_q, cache_seqlens or block_table, so a step
// can be captured in a graph.  Inference only: no autograd.
//
// Built by csrc/Makefile with g++ (host code only).
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/extension.h>

#include <cmath>
#include <string>
#include <tuple>

#include "../../include/mi355fa_ragged.h"

namespace {

using torch::Tensor;

// bad arguments raise AssertionError, as everywhere in the package
[[noreturn]] void assertion(const std::string& msg) {
  PyErr_SetString(PyExc_AssertionError, msg.c_str());
  throw pybind11::error_already_set();
}
#define FA_ASSERT(cond, msg) \
  do {                       \
    if (!(cond)) assertion(msg); \
  } while (0)

void check_rc(long long rc, const char* what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + " failed (code " + std::to_string(rc) + "): " + fa_last_error());
}

// the pool [num_pages, H_kv, page_size, D] in place: torch_binding_paged.cpp pool_ok / strides3
bool pool_ok(const Tensor& t, int64_t esz) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 || t.stride(3) != 1 || t.stride(2) < t.size(3)) return false;
  if ((t.size(2) - 1) * t.stride(2) * esz + t.size(3) * esz > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || (t.stride(i) * esz) % 16 != 0)) return false;
  return true;
}
void strides3(const Tensor& t, long long* v) {
  v[0] = t.size(0) > 1 ? t.stride(0) : t.size(1) * t.size(2) * t.size(3);
  v[1] = t.size(1) > 1 ? t.stride(1) : 0;
  v[2] = t.size(2) > 1 ? t.stride(2) : t.size(3);
}

// Can the kernels address the packed [total_q, H, D] tensor in place?  A 16-byte aligned base, D innermost, head and row
// strides that are multiples of 8 elements (16-byte rows), rows at least D apart; an output's heads and rows are distinct
// memory.  A size-1 dimension may carry any stride: packed_strides gives it a harmless one.
bool packed_ok(const Tensor& t, bool output) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 || t.stride(2) != 1) return false;
  if (t.size(0) > 1 && (t.stride(0) < t.size(2) || t.stride(0) % 8 != 0 || t.stride(0) >= (1ll << 30))) return false;
  if (t.size(1) > 1 && (t.stride(1) < 0 || t.stride(1) % 8 != 0 || t.stride(1) >= (1ll << 30))) return false;
  if (output && t.size(1) > 1 && t.stride(1) < t.size(2)) return false;
  return true;
}
void packed_strides(const Tensor& t, long long* v) {   // {ignored, head, row}
  v[0] = 0;
  v[1] = t.size(1) > 1 ? t.stride(1) : t.size(2);
  v[2] = t.size(0) > 1 ? t.stride(0) : t.size(1) * t.size(2);
}

const float* fptr(const c10::optional<Tensor>& t) { return t.has_value() ? (const float*)t->data_ptr() : nullptr; }

// an fp32 device vector of the call: (n,) or, when B > 0, (B, n)
void check_vec(const c10::optional<Tensor>& t, const char* what, int64_t B, int64_t n, const c10::Device& dev) {
  if (!t.has_value()) return;
  const std::string w(what);
  FA_ASSERT(t->scalar_type() == at::kFloat, w + " must be float32");
  FA_ASSERT((t->dim() == 1 && t->size(0) == n) || (B > 0 && t->dim() == 2 && t->size(0) == B && t->size(1) == n),
            w + " has the wrong shape");
  FA_ASSERT(t->is_contiguous() && !t->requires_grad(), w + " must be contiguous and must not require grad");
  FA_ASSERT(t->is_cuda() && t->device() == dev, w + " must be a device tensor on q's device");
}

// softmax_scale <= 0: 1/sqrt(D); softcap <= 0: none.  The Python wrapper has refused the combinations of transforms.
std::tuple<Tensor, Tensor> kvcache_ragged_forward(const Tensor& Q, const Tensor& Kp, const Tensor& Vp, const Tensor& cu,
                                                  const Tensor& seqlens, const Tensor& table,
                                                  const c10::optional<Tensor>& k_new, const c10::optional<Tensor>& v_new,
                                                  int64_t window_left, int64_t window_right, double softmax_scale,
                                                  double softcap, const c10::optional<Tensor>& slopes,
                                                  const c10::optional<Tensor>& sinks, const c10::optional<Tensor>& k_descale,
                                                  const c10::optional<Tensor>& v_descale, const c10::optional<Tensor>& out) {
  FA_ASSERT(Q.dim() == 3 && Kp.dim() == 4 && Vp.dim() == 4, "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D]");
  const bool fp8 = Kp.scalar_type() == at::kFloat8_e4m3fn;
  FA_ASSERT(Kp.sizes() == Vp.sizes() && Kp.scalar_type() == Vp.scalar_type(), "k_cache and v_cache must have the same shape and dtype");
  FA_ASSERT(Q.size(0) >= 1, "q must have at least one row");
  FA_ASSERT(Kp.size(3) == Q.size(2), "the pools must have q's head dim");
  FA_ASSERT(Kp.size(1) >= 1 && Q.size(1) % Kp.size(1) == 0, "q's head count must be a multiple of the pools' (H % H_kv == 0)");
  FA_ASSERT(Kp.size(2) >= 32 && Kp.size(2) % 32 == 0, "the page size (k_cache.shape[2]) must be a positive multiple of 32");
  FA_ASSERT(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  FA_ASSERT(window_left >= -1 && window_right >= -1 && window_left <= INT32_MAX && window_right <= INT32_MAX,
            "window_left / window_right must be >= -1 (-1 = unbounded) and fit in int32");
  FA_ASSERT(Q.is_cuda() && Kp.is_cuda() && Vp.is_cuda() && cu.is_cuda() && seqlens.is_cuda() && table.is_cuda(),
            "q, the pools, cu_seqlens_q, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(Kp.device() == Q.device() && Vp.device() == Q.device() && cu.device() == Q.device() &&
                seqlens.device() == Q.device() && table.device() == Q.device(),
            "all tensors must be on q's device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
  FA_ASSERT(fp8 || Kp.scalar_type() == Q.scalar_type(), "the pools must have q's dtype or be torch.float8_e4m3fn");
  FA_ASSERT(Q.size(2) == 64 || Q.size(2) == 128, "head dim must be 64 or 128");
  FA_ASSERT(cu.scalar_type() == at::kInt && cu.dim() == 1 && cu.numel() >= 2 && cu.is_contiguous(),
            "cu_seqlens_q must be a contiguous int32 vector of B + 1 entries");
  const int64_t B = cu.numel() - 1, Tq = Q.size(0), Hq = Q.size(1), Hk = Kp.size(1);
  FA_ASSERT(seqlens.scalar_type() == at::kInt && seqlens.dim() == 1 && seqlens.numel() == B && seqlens.is_contiguous(),
            "cache_seqlens must be a contiguous int32 vector of B entries (cu_seqlens_q has B + 1)");
  FA_ASSERT(table.scalar_type() == at::kInt && table.dim() == 2 && table.size(0) == B && table.size(1) >= 1 &&
                (table.size(1) == 1 || table.stride(1) == 1) && (B == 1 || table.stride(0) >= table.size(1)),
            "block_table must be an int32 tensor [B, max_pages_per_seq] with unit stride along the pages");
  FA_ASSERT(!Q.requires_grad() && !Kp.requires_grad() && !Vp.requires_grad(),
            "flash_attention_kvcache_ragged has no backward: q, k_cache and v_cache must not require grad");
  check_vec(slopes, "alibi_slopes", B, Hq, Q.device());
  check_vec(sinks, "sinks", 0, Hq, Q.device());
  check_vec(k_descale, "k_descale", B, Hk, Q.device());
  check_vec(v_descale, "v_descale", B, Hk, Q.device());
  const int64_t esz = fp8 ? 1 : 2;
  FA_ASSERT(pool_ok(Kp, esz) && pool_ok(Vp, esz) && (Kp.size(2) == 1 || Kp.stride(2) == Vp.stride(2)),
            "the pools must be addressable in place: 16-byte aligned rows with unit head-dim stride, strides that are multiples "
            "of 16 bytes, one row stride for K and V");
  // one batch stride serves both descale vectors: a (H_kv,) vector beside a (B, H_kv) one is expanded
  Tensor Kd, Vd;
  long long dstride = 0;
  if (k_descale.has_value()) Kd = *k_descale;
  if (v_descale.has_value()) Vd = *v_descale;
  if ((Kd.defined() && Kd.dim() == 2) || (Vd.defined() && Vd.dim() == 2)) {
    dstride = Hk;
    if (Kd.defined() && Kd.dim() == 1) Kd = Kd.expand({B, Hk}).contiguous();
    if (Vd.defined() && Vd.dim() == 1) Vd = Vd.expand({B, Hk}).contiguous();
  }
  Tensor Kn, Vn;
  if (k_new.has_value()) {
    FA_ASSERT(k_new->dim() == 3 && k_new->sizes() == v_new->sizes() && k_new->size(0) == Tq && k_new->size(1) == Hk &&
                  k_new->size(2) == Q.size(2),
              "k_new and v_new must be [total_q, H_kv, D]: one key and one value per query row");
    FA_ASSERT(k_new->device() == Q.device() && v_new->device() == Q.device() && k_new->scalar_type() == Q.scalar_type() &&
                  v_new->scalar_type() == Q.scalar_type() && !k_new->requires_grad() && !v_new->requires_grad(),
              "k_new and v_new must be on q's device with q's dtype and must not require grad");
    auto packed = [](const Tensor& t) {
      return (t.is_contiguous() && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0) ? t : t.clone(at::MemoryFormat::Contiguous);
    };
    Kn = packed(*k_new);
    Vn = packed(*v_new);
  }
  // q as the kernels read it: in place through its head and row strides when they can, a packed copy otherwise
  const Tensor Qp = packed_ok(Q, false) ? Q : Q.clone(at::MemoryFormat::Contiguous);
  const int H = (int)Hq, Hkv = (int)Hk, D = (int)Q.size(2), page = (int)Kp.size(2);
  FA_ASSERT(Kp.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX && Tq <= INT32_MAX && B <= INT32_MAX,
            "too many pages, rows or sequences");
  const int num_pages = (int)Kp.size(0), max_pages = (int)table.size(1);
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)D));
  const int cache_dtype = fp8 ? MI355FA_PAGED_CACHE_FP8_E4M3 : MI355FA_PAGED_CACHE_16BIT;
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O;
  if (out.has_value()) {   // written in place: a result the caller asked for here is never produced in a copy
    FA_ASSERT(out->sizes() == Q.sizes() && out->scalar_type() == Q.scalar_type(), "out must have q's shape and dtype");
    FA_ASSERT(out->is_cuda() && out->device() == Q.device() && !out->requires_grad(),
              "out must be on q's device and must not require grad");
    FA_ASSERT(packed_ok(*out, true),
              "out must be addressable in place: 16-byte aligned rows with unit head-dim stride, head and row strides that are "
              "multiples of 8 elements");
    O = *out;
  } else {
    O = torch::empty(Q.sizes(), Q.options().memory_format(at::MemoryFormat::Contiguous));
  }
  Tensor LSE = torch::empty({Hq, Tq}, Q.options().dtype(at::kFloat));
  const long long ws_bytes = fa_fwd_kvcache_ragged_workspace_bytes((int)Tq, (int)B, H, Hkv, max_pages, page, D, cache_dtype);
  check_rc(ws_bytes, "fa_fwd_kvcache_ragged_workspace_bytes");
  Tensor ws = torch::empty({ws_bytes}, Q.options().dtype(at::kByte));
  long long qs[3], os[3], ks[3], vs[3];
  packed_strides(Qp, qs);
  packed_strides(O, os);
  strides3(Kp, ks);
  strides3(Vp, vs);
  mi355fa_opts opts{};
  opts.size = sizeof(opts);
  opts.q_strides = qs;
  opts.o_strides = os;
  opts.k_strides = ks;
  opts.v_strides = vs;
  mi355fa_paged_mods mods{};
  mods.softcap = softcap > 0.0 ? (float)softcap : 0.f;
  mods.alibi_slopes = fptr(slopes);
  mods.slopes_batch_stride = slopes.has_value() && slopes->dim() == 2 ? (long long)slopes->size(1) : 0;
  mods.sinks = fptr(sinks);
  mods.k_descale = Kd.defined() ? (const float*)Kd.data_ptr() : nullptr;
  mods.v_descale = Vd.defined() ? (const float*)Vd.data_ptr() : nullptr;
  mods.descale_bstride = dstride;
  void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Q.device().index()).stream();
  check_rc(fa_fwd_kvcache_ragged(Qp.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), Kn.defined() ? Kn.data_ptr() : nullptr,
                                 Vn.defined() ? Vn.data_ptr() : nullptr, (const int*)cu.data_ptr(),
                                 (const int*)seqlens.data_ptr(), (const int*)table.data_ptr(), O.data_ptr(),
                                 (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)Tq, (int)B, H, Hkv, num_pages, page,
                                 max_pages, B > 1 ? (long long)table.stride(0) : (long long)max_pages, D,
                                 Q.scalar_type() == at::kBFloat16 ? MI355FA_BF16 : MI355FA_FP16, cache_dtype, scale,
                                 (int)window_left, (int)window_right, &mods, &opts, stream),
           "fa_fwd_kvcache_ragged");
  return {O, LSE};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_ragged (libmi355fa.so): paged-cache decoding with packed variable-length queries";
  m.def("kvcache_ragged_forward", &kvcache_ragged_forward, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("cu_seqlens_q"), pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("k_new"),
        pybind11::arg("v_new"), pybind11::arg("window_left"), pybind11::arg("window_right"), pybind11::arg("softmax_scale"),
        pybind11::arg("softcap"), pybind11::arg("alibi_slopes"), pybind11::arg("sinks"), pybind11::arg("k_descale"),
        pybind11::arg("v_descale"), pybind11::arg("out"),
        "O, LSE = attention of the packed q over the pages block_table names, after appending k_new / v_new (None: no append)");
}
