// Host-side binding of fa_fwd_kvcache_mla (include_mla/mi355fa_kvcache_mla.h) for PyTorch-ROCm: MLA decoding over a paged
// latent cache, for mla_kvcache.py.  One module, _mi355fa_mla_torch.so, beside the other decode bindings.  It does what they do
// (torch_binding_decode.h says what) and takes from there the few lines whose text is the same; its geometry -- one latent head,
// a 3-d pool, `out` at 512 -- and the order of its checks are its own.  The checks that need no device come first, so that a
// malformed call is refused the same way on any machine.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include_mla/mi355fa_kvcache_mla.h"
#include "torch_binding_decode.h"

namespace {

std::string num(int64_t v) { return std::to_string((long long)v); }

// Can the kernels address q [B, H, S_q, 576] / out [B, H, S_q, 512] in place?  (an output's rows are distinct memory)
bool rows_ok(const Tensor& t, bool output) {
  if (t.stride(3) != 1 || (t.size(2) > 1 && t.stride(2) < t.size(3))) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % 8 != 0 || (output && t.stride(i) == 0))) return false;
  return true;
}

// softmax_scale <= 0: 576 ** -0.5.  The Python wrapper has checked what it can name better (types, grad).
std::tuple<Tensor, Tensor> kvcache_mla_forward(const Tensor& Q, const Tensor& KV, const Tensor& seqlens, const Tensor& table,
                                               const OptTensor& kv_new, bool is_causal, double softmax_scale, const OptTensor& out) {
  FA_ASSERT(Q.dim() == 4, "q must be [B, H, S_q, 576] (got " + num(Q.dim()) + " dims)");
  FA_ASSERT(Q.size(3) == MI355FA_MLA_D,
            "q's last dim must be 576: 512 latent dims, then 64 RoPE dims (got " + num(Q.size(3)) + ")");
  FA_ASSERT(KV.dim() == 3, "kv_cache must be [num_pages, page_size, 576]: one latent head (got " + num(KV.dim()) + " dims)");
  FA_ASSERT(KV.size(2) == MI355FA_MLA_D, "kv_cache's last dim must be 576 (got " + num(KV.size(2)) + ")");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
  FA_ASSERT(KV.scalar_type() == Q.scalar_type(), "kv_cache must have q's dtype");
  FA_ASSERT(Q.size(0) >= 1 && Q.size(1) >= 1 && Q.size(2) >= 1 && KV.size(0) >= 1, "q and kv_cache must not be empty");
  FA_ASSERT(KV.size(1) >= 32 && KV.size(1) % 32 == 0,
            "the page size (kv_cache.shape[1] = " + num(KV.size(1)) + ") must be a positive multiple of 32");
  const int64_t B = Q.size(0), H = Q.size(1), Sq = Q.size(2);
  check_seqlens(seqlens, B, false);
  check_block_table(table, B);
  FA_ASSERT(KV.stride(2) == 1 && KV.stride(1) >= MI355FA_MLA_D && KV.stride(1) % 8 == 0 &&
                (KV.size(0) == 1 || (KV.stride(0) >= 0 && KV.stride(0) % 8 == 0)),
            "kv_cache must be addressable in place: unit stride along the 576 dims, 16-byte aligned rows (a row stride that is a "
            "multiple of 8 elements, got " + num(KV.stride(1)) + ") and a page stride that is a multiple of 8 elements");
  if (kv_new.has_value()) {
    FA_ASSERT(kv_new->dim() == 3 && kv_new->size(0) == B && kv_new->size(1) == Sq && kv_new->size(2) == MI355FA_MLA_D,
              "kv_new must be [B, S_q, 576]: one cached row per query row");
    FA_ASSERT(kv_new->scalar_type() == Q.scalar_type() && !kv_new->requires_grad(),
              "kv_new must have q's dtype and must not require grad");
  }
  if (out.has_value()) {
    FA_ASSERT(out->dim() == 4 && out->size(0) == B && out->size(1) == H && out->size(2) == Sq && out->size(3) == MI355FA_MLA_DV &&
                  out->scalar_type() == Q.scalar_type(),
              "out must be [B, H, S_q, 512] in q's dtype");
    FA_ASSERT(rows_ok(*out, true) && !out->requires_grad(),
              "out must be addressable in place (unit stride along the 512 dims, strides that are non-zero multiples of 8 "
              "elements) and must not require grad");
  }
  FA_ASSERT(!Q.requires_grad() && !KV.requires_grad(),
            "flash_attention_mla_kvcache has no backward: q and kv_cache must not require grad");
  FA_ASSERT(Q.is_cuda() && KV.is_cuda() && seqlens.is_cuda() && table.is_cuda(),
            "q, kv_cache, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(KV.device() == Q.device() && seqlens.device() == Q.device() && table.device() == Q.device() &&
                (!kv_new.has_value() || kv_new->device() == Q.device()) && (!out.has_value() || out->device() == Q.device()),
            "all tensors must be on q's device");
  FA_ASSERT(reinterpret_cast<uintptr_t>(KV.data_ptr()) % 16 == 0 && (!out.has_value() || reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0),
            "kv_cache and out must be 16-byte aligned");
  FA_ASSERT(KV.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX && B <= INT32_MAX && H <= INT32_MAX && Sq <= INT32_MAX,
            "too many pages, sequences, heads or rows");
  // q as the kernels read it: in place through its strides when they can, a contiguous copy otherwise
  const Tensor Qp = (reinterpret_cast<uintptr_t>(Q.data_ptr()) % 16 == 0 && rows_ok(Q, false)) ? Q : Q.clone(at::MemoryFormat::Contiguous);
  Tensor Kn;
  int S_new = 0;
  if (kv_new.has_value()) {
    Kn = contiguous16(*kv_new);
    S_new = (int)Sq;
  }
  const int page = (int)KV.size(1), num_pages = (int)KV.size(0), max_pages = (int)table.size(1);
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)MI355FA_MLA_D));
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out.has_value() ? *out : torch::empty({B, H, Sq, MI355FA_MLA_DV}, Q.options().memory_format(at::MemoryFormat::Contiguous));
  Tensor LSE = torch::empty({B, H, Sq}, Q.options().dtype(at::kFloat));
  const long long ws_bytes = fa_fwd_kvcache_mla_workspace_bytes((int)B, (int)H, (int)Sq, max_pages, page, S_new);
  Tensor ws = workspace(ws_bytes, "fa_fwd_kvcache_mla", Q);
  long long qs[3], os[3];
  strides3(Qp, qs);
  strides3(O, os);
  const long long ks[2] = {KV.size(0) > 1 ? KV.stride(0) : KV.size(1) * KV.stride(1), KV.stride(1)};
  check_rc(fa_fwd_kvcache_mla(Qp.data_ptr(), KV.data_ptr(), Kn.defined() ? Kn.data_ptr() : nullptr, (const int*)seqlens.data_ptr(),
                              (const int*)table.data_ptr(), O.data_ptr(), (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)B,
                              (int)H, (int)Sq, num_pages, page, max_pages, table_stride_of(table, B), S_new, dtype_of(Q), scale,
                              is_causal ? 1 : 0, Qp.is_contiguous() ? nullptr : qs, ks, O.is_contiguous() ? nullptr : os,
                              current_stream(Q)),
           "fa_fwd_kvcache_mla");
  return {O, LSE};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_mla (libmi355fa.so): MLA decoding attention over a paged latent cache";
  m.def("kvcache_mla_forward", &kvcache_mla_forward, pybind11::arg("q"), pybind11::arg("kv_cache"), pybind11::arg("cache_seqlens"),
        pybind11::arg("block_table"), pybind11::arg("kv_new"), pybind11::arg("is_causal"), pybind11::arg("softmax_scale"),
        pybind11::arg("out"),
        "O, LSE = attention of q over the latent rows block_table names, after appending kv_new (None: no append)");
}
