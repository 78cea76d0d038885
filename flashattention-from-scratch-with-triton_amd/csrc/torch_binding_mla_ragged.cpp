// Host-side binding of fa_fwd_kvcache_mla_ragged (include_mla_ragged/mi355fa_ragged_mla.h) for PyTorch-ROCm: MLA decoding over a
// paged latent cache with packed variable-length queries, for mla_ragged_kvcache.py.  One module, _mi355fa_mla_ragged_torch.so,
// beside _mi355fa_mla_torch.so, whose one export is a recorded surface.  It does what the other decode bindings do
// (torch_binding_decode.h says what) and takes from there the helpers whose text is the same; its geometry -- packed q at 576,
// a 3-d pool of one latent head, `out` at 512, LSE [H, total_q] -- and the order of its checks are its own.  The checks that need
// no device come first, so that a malformed call is refused the same way on any machine.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include_mla_ragged/mi355fa_ragged_mla.h"
#include "torch_binding_decode.h"

namespace {

std::string num(int64_t v) { return std::to_string((long long)v); }

// softmax_scale <= 0: 576 ** -0.5.  The Python wrapper has checked what it can name better (types, grad).
std::tuple<Tensor, Tensor> kvcache_mla_ragged_forward(const Tensor& Q, const Tensor& KV, const Tensor& cu, const Tensor& seqlens,
                                                      const Tensor& table, const OptTensor& kv_new, bool is_causal,
                                                      double softmax_scale, const OptTensor& out) {
  FA_ASSERT(Q.dim() == 3, "packed q must be [total_q, H, 576] (got " + num(Q.dim()) + " dims)");
  FA_ASSERT(Q.size(2) == MI355FA_MLA_D,
            "packed q's last dim must be 576: 512 latent dims, then 64 RoPE dims (got " + num(Q.size(2)) + ")");
  FA_ASSERT(KV.dim() == 3, "kv_cache must be [num_pages, page_size, 576]: one latent head, as flash_attention_mla_kvcache takes it (got " +
                               num(KV.dim()) + " dims)");
  FA_ASSERT(KV.size(2) == MI355FA_MLA_D, "kv_cache's last dim must be 576, as packed q's (got " + num(KV.size(2)) + ")");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16,
            "packed q's dtype must be float16 or bfloat16 (flash_attention_mla_kvcache_ragged)");
  FA_ASSERT(KV.scalar_type() == Q.scalar_type(), "kv_cache must have packed q's dtype");
  FA_ASSERT(Q.size(0) >= 1 && Q.size(1) >= 1 && KV.size(0) >= 1, "packed q and kv_cache must not be empty");
  FA_ASSERT(KV.size(1) >= 32 && KV.size(1) % 32 == 0,
            "the page size of the latent pool (kv_cache.shape[1] = " + num(KV.size(1)) + ") must be a positive multiple of 32");
  check_cu_seqlens(cu);
  const int64_t Tq = Q.size(0), H = Q.size(1), B = cu.numel() - 1;
  check_seqlens(seqlens, B, true);
  check_block_table(table, B);
  FA_ASSERT(KV.stride(2) == 1 && KV.stride(1) >= MI355FA_MLA_D && KV.stride(1) % 8 == 0 &&
                (KV.size(0) == 1 || (KV.stride(0) >= 0 && KV.stride(0) % 8 == 0)),
            "the latent pool must be addressable in place: unit stride along the 576 dims, 16-byte aligned rows (a row stride that "
            "is a multiple of 8 elements, got " + num(KV.stride(1)) + ") and a page stride that is a multiple of 8 elements");
  if (kv_new.has_value()) {
    FA_ASSERT(kv_new->dim() == 2 && kv_new->size(0) == Tq && kv_new->size(1) == MI355FA_MLA_D,
              "kv_new must be [total_q, 576]: one cached row per packed query row");
    FA_ASSERT(kv_new->scalar_type() == Q.scalar_type() && !kv_new->requires_grad(),
              "kv_new must have packed q's dtype and must not require grad");
  }
  if (out.has_value()) {
    FA_ASSERT(out->dim() == 3 && out->size(0) == Tq && out->size(1) == H && out->size(2) == MI355FA_MLA_DV &&
                  out->scalar_type() == Q.scalar_type(),
              "out must be [total_q, H, 512] in packed q's dtype");
    FA_ASSERT(out->stride(2) == 1 && (Tq == 1 || (out->stride(0) >= MI355FA_MLA_DV && out->stride(0) % 8 == 0 && out->stride(0) < (1ll << 30))) &&
                  (H == 1 || (out->stride(1) >= MI355FA_MLA_DV && out->stride(1) % 8 == 0 && out->stride(1) < (1ll << 30))) &&
                  !out->requires_grad(),
              "out must be addressable in place (unit stride along the 512 dims, row and head strides that are multiples of 8 "
              "elements, at least 512 and below 2^30) and must not require grad");
  }
  FA_ASSERT(!Q.requires_grad() && !KV.requires_grad(),
            "flash_attention_mla_kvcache_ragged has no backward: q and kv_cache must not require grad");
  FA_ASSERT(Q.is_cuda() && KV.is_cuda() && cu.is_cuda() && seqlens.is_cuda() && table.is_cuda(),
            "packed q, kv_cache, cu_seqlens_q, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(KV.device() == Q.device() && cu.device() == Q.device() && seqlens.device() == Q.device() && table.device() == Q.device() &&
                (!kv_new.has_value() || kv_new->device() == Q.device()) && (!out.has_value() || out->device() == Q.device()),
            "all tensors must be on packed q's device");
  FA_ASSERT(reinterpret_cast<uintptr_t>(KV.data_ptr()) % 16 == 0 && (!out.has_value() || reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0),
            "the latent pool and out must be 16-byte aligned");
  FA_ASSERT(KV.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX && B <= INT32_MAX && H <= INT32_MAX && Tq <= INT32_MAX,
            "too many pages, sequences, heads or packed rows");
  // q as the kernels read it: in place through its row and head strides when they can, a contiguous copy otherwise
  const Tensor Qp = packed_ok(Q, false) ? Q : Q.clone(at::MemoryFormat::Contiguous);
  Tensor Kn;
  if (kv_new.has_value()) Kn = contiguous16(*kv_new);
  const int page = (int)KV.size(1), num_pages = (int)KV.size(0), max_pages = (int)table.size(1);
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)MI355FA_MLA_D));
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out.has_value() ? *out : torch::empty({Tq, H, MI355FA_MLA_DV}, Q.options().memory_format(at::MemoryFormat::Contiguous));
  Tensor LSE = torch::empty({H, Tq}, Q.options().dtype(at::kFloat));
  const long long ws_bytes = fa_fwd_kvcache_mla_ragged_workspace_bytes((int)Tq, (int)B, (int)H, max_pages, page);
  Tensor ws = workspace(ws_bytes, "fa_fwd_kvcache_mla_ragged", Q);
  long long q3[3], o3[3];   // packed_strides: {ignored, head, row}; the call takes {row, head}
  packed_strides(Qp, q3);
  packed_strides(O, o3);
  const long long qs[2] = {q3[2], q3[1]}, os[2] = {o3[2], o3[1]};
  const long long ks[2] = {KV.size(0) > 1 ? KV.stride(0) : KV.size(1) * KV.stride(1), KV.stride(1)};
  check_rc(fa_fwd_kvcache_mla_ragged(Qp.data_ptr(), KV.data_ptr(), Kn.defined() ? Kn.data_ptr() : nullptr, (const int*)cu.data_ptr(),
                                     (const int*)seqlens.data_ptr(), (const int*)table.data_ptr(), O.data_ptr(),
                                     (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)Tq, (int)B, (int)H, num_pages, page,
                                     max_pages, table_stride_of(table, B), Kn.defined() ? 1 : 0, dtype_of(Q), scale,
                                     is_causal ? 1 : 0, qs, ks, os, current_stream(Q)),
           "fa_fwd_kvcache_mla_ragged");
  return {O, LSE};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_mla_ragged (libmi355fa.so): MLA decoding attention over a paged latent cache "
            "with packed variable-length queries";
  m.def("kvcache_mla_ragged_forward", &kvcache_mla_ragged_forward, pybind11::arg("q"), pybind11::arg("kv_cache"),
        pybind11::arg("cu_seqlens_q"), pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("kv_new"),
        pybind11::arg("is_causal"), pybind11::arg("softmax_scale"), pybind11::arg("out"),
        "O, LSE = attention of packed q over the latent rows block_table names, after appending kv_new (None: no append)");
}
