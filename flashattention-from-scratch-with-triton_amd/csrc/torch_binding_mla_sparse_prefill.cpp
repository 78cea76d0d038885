// Host-side binding of fa_fwd_mla_sparse_prefill (include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h) for PyTorch-ROCm:
// sparse (top-k indexed) MLA prefill over one contiguous latent array, for mla_sparse_prefill.py.  One module,
// _mi355fa_mla_sparse_prefill_torch.so, beside the other decode bindings.  The checks that need no device come first, so that a
// malformed call is refused the same way on any machine.  q goes in through its row and head strides when the kernel can read
// it and as a contiguous copy otherwise; kv, indices and `out` in place, never copied; indices is never read here.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <cmath>
#include <string>
#include <tuple>

#include "../../include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h"
#include "torch_binding_decode.h"

namespace {

std::string num(int64_t v) { return std::to_string((long long)v); }

// softmax_scale <= 0: 576 ** -0.5.  The Python wrapper has checked what it can name better (types, grad).
std::tuple<Tensor, Tensor> mla_sparse_prefill_forward(const Tensor& Q, const Tensor& KV, const Tensor& indices, double softmax_scale,
                                                      const OptTensor& out) {
  FA_ASSERT(Q.dim() == 3 && Q.size(2) == 576, "q must be [M, H, 576]: 512 latent dims, then 64 RoPE dims (got " + num(Q.dim()) + " dims)");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
  const int64_t M = Q.size(0), H = Q.size(1);
  FA_ASSERT(H >= 1 && H <= 1024, "H (q.shape[1]) must be in [1, 1024] (got " + num(H) + ")");
  FA_ASSERT(M <= (1 << 22), "M (q.shape[0]) must be at most 2^22 (got " + num(M) + ")");
  FA_ASSERT(KV.dim() == 2 && KV.size(1) == 576, "kv must be [N, 576]: one latent row per key (got " + num(KV.dim()) + " dims)");
  FA_ASSERT(KV.scalar_type() == Q.scalar_type(), "kv must have q's dtype");
  const int64_t N = KV.size(0);
  FA_ASSERT(N <= INT32_MAX, "N (kv.shape[0]) must be below 2^31 (got " + num(N) + ")");
  FA_ASSERT(indices.scalar_type() == at::kInt && indices.dim() == 2 && indices.size(0) == M && indices.size(1) >= 1 &&
                indices.size(1) <= (1 << 24),
            "indices must be an int32 tensor [M, topk] with 1 <= topk <= 2^24");
  FA_ASSERT((indices.size(1) == 1 || indices.stride(1) == 1) && (M <= 1 || indices.stride(0) >= 0),
            "indices must have unit stride along topk and a non-negative row stride");
  FA_ASSERT(KV.stride(1) == 1 && (N <= 1 || (KV.stride(0) >= 576 && KV.stride(0) % 8 == 0 && KV.stride(0) <= (1 << 24))),
            "kv must be addressable in place: unit stride along the 576 dims and 16-byte aligned rows (a row stride that is a "
            "multiple of 8 elements and at least 576, got " + num(KV.stride(0)) + ")");
  if (out.has_value()) {
    FA_ASSERT(out->dim() == 3 && out->size(0) == M && out->size(1) == H && out->size(2) == 512 && out->scalar_type() == Q.scalar_type(),
              "out must be [M, H, 512] in q's dtype");
    FA_ASSERT(out->stride(2) == 1 && (M <= 1 || (out->stride(0) >= 512 && out->stride(0) % 8 == 0)) &&
                  (H <= 1 || (out->stride(1) >= 512 && out->stride(1) % 8 == 0)) && !out->requires_grad(),
              "out must be addressable in place (unit stride along the 512 dims, row and head strides that are multiples of 8 "
              "elements and at least 512) and must not require grad");
  }
  FA_ASSERT(!Q.requires_grad() && !KV.requires_grad(), "flash_attention_mla_sparse_prefill has no backward: q and kv must not require grad");
  FA_ASSERT(Q.is_cuda() && KV.is_cuda() && indices.is_cuda() && (!out.has_value() || out->is_cuda()),
            "q, kv, indices and out must be device tensors");
  FA_ASSERT(KV.device() == Q.device() && indices.device() == Q.device() && (!out.has_value() || out->device() == Q.device()),
            "all tensors must be on q's device");
  FA_ASSERT((N == 0 || reinterpret_cast<uintptr_t>(KV.data_ptr()) % 16 == 0) &&
                (!out.has_value() || M == 0 || reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0),
            "kv and out must be 16-byte aligned");
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out.has_value() ? *out : torch::empty({M, H, 512}, Q.options().memory_format(at::MemoryFormat::Contiguous));
  Tensor LSE = torch::empty({M, H}, Q.options().dtype(at::kFloat));
  if (M == 0) return {O, LSE};
  const bool in_place = reinterpret_cast<uintptr_t>(Q.data_ptr()) % 16 == 0 && Q.stride(2) == 1 &&
                        (M == 1 || (Q.stride(0) >= 0 && Q.stride(0) % 8 == 0)) && (H == 1 || (Q.stride(1) >= 0 && Q.stride(1) % 8 == 0));
  const Tensor Qp = in_place ? Q : Q.clone(at::MemoryFormat::Contiguous);
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt(576.0));
  const long long qs[2] = {M > 1 ? Qp.stride(0) : 0, H > 1 ? Qp.stride(1) : 0};   // a size-1 dim: a harmless stride
  const long long os[2] = {M > 1 ? O.stride(0) : H * 512, H > 1 ? O.stride(1) : 512};
  check_rc(fa_fwd_mla_sparse_prefill(Qp.data_ptr(), N ? KV.data_ptr() : nullptr, (const int*)indices.data_ptr(), O.data_ptr(),
                                     (float*)LSE.data_ptr(), (int)M, (int)H, (int)N, (int)indices.size(1), dtype_of(Q), scale, qs,
                                     N > 1 ? KV.stride(0) : 576, os, M > 1 ? indices.stride(0) : 0, current_stream(Q)),
           "fa_fwd_mla_sparse_prefill");
  return {O, LSE};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_mla_sparse_prefill (libmi355fa.so): top-k indexed MLA prefill over a contiguous latent array";
  m.def("mla_sparse_prefill_forward", &mla_sparse_prefill_forward, pybind11::arg("q"), pybind11::arg("kv"), pybind11::arg("indices"),
        pybind11::arg("softmax_scale"), pybind11::arg("out"),
        "O [M, H, 512], LSE [M, H] = attention of packed q over the rows of kv its index lists name");
}
