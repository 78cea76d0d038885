// Host-side binding of fa_fwd_kvcache_mla_sparse_fp8 (include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h) for PyTorch-ROCm:
// sparse (top-k indexed) MLA decoding over the paged FP8 latent cache, for mla_sparse_fp8_kvcache.py.  One module,
// _mi355fa_mla_sparse_fp8_torch.so, beside the other decode bindings.  It does what torch_binding_mla_fp8.cpp does -- the pool is
// a uint8 tensor [num_pages, page_size, 656] whose strides are byte strides -- with the index lists of
// torch_binding_mla_sparse.cpp beside the table.  The checks that need no device come first, so that a malformed call is
// refused the same way on any machine.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h"
#include "torch_binding_mla.h"

namespace {

// softmax_scale <= 0: 576 ** -0.5.  The Python wrapper has checked what it can name better (types, grad).
std::tuple<Tensor, Tensor> kvcache_mla_sparse_fp8_forward(const Tensor& Q, const Tensor& KV, const Tensor& indices, const Tensor& seqlens,
                                                          const Tensor& table, const OptTensor& kv_new, bool is_causal,
                                                          double softmax_scale, const OptTensor& out) {
  const Pool pool{true};
  check_q(Q);
  check_q_dtype(Q);
  check_pool_dtype(KV, Q, pool);
  check_pool_shape(KV, pool);
  check_sizes(Q, KV);
  const int64_t B = Q.size(0), H = Q.size(1), Sq = Q.size(2);
  check_indices(indices, B, Sq);
  check_seqlens(seqlens, B, false);
  check_block_table(table, B);
  check_pool_in_place(KV, pool);
  check_new_and_out(kv_new, out, Q, pool);
  FA_ASSERT(!Q.requires_grad(), "flash_attention_mla_kvcache_sparse_fp8 has no backward: q must not require grad");   // a uint8 pool cannot
  check_placement(Q, KV, &indices, seqlens, table, kv_new, out);
  MlaCall c;
  prepare_mla(c, Q, KV, table, kv_new, out, softmax_scale, false);
  const int topk = (int)indices.size(2);
  const long long ws_bytes = fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes((int)B, (int)H, (int)Sq, topk, c.max_pages, c.page, c.S_new);
  Tensor ws = workspace(ws_bytes, "fa_fwd_kvcache_mla_sparse_fp8", Q);
  const long long is[2] = {B > 1 ? indices.stride(0) : 0, Sq > 1 ? indices.stride(1) : 0};   // a size-1 dim: a harmless stride
  check_rc(fa_fwd_kvcache_mla_sparse_fp8(c.Qp.data_ptr(), KV.data_ptr(), c.kn(), (const int*)indices.data_ptr(), (const int*)seqlens.data_ptr(),
      (const int*)table.data_ptr(), c.O.data_ptr(), (float*)c.LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)B, (int)H, (int)Sq, topk,
      c.num_pages, c.page, c.max_pages, table_stride_of(table, B), c.S_new, dtype_of(Q), c.scale, is_causal ? 1 : 0,
      c.Qp.is_contiguous() ? nullptr : c.qs, c.ks, c.O.is_contiguous() ? nullptr : c.os, is, current_stream(Q)),
           "fa_fwd_kvcache_mla_sparse_fp8");
  return {c.O, c.LSE};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_mla_sparse_fp8 (libmi355fa.so): top-k indexed MLA decoding over a paged FP8 latent cache";
  m.def("kvcache_mla_sparse_fp8_forward", &kvcache_mla_sparse_fp8_forward, pybind11::arg("q"), pybind11::arg("kv_cache"),
        pybind11::arg("indices"), pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("kv_new"),
        pybind11::arg("is_causal"), pybind11::arg("softmax_scale"), pybind11::arg("out"),
        "O, LSE = attention of q over the FP8 latent rows its index lists name through block_table, after quantising kv_new into "
        "them (None: no append)");
}
