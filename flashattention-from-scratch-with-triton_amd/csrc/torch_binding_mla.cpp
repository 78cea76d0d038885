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
#include "torch_binding_mla.h"

namespace {

// softmax_scale <= 0: 576 ** -0.5.  The Python wrapper has checked what it can name better (types, grad).
std::tuple<Tensor, Tensor> kvcache_mla_forward(const Tensor& Q, const Tensor& KV, const Tensor& seqlens, const Tensor& table,
                                               const OptTensor& kv_new, bool is_causal, double softmax_scale, const OptTensor& out) {
  const Pool pool{false};
  check_q(Q);
  check_pool_shape(KV, pool);
  check_q_dtype(Q);
  check_pool_dtype(KV, Q, pool);
  check_sizes(Q, KV);
  const int64_t B = Q.size(0), H = Q.size(1), Sq = Q.size(2);
  check_seqlens(seqlens, B, false);
  check_block_table(table, B);
  check_pool_in_place(KV, pool);
  check_new_and_out(kv_new, out, Q, pool);
  FA_ASSERT(!Q.requires_grad() && !KV.requires_grad(),
            "flash_attention_mla_kvcache has no backward: q and kv_cache must not require grad");
  check_placement(Q, KV, nullptr, seqlens, table, kv_new, out);
  MlaCall c;
  prepare_mla(c, Q, KV, table, kv_new, out, softmax_scale, false);
  const long long ws_bytes = fa_fwd_kvcache_mla_workspace_bytes((int)B, (int)H, (int)Sq, c.max_pages, c.page, c.S_new);
  Tensor ws = workspace(ws_bytes, "fa_fwd_kvcache_mla", Q);
  check_rc(fa_fwd_kvcache_mla(c.Qp.data_ptr(), KV.data_ptr(), c.kn(), (const int*)seqlens.data_ptr(), (const int*)table.data_ptr(),
      c.O.data_ptr(), (float*)c.LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)B, (int)H, (int)Sq, c.num_pages, c.page, c.max_pages,
      table_stride_of(table, B), c.S_new, dtype_of(Q), c.scale, is_causal ? 1 : 0, c.Qp.is_contiguous() ? nullptr : c.qs, c.ks,
      c.O.is_contiguous() ? nullptr : c.os, current_stream(Q)),
           "fa_fwd_kvcache_mla");
  return {c.O, c.LSE};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_mla (libmi355fa.so): MLA decoding attention over a paged latent cache";
  m.def("kvcache_mla_forward", &kvcache_mla_forward, pybind11::arg("q"), pybind11::arg("kv_cache"), pybind11::arg("cache_seqlens"),
        pybind11::arg("block_table"), pybind11::arg("kv_new"), pybind11::arg("is_causal"), pybind11::arg("softmax_scale"),
        pybind11::arg("out"),
        "O, LSE = attention of q over the latent rows block_table names, after appending kv_new (None: no append)");
}
