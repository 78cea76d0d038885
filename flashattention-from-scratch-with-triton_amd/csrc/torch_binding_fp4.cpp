// Host-side binding of fa_fwd_kvcache_fp4 and fa_fwd_kvcache_fp4_paged (include/mi355fa_kvcache_fp4.h) and of
// fa_fwd_kvcache_fp4_ragged (include/mi355fa_ragged_fp4.h) for PyTorch-ROCm: decoding attention over an MXFP4 KV cache, padded
// or paged, for fp4_kvcache.py, and with packed variable-length queries over paged pools for fp4_ragged_kvcache.py.  One module,
// _mi355fa_fp4_torch.so, beside _mi355fa_torch.so and _mi355fa_paged_torch.so, whose sets of functions are recorded surfaces.
// What a decode call does and the shared part of its path are torch_binding_decode.h's; here are the checks of the format, the
// workspace calls and the three launches.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include/mi355fa_ragged_fp4.h"
#include "torch_binding_decode.h"

namespace {

// Kc / Vc: uint8 [B | num_pages, H_kv, S_cache | page_size, D / 2]; Ks / Vs: uint8 [.., D / 32]; table: int32 [B, max_pages]
// for a paged cache, None for a padded one.  softmax_scale <= 0: 1/sqrt(D).  g (torch_binding_common.h Queries): cu == nullptr
// is q [B, H, S_q, D] and fa_fwd_kvcache_fp4 / _fp4_paged, otherwise packed q [total_q, H, D] over paged pools and
// fa_fwd_kvcache_fp4_ragged, the one form with D = 256.
std::tuple<Tensor, Tensor> fp4_impl(const Queries& g, const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& Ks,
                                    const Tensor& Vs, const Tensor& seqlens, const OptTensor& table, const OptTensor& k_new,
                                    const OptTensor& v_new, int64_t window_left, int64_t window_right, double softmax_scale,
                                    const OptTensor& sinks) {
  const bool packed = g.cu != nullptr, paged = table.has_value();
  const int qdim = packed ? 3 : 4;
  FA_ASSERT(Q.dim() == qdim && Kc.dim() == 4 && Vc.dim() == 4 && Ks.dim() == 4 && Vs.dim() == 4,
            packed ? "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D / 2] and the scales [num_pages, H_kv, page_size, D / 32]"
                   : "q must be [B, H, S_q, D], the caches [.., H_kv, rows, D / 2] and the scales [.., H_kv, rows, D / 32]");
  check_packed_front(g, Q, table);
  for (const Tensor* t : {&Kc, &Vc, &Ks, &Vs})
    FA_ASSERT(t->scalar_type() == at::kByte, "the MXFP4 caches and their scales are passed as bytes");
  const int64_t Dq = Q.size(qdim - 1);
  if (packed)
    FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "packed queries over an MXFP4 cache take head dim 64, 128 or 256");
  else
    FA_ASSERT(Dq == 64 || Dq == 128, "an MXFP4 cache takes head dim 64 or 128");
  FA_ASSERT(Kc.sizes() == Vc.sizes() && Kc.size(3) == Dq / 2, "k_cache and v_cache must have the same shape, rows of D / 2 bytes");
  FA_ASSERT(Ks.sizes() == Vs.sizes() && Ks.size(3) == Dq / 32 && Ks.size(0) == Kc.size(0) && Ks.size(1) == Kc.size(1) &&
                Ks.size(2) == Kc.size(2),
            "k_scale and v_scale must have the caches' leading dimensions and rows of D / 32 bytes");
  check_heads_new_window(Q, Kc, k_new, v_new, window_left, window_right);
  const Dims d = check_placement_and_geometry(g, Q, Kc, Vc, &Ks, &Vs, seqlens, table, "flash_attention_kvcache_fp4", false);
  check_sinks(sinks, d.Hq, Q.device());
  check_caches_in_place(Kc, Vc);
  FA_ASSERT(bytes_ok(Ks, Dq / 32) && bytes_ok(Vs, Dq / 32),
            "the scales must be addressable in place: rows of D / 32 bytes with unit stride, aligned to D / 32 bytes, strides "
            "that are multiples of D / 32 bytes");
  DecodeCall c;
  prepare_inputs(c, g, Q, Kc, k_new, v_new, d, softmax_scale);
  prepare_launch(c, g, Q, Kc, Vc, seqlens, paged ? &*table : nullptr);
  const long long ws_bytes = packed  ? fa_fwd_kvcache_fp4_ragged_workspace_bytes(c.Tq, c.B, c.H, c.Hkv, c.max_pages, c.rows, c.D)
                             : paged ? fa_fwd_kvcache_fp4_paged_workspace_bytes(c.B, c.H, c.Hkv, c.Sq, c.max_pages, c.rows, c.S_new, c.D)
                                     : fa_fwd_kvcache_fp4_workspace_bytes(c.B, c.H, c.Hkv, c.Sq, c.rows, c.S_new, c.D);
  const char* fn = packed ? "fa_fwd_kvcache_fp4_ragged" : paged ? "fa_fwd_kvcache_fp4_paged" : "fa_fwd_kvcache_fp4";
  Tensor ws = workspace(ws_bytes, fn, Q);
  long long kss[3], vss[3];
  strides3(Ks, kss);
  strides3(Vs, vss);
  const float* sk = fptr(sinks);
  const int wl = (int)window_left, wr = (int)window_right;
  check_rc(packed  ? fa_fwd_kvcache_fp4_ragged(c.q, Kc.data_ptr(), Vc.data_ptr(), Ks.data_ptr(), Vs.data_ptr(), c.kn, c.vn, c.cu,
                                               c.seqlens, c.table, kss, vss, sk, c.o, c.lse, ws.data_ptr(), ws_bytes, c.Tq, c.B, c.H,
                                               c.Hkv, c.num_pages, c.rows, c.max_pages, c.table_stride, c.D, c.dtype,
                                               MI355FA_KV_MXFP4, c.scale, wl, wr, &c.opts, c.stream)
           : paged ? fa_fwd_kvcache_fp4_paged(c.q, Kc.data_ptr(), Vc.data_ptr(), Ks.data_ptr(), Vs.data_ptr(), c.kn, c.vn, c.seqlens,
                                              c.table, kss, vss, sk, c.o, c.lse, ws.data_ptr(), ws_bytes, c.B, c.H, c.Hkv, c.Sq,
                                              c.num_pages, c.rows, c.max_pages, c.table_stride, c.S_new, c.D, c.dtype,
                                              MI355FA_KV_MXFP4, c.scale, wl, wr, &c.opts, c.stream)
                   : fa_fwd_kvcache_fp4(c.q, Kc.data_ptr(), Vc.data_ptr(), Ks.data_ptr(), Vs.data_ptr(), c.kn, c.vn, c.seqlens, kss,
                                        vss, sk, c.o, c.lse, ws.data_ptr(), ws_bytes, c.B, c.H, c.Hkv, c.Sq, c.rows, c.S_new, c.D,
                                        c.dtype, MI355FA_KV_MXFP4, c.scale, wl, wr, &c.opts, c.stream),
           fn);
  return {c.O, c.LSE};
}

std::tuple<Tensor, Tensor> kvcache_fp4_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& Ks,
                                               const Tensor& Vs, const Tensor& seqlens, const OptTensor& table,
                                               const OptTensor& k_new, const OptTensor& v_new, int64_t window_left,
                                               int64_t window_right, double softmax_scale, const OptTensor& sinks) {
  return fp4_impl(Queries{}, Q, Kc, Vc, Ks, Vs, seqlens, table, k_new, v_new, window_left, window_right, softmax_scale, sinks);
}

std::tuple<Tensor, Tensor> kvcache_fp4_ragged_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& Ks,
                                                      const Tensor& Vs, const Tensor& cu, const Tensor& seqlens,
                                                      const Tensor& table, const OptTensor& k_new, const OptTensor& v_new,
                                                      int64_t window_left, int64_t window_right, double softmax_scale,
                                                      const OptTensor& sinks, const OptTensor& out) {
  return fp4_impl(Queries{&cu, &out}, Q, Kc, Vc, Ks, Vs, seqlens, OptTensor(table), k_new, v_new, window_left, window_right,
                  softmax_scale, sinks);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  using pybind11::arg;
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_fp4, fa_fwd_kvcache_fp4_paged and fa_fwd_kvcache_fp4_ragged (libmi355fa.so): "
            "decoding attention over an MXFP4 KV cache, padded or paged, also with packed variable-length queries";
  m.def("kvcache_fp4_forward", &kvcache_fp4_forward, arg("q"), arg("k_cache"), arg("v_cache"), arg("k_scale"), arg("v_scale"),
        arg("cache_seqlens"), arg("block_table"), arg("k_new"), arg("v_new"), arg("window_left"), arg("window_right"),
        arg("softmax_scale"), arg("sinks"),
        "O, LSE = attention of q over the MXFP4 cache (block_table: its pages), after appending k_new / v_new (None: no append)");
  m.def("kvcache_fp4_ragged_forward", &kvcache_fp4_ragged_forward, arg("q"), arg("k_cache"), arg("v_cache"), arg("k_scale"),
        arg("v_scale"), arg("cu_seqlens_q"), arg("cache_seqlens"), arg("block_table"), arg("k_new"), arg("v_new"),
        arg("window_left"), arg("window_right"), arg("softmax_scale"), arg("sinks"), arg("out"),
        "O, LSE = attention of the packed q over the MXFP4 pages block_table names, after appending k_new / v_new (None: no append)");
}
