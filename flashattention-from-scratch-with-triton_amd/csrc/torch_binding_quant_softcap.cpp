// Host-side binding of fa_fwd_kvcache_quant_softcap, _paged and _ragged (include_quant/mi355fa_kvcache_quant_softcap.h) for
// PyTorch-ROCm: soft-capped decoding attention over a per-tensor e4m3, a per-token-scaled e4m3 or an MXFP4 KV cache -- padded,
// paged, and with packed variable-length queries over paged pools -- for quant_softcap_kvcache.py.  One module,
// _mi355fa_quant_softcap_torch.so, beside the others, whose sets of functions are recorded surfaces.  What a decode call does and
// the shared part of its path are torch_binding_decode.h's; here are the checks of the three formats, the workspace calls and the
// three launches.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <cmath>
#include <string>
#include <tuple>

#include "../../include_quant/mi355fa_kvcache_quant_softcap.h"
#include "torch_binding_decode.h"

namespace {

// format: the header's MI355FA_QUANT_* (the Python wrapper derives it from the tensors).  Kc / Vc: float8_e4m3fn [.., H_kv, rows, D]
// (E4M3, E4M3_TOKEN) or uint8 [.., H_kv, rows, D / 2] (MXFP4); Ks / Vs: float32 [.., H_kv, rows] (E4M3_TOKEN), uint8
// [.., H_kv, rows, D / 32] (MXFP4) or None (E4M3); Kd / Vd: float32 (H_kv,) or (B, H_kv), E4M3 only; table: int32 [B, max_pages] for a
// paged cache, None for a padded one.  softmax_scale <= 0: 1/sqrt(D).  g (torch_binding_common.h Queries): cu == nullptr is q
// [B, H, S_q, D], otherwise packed q [total_q, H, D] over paged pools.
std::tuple<Tensor, Tensor> quant_impl(const Queries& g, const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                      const OptTensor& table, double softcap, int64_t format, const OptTensor& Ks,
                                      const OptTensor& Vs, const OptTensor& Kd, const OptTensor& Vd, const OptTensor& k_new,
                                      const OptTensor& v_new, int64_t window_left, int64_t window_right, double softmax_scale) {
  const bool packed = g.cu != nullptr, paged = table.has_value();
  const bool e4m3 = format == MI355FA_QUANT_E4M3, token = format == MI355FA_QUANT_E4M3_TOKEN, fp4 = format == MI355FA_QUANT_MXFP4;
  FA_ASSERT(e4m3 || token || fp4, "format must be 0 (per-tensor e4m3), 1 (per-token e4m3) or 2 (MXFP4)");
  const int qdim = packed ? 3 : 4;
  FA_ASSERT(Q.dim() == qdim && Kc.dim() == 4 && Vc.dim() == 4,
            packed ? "q must be [total_q, H, D] and the pools 4-d [num_pages, H_kv, page_size, row]"
                   : "q must be [B, H, S_q, D] and the caches 4-d [.., H_kv, rows, row]");
  check_packed_front(g, Q, table);
  FA_ASSERT(Ks.has_value() == Vs.has_value() && Ks.has_value() == !e4m3,
            "k_scale and v_scale come with a per-token e4m3 or an MXFP4 cache, and with no other");
  FA_ASSERT(e4m3 || (!Kd.has_value() && !Vd.has_value()), "k_descale / v_descale belong to a per-tensor e4m3 cache");
  const int64_t Dq = Q.size(qdim - 1);
  if (fp4) {
    for (const Tensor* t : {&Kc, &Vc, &*Ks, &*Vs})
      FA_ASSERT(t->scalar_type() == at::kByte, "the MXFP4 caches and their scales are passed as bytes");
    FA_ASSERT(Ks->dim() == 4 && Vs->dim() == 4, "the MXFP4 scales must be [.., H_kv, rows, D / 32]");
  } else {
    FA_ASSERT(Kc.scalar_type() == at::kFloat8_e4m3fn && Vc.scalar_type() == at::kFloat8_e4m3fn,
              "k_cache and v_cache must be torch.float8_e4m3fn");
    if (token)
      FA_ASSERT(Ks->scalar_type() == at::kFloat && Vs->scalar_type() == at::kFloat && Ks->dim() == 3 && Vs->dim() == 3,
                "k_scale and v_scale must be float32 [.., H_kv, rows]");
  }
  if (e4m3)
    FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "a per-tensor e4m3 cache takes head dim 64, 128 or 256");
  else if (packed)
    FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "packed queries over a per-token e4m3 or an MXFP4 cache take head dim 64, 128 or 256");
  else
    FA_ASSERT(Dq == 64 || Dq == 128, "a per-token e4m3 or an MXFP4 cache takes head dim 64 or 128 (256 with packed queries)");
  FA_ASSERT(Kc.sizes() == Vc.sizes() && Kc.size(3) == (fp4 ? Dq / 2 : Dq),
            "k_cache and v_cache must have the same shape, rows of D bytes (MXFP4: D / 2)");
  if (!e4m3) {
    FA_ASSERT(Ks->sizes() == Vs->sizes() && Ks->size(0) == Kc.size(0) && Ks->size(1) == Kc.size(1) && Ks->size(2) == Kc.size(2) &&
                  (!fp4 || Ks->size(3) == Dq / 32),
              "k_scale and v_scale must have the caches' leading dimensions (MXFP4: and rows of D / 32 bytes)");
  }
  check_heads_new_window(Q, Kc, k_new, v_new, window_left, window_right);
  FA_ASSERT(std::isfinite(softcap) && softcap > 0.0, "softcap must be finite and > 0");
  const Dims d = check_placement_and_geometry(g, Q, Kc, Vc, e4m3 ? nullptr : &*Ks, e4m3 ? nullptr : &*Vs, seqlens, table,
                                              "flash_attention_kvcache_quant_softcap", true);
  check_vec(Kd, "k_descale", true, d.B, d.Hk, Q.device());
  check_vec(Vd, "v_descale", true, d.B, d.Hk, Q.device());
  check_caches_in_place(Kc, Vc);
  if (fp4)
    FA_ASSERT(bytes_ok(*Ks, Dq / 32) && bytes_ok(*Vs, Dq / 32),
              "the scales must be addressable in place: rows of D / 32 bytes with unit stride, aligned to D / 32 bytes, strides "
              "that are multiples of D / 32 bytes");
  if (token)
    FA_ASSERT(row_scales_ok(*Ks) && row_scales_ok(*Vs) && !Ks->requires_grad() && !Vs->requires_grad(),
              "the scales must be addressable in place: non-negative strides, one (batch, head) slice below 2^31 bytes, no grad");
  const Descales ds = expand_descales(Kd, Vd, d.B, d.Hk);
  DecodeCall c;
  prepare_inputs(c, g, Q, Kc, k_new, v_new, d, softmax_scale);
  prepare_launch(c, g, Q, Kc, Vc, seqlens, paged ? &*table : nullptr);
  const int fmt = (int)format;
  const long long ws_bytes =
      packed  ? fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes(fmt, c.Tq, c.B, c.H, c.Hkv, c.max_pages, c.rows, c.D)
      : paged ? fa_fwd_kvcache_quant_softcap_paged_workspace_bytes(fmt, c.B, c.H, c.Hkv, c.Sq, c.max_pages, c.rows, c.S_new, c.D)
              : fa_fwd_kvcache_quant_softcap_workspace_bytes(fmt, c.B, c.H, c.Hkv, c.Sq, c.rows, c.S_new, c.D);
  const char* fn = packed  ? "fa_fwd_kvcache_quant_softcap_ragged"
                   : paged ? "fa_fwd_kvcache_quant_softcap_paged"
                           : "fa_fwd_kvcache_quant_softcap";
  Tensor ws = workspace(ws_bytes, fn, Q);
  long long kss[3], vss[3];
  mi355fa_quant_cache cache{};
  cache.format = fmt;
  if (e4m3) {
    cache.k_descale = fptr(ds.k);
    cache.v_descale = fptr(ds.v);
    cache.descale_bstride = ds.bstride;
  } else {
    if (fp4) {
      strides3(*Ks, kss);
      strides3(*Vs, vss);
    } else {
      row_scale_strides(*Ks, kss);
      row_scale_strides(*Vs, vss);
    }
    cache.k_scale = Ks->data_ptr();
    cache.v_scale = Vs->data_ptr();
    cache.k_scale_strides = kss;
    cache.v_scale_strides = vss;
  }
  const float cap = (float)softcap;
  const int wl = (int)window_left, wr = (int)window_right;
  check_rc(packed  ? fa_fwd_kvcache_quant_softcap_ragged(c.q, Kc.data_ptr(), Vc.data_ptr(), c.kn, c.vn, c.cu, c.seqlens, c.table, c.o,
                                                         c.lse, ws.data_ptr(), ws_bytes, c.Tq, c.B, c.H, c.Hkv, c.num_pages, c.rows,
                                                         c.max_pages, c.table_stride, c.D, c.dtype, c.scale, cap, wl, wr, &cache,
                                                         &c.opts, c.stream)
           : paged ? fa_fwd_kvcache_quant_softcap_paged(c.q, Kc.data_ptr(), Vc.data_ptr(), c.kn, c.vn, c.seqlens, c.table, c.o, c.lse,
                                                        ws.data_ptr(), ws_bytes, c.B, c.H, c.Hkv, c.Sq, c.num_pages, c.rows,
                                                        c.max_pages, c.table_stride, c.S_new, c.D, c.dtype, c.scale, cap, wl, wr,
                                                        &cache, &c.opts, c.stream)
                   : fa_fwd_kvcache_quant_softcap(c.q, Kc.data_ptr(), Vc.data_ptr(), c.kn, c.vn, c.seqlens, c.o, c.lse, ws.data_ptr(),
                                                  ws_bytes, c.B, c.H, c.Hkv, c.Sq, c.rows, c.S_new, c.D, c.dtype, c.scale, cap, wl,
                                                  wr, &cache, &c.opts, c.stream),
           fn);
  return {c.O, c.LSE};
}

std::tuple<Tensor, Tensor> kvcache_quant_softcap_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                                         const OptTensor& table, double softcap, int64_t format,
                                                         const OptTensor& Ks, const OptTensor& Vs, const OptTensor& Kd,
                                                         const OptTensor& Vd, const OptTensor& k_new, const OptTensor& v_new,
                                                         int64_t window_left, int64_t window_right, double softmax_scale) {
  return quant_impl(Queries{}, Q, Kc, Vc, seqlens, table, softcap, format, Ks, Vs, Kd, Vd, k_new, v_new, window_left, window_right,
                    softmax_scale);
}

std::tuple<Tensor, Tensor> kvcache_quant_softcap_ragged_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& cu,
                                                                const Tensor& seqlens, const Tensor& table, double softcap,
                                                                int64_t format, const OptTensor& Ks, const OptTensor& Vs,
                                                                const OptTensor& Kd, const OptTensor& Vd, const OptTensor& k_new,
                                                                const OptTensor& v_new, int64_t window_left, int64_t window_right,
                                                                double softmax_scale, const OptTensor& out) {
  return quant_impl(Queries{&cu, &out}, Q, Kc, Vc, seqlens, OptTensor(table), softcap, format, Ks, Vs, Kd, Vd, k_new, v_new,
                    window_left, window_right, softmax_scale);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  using pybind11::arg;
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_quant_softcap, _paged and _ragged (libmi355fa.so): soft-capped decoding "
            "attention over per-tensor e4m3, per-token e4m3 and MXFP4 KV caches";
  m.def("kvcache_quant_softcap_forward", &kvcache_quant_softcap_forward, arg("q"), arg("k_cache"), arg("v_cache"),
        arg("cache_seqlens"), arg("block_table"), arg("softcap"), arg("format"), arg("k_scale"), arg("v_scale"), arg("k_descale"),
        arg("v_descale"), arg("k_new"), arg("v_new"), arg("window_left"), arg("window_right"), arg("softmax_scale"),
        "O, LSE = soft-capped attention of q over the quantised cache (block_table: its pages), after appending k_new / v_new "
        "(None: no append)");
  m.def("kvcache_quant_softcap_ragged_forward", &kvcache_quant_softcap_ragged_forward, arg("q"), arg("k_cache"), arg("v_cache"),
        arg("cu_seqlens_q"), arg("cache_seqlens"), arg("block_table"), arg("softcap"), arg("format"), arg("k_scale"),
        arg("v_scale"), arg("k_descale"), arg("v_descale"), arg("k_new"), arg("v_new"), arg("window_left"), arg("window_right"),
        arg("softmax_scale"), arg("out"),
        "O, LSE = soft-capped attention of the packed q over the quantised pages block_table names, after appending k_new / v_new "
        "(None: no append)");
}
