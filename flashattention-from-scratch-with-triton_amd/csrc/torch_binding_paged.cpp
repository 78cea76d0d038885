// Host-side binding of fa_fwd_kvcache_paged (include/mi355fa_paged.h) and fa_fwd_kvcache_ragged (include/mi355fa_ragged.h)
// for PyTorch-ROCm: decoding attention over a paged KV cache, with q [B, H, S_q, D] for paged_kvcache.py or with packed
// variable-length queries [total_q, H, D] for ragged_kvcache.py.  One module, _mi355fa_paged_torch.so, beside
// _mi355fa_torch.so (torch_binding.cpp), whose set of functions is a recorded surface.  It does what kvcache_forward does
// there; what a decode call does and the shared part of its path are torch_binding_decode.h's.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include/mi355fa_ragged.h"
#include "torch_binding_decode.h"

namespace {

// Can the kernels address the pool [num_pages, H_kv, page_size, D] in place?  16-byte aligned rows of unit head-dim stride,
// strides that are multiples of 16 bytes (esz: bytes per element) and one (page, head) slice inside 2^31 bytes.  A pool is
// never copied -- the append writes it and a copy of a whole pool is no decode step --, so anything else is refused.
bool pool_ok(const Tensor& t, int64_t esz) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 || t.stride(3) != 1 || t.stride(2) < t.size(3)) return false;
  if ((t.size(2) - 1) * t.stride(2) * esz + t.size(3) * esz > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || (t.stride(i) * esz) % 16 != 0)) return false;
  return true;
}

// The geometry of the queries (torch_binding_common.h Queries): cu == nullptr is fa_fwd_kvcache_paged, otherwise
// fa_fwd_kvcache_ragged.
// softmax_scale <= 0: 1/sqrt(D); softcap <= 0: none.  The Python wrapper has refused the combinations of transforms.
std::tuple<Tensor, Tensor> paged_impl(const Queries& g, const Tensor& Q, const Tensor& Kp, const Tensor& Vp,
                                      const Tensor& seqlens, const Tensor& table, const OptTensor& k_new, const OptTensor& v_new,
                                      int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                                      const OptTensor& slopes, const OptTensor& sinks, const OptTensor& k_descale,
                                      const OptTensor& v_descale) {
  const bool packed = g.cu != nullptr;
  const int qdim = packed ? 3 : 4;
  FA_ASSERT(Q.dim() == qdim && Kp.dim() == 4 && Vp.dim() == 4,
            packed ? "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D]"
                   : "q must be [B, H, S_q, D], the pools [num_pages, H_kv, page_size, D]");
  const bool fp8 = Kp.scalar_type() == at::kFloat8_e4m3fn;
  FA_ASSERT(Kp.sizes() == Vp.sizes() && Kp.scalar_type() == Vp.scalar_type(), "k_cache and v_cache must have the same shape and dtype");
  if (packed) FA_ASSERT(Q.size(0) >= 1, "q must have at least one row");
  const int64_t Dq = Q.size(qdim - 1);
  FA_ASSERT(Kp.size(3) == Dq, "the pools must have q's head dim");
  FA_ASSERT(Kp.size(1) >= 1 && Q.size(1) % Kp.size(1) == 0, "q's head count must be a multiple of the pools' (H % H_kv == 0)");
  FA_ASSERT(Kp.size(2) >= 32 && Kp.size(2) % 32 == 0, "the page size (k_cache.shape[2]) must be a positive multiple of 32");
  FA_ASSERT(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  FA_ASSERT(window_left >= -1 && window_right >= -1 && window_left <= INT32_MAX && window_right <= INT32_MAX,
            "window_left / window_right must be >= -1 (-1 = unbounded) and fit in int32");
  FA_ASSERT(Q.is_cuda() && Kp.is_cuda() && Vp.is_cuda() && (!packed || g.cu->is_cuda()) && seqlens.is_cuda() && table.is_cuda(),
            packed ? "q, the pools, cu_seqlens_q, cache_seqlens and block_table must be device tensors"
                   : "q, the pools, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(Kp.device() == Q.device() && Vp.device() == Q.device() && (!packed || g.cu->device() == Q.device()) &&
                seqlens.device() == Q.device() && table.device() == Q.device(),
            "all tensors must be on q's device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
  FA_ASSERT(fp8 || Kp.scalar_type() == Q.scalar_type(), "the pools must have q's dtype or be torch.float8_e4m3fn");
  FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "head dim must be 64 or 128");   // (the decode kernels also exist at D = 256)
  if (packed) check_cu_seqlens(*g.cu);
  const int64_t B = packed ? g.cu->numel() - 1 : Q.size(0), Tq = packed ? Q.size(0) : 0, Hq = Q.size(1), Hk = Kp.size(1);
  check_seqlens(seqlens, B, packed);
  check_block_table(table, B);
  FA_ASSERT(!Q.requires_grad() && !Kp.requires_grad() && !Vp.requires_grad(),
            std::string(packed ? "flash_attention_kvcache_ragged" : "flash_attention_kvcache_paged") +
                " has no backward: q, k_cache and v_cache must not require grad");
  check_vec(slopes, "alibi_slopes", B > 0, B, Hq, Q.device());
  check_vec(sinks, "sinks", false, B, Hq, Q.device());
  check_vec(k_descale, "k_descale", B > 0, B, Hk, Q.device());
  check_vec(v_descale, "v_descale", B > 0, B, Hk, Q.device());
  const int64_t esz = fp8 ? 1 : 2;
  FA_ASSERT(pool_ok(Kp, esz) && pool_ok(Vp, esz) && (Kp.size(2) == 1 || Kp.stride(2) == Vp.stride(2)),
            "the pools must be addressable in place: 16-byte aligned rows with unit head-dim stride, strides that are multiples "
            "of 16 bytes, one row stride for K and V");
  const Descales ds = expand_descales(k_descale, v_descale, B, Hk);
  DecodeCall c;
  prepare_inputs(c, g, Q, Kp, k_new, v_new, Dims{B, Tq, Hq, Hk}, softmax_scale);
  if (packed)
    FA_ASSERT(Kp.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX && Tq <= INT32_MAX && B <= INT32_MAX,
              "too many pages, rows or sequences");
  else
    FA_ASSERT(Kp.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX, "too many pages");
  const int cache_dtype = fp8 ? MI355FA_PAGED_CACHE_FP8_E4M3 : MI355FA_PAGED_CACHE_16BIT;
  prepare_launch(c, g, Q, Kp, Vp, seqlens, &table);
  const long long ws_bytes =
      packed ? fa_fwd_kvcache_ragged_workspace_bytes(c.Tq, c.B, c.H, c.Hkv, c.max_pages, c.rows, c.D, cache_dtype)
             : fa_fwd_kvcache_paged_workspace_bytes(c.B, c.H, c.Hkv, c.Sq, c.max_pages, c.rows, c.S_new, c.D, cache_dtype);
  const char* fn = packed ? "fa_fwd_kvcache_ragged" : "fa_fwd_kvcache_paged";
  Tensor ws = workspace(ws_bytes, fn, Q);
  mi355fa_paged_mods mods{};
  mods.softcap = softcap > 0.0 ? (float)softcap : 0.f;
  mods.alibi_slopes = fptr(slopes);
  mods.slopes_batch_stride = slopes.has_value() && slopes->dim() == 2 ? (long long)slopes->size(1) : 0;
  mods.sinks = fptr(sinks);
  mods.k_descale = fptr(ds.k);
  mods.v_descale = fptr(ds.v);
  mods.descale_bstride = ds.bstride;
  const int wl = (int)window_left, wr = (int)window_right;
  check_rc(packed ? fa_fwd_kvcache_ragged(c.q, Kp.data_ptr(), Vp.data_ptr(), c.kn, c.vn, c.cu, c.seqlens, c.table, c.o, c.lse,
                                          ws.data_ptr(), ws_bytes, c.Tq, c.B, c.H, c.Hkv, c.num_pages, c.rows, c.max_pages,
                                          c.table_stride, c.D, c.dtype, cache_dtype, c.scale, wl, wr, &mods, &c.opts, c.stream)
                  : fa_fwd_kvcache_paged(c.q, Kp.data_ptr(), Vp.data_ptr(), c.kn, c.vn, c.seqlens, c.table, c.o, c.lse, ws.data_ptr(),
                                         ws_bytes, c.B, c.H, c.Hkv, c.Sq, c.num_pages, c.rows, c.max_pages, c.table_stride, c.S_new,
                                         c.D, c.dtype, cache_dtype, c.scale, wl, wr, &mods, &c.opts, c.stream),
           fn);
  return {c.O, c.LSE};
}

std::tuple<Tensor, Tensor> kvcache_paged_forward(const Tensor& Q, const Tensor& Kp, const Tensor& Vp, const Tensor& seqlens,
                                                 const Tensor& table, const OptTensor& k_new, const OptTensor& v_new,
                                                 int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                                                 const OptTensor& slopes, const OptTensor& sinks, const OptTensor& k_descale,
                                                 const OptTensor& v_descale) {
  return paged_impl(Queries{}, Q, Kp, Vp, seqlens, table, k_new, v_new, window_left, window_right, softmax_scale, softcap,
                    slopes, sinks, k_descale, v_descale);
}

std::tuple<Tensor, Tensor> kvcache_ragged_forward(const Tensor& Q, const Tensor& Kp, const Tensor& Vp, const Tensor& cu,
                                                  const Tensor& seqlens, const Tensor& table, const OptTensor& k_new,
                                                  const OptTensor& v_new, int64_t window_left, int64_t window_right,
                                                  double softmax_scale, double softcap, const OptTensor& slopes,
                                                  const OptTensor& sinks, const OptTensor& k_descale, const OptTensor& v_descale,
                                                  const OptTensor& out) {
  return paged_impl(Queries{&cu, &out}, Q, Kp, Vp, seqlens, table, k_new, v_new, window_left, window_right, softmax_scale,
                    softcap, slopes, sinks, k_descale, v_descale);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  using pybind11::arg;
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_paged and fa_fwd_kvcache_ragged (libmi355fa.so): decoding attention over a "
            "paged KV cache, also with packed variable-length queries";
  m.def("kvcache_paged_forward", &kvcache_paged_forward, arg("q"), arg("k_cache"), arg("v_cache"), arg("cache_seqlens"),
        arg("block_table"), arg("k_new"), arg("v_new"), arg("window_left"), arg("window_right"), arg("softmax_scale"),
        arg("softcap"), arg("alibi_slopes"), arg("sinks"), arg("k_descale"), arg("v_descale"),
        "O, LSE = attention of q over the pages block_table names, after appending k_new / v_new (None: no append)");
  m.def("kvcache_ragged_forward", &kvcache_ragged_forward, arg("q"), arg("k_cache"), arg("v_cache"), arg("cu_seqlens_q"),
        arg("cache_seqlens"), arg("block_table"), arg("k_new"), arg("v_new"), arg("window_left"), arg("window_right"),
        arg("softmax_scale"), arg("softcap"), arg("alibi_slopes"), arg("sinks"), arg("k_descale"), arg("v_descale"), arg("out"),
        "O, LSE = attention of the packed q over the pages block_table names, after appending k_new / v_new (None: no append)");
}
