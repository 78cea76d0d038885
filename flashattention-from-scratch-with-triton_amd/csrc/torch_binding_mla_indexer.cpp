// Host-side binding of fa_mla_indexer_logits_fp8 (include_mla_indexer/mi355fa_mla_indexer.h) for PyTorch-ROCm: the DeepSeek-V3.2
// indexer logits over a paged FP8 key cache, and of fa_mla_indexer_select (include_mla_select/mi355fa_mla_select.h), the top-k
// selection from them, and of fa_mla_indexer_logits_fp8_prefill (include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h), the
// logits of a prefill step, for mla_indexer.py.  One module, _mi355fa_mla_indexer_torch.so, beside the other
// decode bindings.  The checks that need no device come first, so that a malformed call is refused the same way on any machine.
// The pools are addressed in place -- the append writes them --, q through its strides when the kernel can and as a contiguous
// copy otherwise; the launch goes to the current stream and nothing reads cache_seqlens or block_table.
//
// Built by csrc/Makefile with g++ (host code only).
#include <torch/extension.h>

#include <string>

#include "../../include_mla_indexer/mi355fa_mla_indexer.h"
#include "../../include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h"
#include "../../include_mla_select/mi355fa_mla_select.h"
#include "torch_binding_decode.h"

namespace {

std::string num(int64_t v) { return std::to_string((long long)v); }

bool is_bytes(const Tensor& t) { return t.scalar_type() == at::kFloat8_e4m3fn || t.scalar_type() == at::kByte; }

// Can the kernel read q [B, S_q, H_i, 128] in place?  16-byte rows with unit stride along the dims.
bool q_ok(const Tensor& t) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 || t.stride(3) != 1) return false;
  if (t.size(2) > 1 && t.stride(2) < t.size(3)) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % 16 != 0)) return false;
  return true;
}

Tensor indexer_logits_fp8(const Tensor& Q, const Tensor& Wt, const Tensor& Kc, const Tensor& Ks, const Tensor& seqlens,
                          const Tensor& table, const OptTensor& k_new, bool is_causal, const OptTensor& out) {
  FA_ASSERT(is_bytes(Q), "q must be torch.float8_e4m3fn or its uint8 view");
  FA_ASSERT(Q.dim() == 4, "q must be [B, S_q, H_i, 128] (got " + num(Q.dim()) + " dims)");
  FA_ASSERT(Q.size(3) == 128, "q's last dim must be 128 (got " + num(Q.size(3)) + ")");
  FA_ASSERT(Q.size(2) >= 16 && Q.size(2) <= 64 && Q.size(2) % 16 == 0,
            "H_i (q.shape[2]) must be a multiple of 16 in [16, 64] (got " + num(Q.size(2)) + ")");
  FA_ASSERT(Q.size(0) >= 1 && Q.size(1) >= 1, "q must not be empty");
  const int64_t B = Q.size(0), Sq = Q.size(1), Hi = Q.size(2);
  FA_ASSERT(Wt.scalar_type() == at::kFloat && Wt.dim() == 3 && Wt.size(0) == B && Wt.size(1) == Sq && Wt.size(2) == Hi,
            "weights must be float32 [B, S_q, H_i]");
  FA_ASSERT(is_bytes(Kc), "k_cache must be torch.float8_e4m3fn or its uint8 view");
  FA_ASSERT(Kc.dim() == 3 && Kc.size(2) == 128 && Kc.size(0) >= 1, "k_cache must be [num_pages, page_size, 128]");
  FA_ASSERT(Kc.size(1) >= 32 && Kc.size(1) % 32 == 0,
            "the page size (k_cache.shape[1] = " + num(Kc.size(1)) + ") must be a positive multiple of 32");
  FA_ASSERT(Ks.scalar_type() == at::kFloat && Ks.dim() == 2 && Ks.size(0) == Kc.size(0) && Ks.size(1) == Kc.size(1),
            "k_scale must be float32 [num_pages, page_size]");
  check_seqlens(seqlens, B, false);
  check_block_table(table, B);
  FA_ASSERT(Kc.stride(2) == 1 && Kc.stride(1) >= 128 && Kc.stride(1) % 16 == 0 && Kc.stride(1) <= (1 << 24) &&
                (Kc.size(0) == 1 || (Kc.stride(0) >= 0 && Kc.stride(0) % 16 == 0)),
            "k_cache must be addressable in place: unit stride along the 128 bytes, a row stride that is a multiple of 16 and at "
            "least 128 (got " + num(Kc.stride(1)) + ") and a page stride that is a multiple of 16");
  if (k_new.has_value()) {
    FA_ASSERT(k_new->dim() == 3 && k_new->size(0) == B && k_new->size(1) == Sq && k_new->size(2) == 128,
              "k_new must be [B, S_q, 128]: one cached key per query row");
    FA_ASSERT((k_new->scalar_type() == at::kHalf || k_new->scalar_type() == at::kBFloat16) && !k_new->requires_grad(),
              "k_new must be float16 or bfloat16 and must not require grad");
  }
  if (out.has_value()) {
    FA_ASSERT(out->scalar_type() == at::kFloat && out->dim() == 3 && out->size(0) == B && out->size(1) == Sq && out->size(2) >= 1,
              "out must be float32 [B, S_q, W] with W >= 1");
    FA_ASSERT((out->size(2) == 1 || out->stride(2) == 1) && (Sq == 1 || out->stride(1) >= out->size(2)) && (B == 1 || out->stride(0) > 0) &&
                  !out->requires_grad(),
              "out must be addressable in place (unit stride along W, rows that do not overlap) and must not require grad");
  }
  FA_ASSERT(!Q.requires_grad() && !Wt.requires_grad() && !Kc.requires_grad() && !Ks.requires_grad(),
            "mla_indexer_logits_fp8 has no backward: no input may require grad");
  FA_ASSERT(Q.is_cuda() && Wt.is_cuda() && Kc.is_cuda() && Ks.is_cuda() && seqlens.is_cuda() && table.is_cuda(),
            "q, weights, k_cache, k_scale, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(Wt.device() == Q.device() && Kc.device() == Q.device() && Ks.device() == Q.device() && seqlens.device() == Q.device() &&
                table.device() == Q.device() && (!k_new.has_value() || k_new->device() == Q.device()) &&
                (!out.has_value() || out->device() == Q.device()),
            "all tensors must be on q's device");
  FA_ASSERT(reinterpret_cast<uintptr_t>(Kc.data_ptr()) % 16 == 0, "k_cache must be 16-byte aligned");
  FA_ASSERT(Kc.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX && table.size(1) * Kc.size(1) <= INT32_MAX && B <= 65535,
            "too many pages or sequences");
  const Tensor Qp = q_ok(Q) ? Q : Q.clone(at::MemoryFormat::Contiguous);
  Tensor Kn;
  if (k_new.has_value()) Kn = contiguous16(*k_new);
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out.has_value() ? *out : torch::empty({B, Sq, table.size(1) * Kc.size(1)}, Q.options().dtype(at::kFloat));
  FA_ASSERT(O.size(2) <= INT32_MAX, "W too large");
  const long long qs[3] = {B > 1 ? Qp.stride(0) : 0, Sq > 1 ? Qp.stride(1) : 0, Qp.stride(2)};   // a size-1 dim: a harmless stride
  const long long ws[3] = {B > 1 ? Wt.stride(0) : 0, Sq > 1 ? Wt.stride(1) : 0, Wt.stride(2)};
  const long long ks[2] = {Kc.size(0) > 1 ? Kc.stride(0) : 0, Kc.stride(1)};
  const long long ss[2] = {Ks.size(0) > 1 ? Ks.stride(0) : 0, Ks.stride(1)};
  const long long os[2] = {B > 1 ? O.stride(0) : Sq * O.size(2), Sq > 1 ? O.stride(1) : O.size(2)};
  check_rc(fa_mla_indexer_logits_fp8(Qp.data_ptr(), (const float*)Wt.data_ptr(), Kc.data_ptr(), (float*)Ks.data_ptr(),
                                     Kn.defined() ? Kn.data_ptr() : nullptr, (const int*)seqlens.data_ptr(), (const int*)table.data_ptr(),
                                     (float*)O.data_ptr(), (int)B, (int)Sq, (int)Hi, (int)O.size(2), (int)Kc.size(0), (int)Kc.size(1),
                                     (int)table.size(1), table_stride_of(table, B), Kn.defined() ? (int)Sq : 0,
                                     Kn.defined() && Kn.scalar_type() == at::kBFloat16 ? MI355FA_BF16 : MI355FA_FP16, is_causal ? 1 : 0, qs,
                                     ws, ks, ss, os, current_stream(Q)),
           "fa_mla_indexer_logits_fp8");
  return O;
}

// fa_mla_indexer_select (include_mla_select/mi355fa_mla_select.h): logits and `out` in place through their batch and row strides,
// nothing copied, nothing but a missing `out` allocated, `lengths` never read.
Tensor indexer_select(const Tensor& L, int64_t topk, const OptTensor& lengths, const OptTensor& out) {
  FA_ASSERT(L.scalar_type() == at::kFloat && L.dim() == 3, "logits must be float32 [B, S_q, W]");
  FA_ASSERT(L.size(0) >= 1 && L.size(1) >= 1 && L.size(2) >= 1, "logits must not be empty");
  const int64_t B = L.size(0), Sq = L.size(1), W = L.size(2);
  FA_ASSERT(topk >= 1 && topk <= 65536, "topk must be in [1, 65536] (got " + num(topk) + ")");
  FA_ASSERT((W == 1 || L.stride(2) == 1) && (Sq == 1 || L.stride(1) >= W) && (B == 1 || L.stride(0) > 0),
            "logits must be addressable in place: unit stride along W, rows that do not overlap (row stride " + num(L.stride(1)) + ")");
  if (lengths.has_value())
    FA_ASSERT(lengths->scalar_type() == at::kInt && lengths->dim() == 1 && lengths->numel() == B && lengths->is_contiguous(),
              "lengths must be a contiguous int32 vector of B entries");
  if (out.has_value()) {
    FA_ASSERT(out->scalar_type() == at::kInt && out->dim() == 3 && out->size(0) == B && out->size(1) == Sq && out->size(2) == topk,
              "out must be int32 [B, S_q, topk]");
    FA_ASSERT((topk == 1 || out->stride(2) == 1) && (Sq == 1 || out->stride(1) >= topk) && (B == 1 || out->stride(0) > 0),
              "out must be addressable in place: unit stride along topk, rows that do not overlap (row stride " + num(out->stride(1)) + ")");
  }
  FA_ASSERT(!L.requires_grad(), "mla_indexer_select has no backward: logits must not require grad");
  FA_ASSERT(L.is_cuda() && (!lengths.has_value() || lengths->is_cuda()) && (!out.has_value() || out->is_cuda()),
            "logits, lengths and out must be device tensors");
  FA_ASSERT((!lengths.has_value() || lengths->device() == L.device()) && (!out.has_value() || out->device() == L.device()),
            "all tensors must be on logits' device");
  FA_ASSERT(B <= 65535 && Sq <= (1 << 20) && W <= (1 << 30), "too many sequences, rows or columns");
  c10::OptionalDeviceGuard guard(L.device());
  Tensor O = out.has_value() ? *out : torch::empty({B, Sq, topk}, L.options().dtype(at::kInt));
  const long long ls[2] = {B > 1 ? L.stride(0) : Sq * W, Sq > 1 ? L.stride(1) : W};   // a size-1 dim: a harmless stride
  const long long os[2] = {B > 1 ? O.stride(0) : Sq * topk, Sq > 1 ? O.stride(1) : topk};
  check_rc(fa_mla_indexer_select((const float*)L.data_ptr(), lengths.has_value() ? (const int*)lengths->data_ptr() : nullptr,
                                 (int*)O.data_ptr(), (int)B, (int)Sq, (int)W, (int)topk, ls, os, current_stream(L)),
           "fa_mla_indexer_select");
  return O;
}

// fa_mla_indexer_logits_fp8_prefill (include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h): q in place through its row and head
// strides when the kernel can and as a contiguous copy otherwise; weights, k, k_scale and `out` in place, never copied; ks and ke
// never read.  M == 0, and N == 0 without `out`, launch nothing.
Tensor indexer_logits_fp8_prefill(const Tensor& Q, const Tensor& Wt, const Tensor& K, const Tensor& Ks, const Tensor& lo, const Tensor& hi,
                                  const OptTensor& out) {
  FA_ASSERT(is_bytes(Q), "q must be torch.float8_e4m3fn or its uint8 view");
  FA_ASSERT(Q.dim() == 3 && Q.size(2) == 128, "q must be [M, H_i, 128] (got " + num(Q.dim()) + " dims)");
  FA_ASSERT(Q.size(1) >= 16 && Q.size(1) <= 64 && Q.size(1) % 16 == 0,
            "H_i (q.shape[1]) must be a multiple of 16 in [16, 64] (got " + num(Q.size(1)) + ")");
  const int64_t M = Q.size(0), Hi = Q.size(1);
  FA_ASSERT(M <= 1048560, "M (q.shape[0]) must be at most 1048560 (got " + num(M) + ")");
  FA_ASSERT(Wt.scalar_type() == at::kFloat && Wt.dim() == 2 && Wt.size(0) == M && Wt.size(1) == Hi, "weights must be float32 [M, H_i]");
  FA_ASSERT(is_bytes(K), "k must be torch.float8_e4m3fn or its uint8 view");
  FA_ASSERT(K.dim() == 2 && K.size(1) == 128, "k must be [N, 128]");
  const int64_t N = K.size(0);
  FA_ASSERT(N <= (1 << 30), "N (k.shape[0]) must be at most 2^30 (got " + num(N) + ")");
  FA_ASSERT(Ks.scalar_type() == at::kFloat && Ks.dim() == 1 && Ks.size(0) == N, "k_scale must be float32 [N]");
  for (const Tensor* r : {&lo, &hi})
    FA_ASSERT(r->scalar_type() == at::kInt && r->dim() == 1 && r->size(0) == M && r->is_contiguous(),
              "ks and ke must be contiguous int32 vectors of M entries");
  FA_ASSERT(K.stride(1) == 1 && (N <= 1 || (K.stride(0) >= 128 && K.stride(0) % 16 == 0 && K.stride(0) <= (1 << 24))),
            "k must be addressable in place: unit stride along the 128 bytes and a row stride that is a multiple of 16 and at least "
            "128 (got " + num(K.stride(0)) + ")");
  FA_ASSERT(N <= 1 || Ks.stride(0) >= 0, "k_scale must have a non-negative stride (got " + num(Ks.stride(0)) + ")");
  FA_ASSERT(Wt.stride(0) >= 0 && Wt.stride(1) >= 0, "weights must have non-negative strides");
  if (out.has_value()) {
    FA_ASSERT(out->scalar_type() == at::kFloat && out->dim() == 2 && out->size(0) == M && out->size(1) >= N,
              "out must be float32 [M, W] with W >= N (N = " + num(N) + ")");
    FA_ASSERT((out->size(1) <= 1 || out->stride(1) == 1) && (M <= 1 || out->stride(0) >= out->size(1)) && !out->requires_grad(),
              "out must be addressable in place (unit stride along W, rows that do not overlap) and must not require grad");
    FA_ASSERT(out->size(1) <= (1 << 30), "W (out.shape[1]) must be at most 2^30 (got " + num(out->size(1)) + ")");
  }
  FA_ASSERT(!Q.requires_grad() && !Wt.requires_grad() && !K.requires_grad() && !Ks.requires_grad(),
            "mla_indexer_logits_fp8_prefill has no backward: no input may require grad");
  FA_ASSERT(Q.is_cuda() && Wt.is_cuda() && K.is_cuda() && Ks.is_cuda() && lo.is_cuda() && hi.is_cuda() && (!out.has_value() || out->is_cuda()),
            "q, weights, k, k_scale, ks, ke and out must be device tensors");
  FA_ASSERT(Wt.device() == Q.device() && K.device() == Q.device() && Ks.device() == Q.device() && lo.device() == Q.device() &&
                hi.device() == Q.device() && (!out.has_value() || out->device() == Q.device()),
            "all tensors must be on q's device");
  FA_ASSERT(N == 0 || reinterpret_cast<uintptr_t>(K.data_ptr()) % 16 == 0, "k must be 16-byte aligned");
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out.has_value() ? *out : torch::empty({M, N}, Q.options().dtype(at::kFloat));
  const int64_t W = O.size(1);
  if (M == 0 || W == 0) return O;
  // q [M, H_i, 128] in place?  16-byte rows with unit stride along the dims, heads that do not overlap
  const bool in_place = reinterpret_cast<uintptr_t>(Q.data_ptr()) % 16 == 0 && Q.stride(2) == 1 && Q.stride(1) >= 128 &&
                        Q.stride(1) % 16 == 0 && (M == 1 || (Q.stride(0) >= 0 && Q.stride(0) % 16 == 0));
  const Tensor Qp = in_place ? Q : Q.clone(at::MemoryFormat::Contiguous);
  const long long qs[2] = {M > 1 ? Qp.stride(0) : 0, Qp.stride(1)};   // a size-1 dim: a harmless stride
  const long long ws[2] = {M > 1 ? Wt.stride(0) : 0, Wt.stride(1)};
  check_rc(fa_mla_indexer_logits_fp8_prefill(Qp.data_ptr(), (const float*)Wt.data_ptr(), N ? K.data_ptr() : nullptr,
                                             N ? (const float*)Ks.data_ptr() : nullptr, (const int*)lo.data_ptr(), (const int*)hi.data_ptr(),
                                             (float*)O.data_ptr(), (int)M, (int)Hi, (int)N, (int)W, qs, ws, N > 1 ? K.stride(0) : 128,
                                             N > 1 ? Ks.stride(0) : 1, M > 1 ? O.stride(0) : W, current_stream(Q)),
           "fa_mla_indexer_logits_fp8_prefill");
  return O;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_mla_indexer_logits_fp8 (libmi355fa.so): the DeepSeek-V3.2 indexer logits over a paged FP8 key cache";
  m.def("indexer_logits_fp8", &indexer_logits_fp8, pybind11::arg("q"), pybind11::arg("weights"), pybind11::arg("k_cache"),
        pybind11::arg("k_scale"), pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("k_new"),
        pybind11::arg("is_causal"), pybind11::arg("out"),
        "logits [B, S_q, W] = k_scale * sum_h weights * relu(q . k) over the keys block_table names, -inf where hidden, after "
        "quantising k_new in (None: no append)");
  m.def("indexer_select", &indexer_select, pybind11::arg("logits"), pybind11::arg("topk"), pybind11::arg("lengths"), pybind11::arg("out"),
        "indices [B, S_q, topk]: per row the best min(topk, #candidates) columns below lengths[b], ascending, then -1");
  m.def("indexer_logits_fp8_prefill", &indexer_logits_fp8_prefill, pybind11::arg("q"), pybind11::arg("weights"), pybind11::arg("k"),
        pybind11::arg("k_scale"), pybind11::arg("ks"), pybind11::arg("ke"), pybind11::arg("out"),
        "logits [M, W] = k_scale * sum_h weights * relu(q . k) over the keys [ks[m], ke[m]) of a contiguous k, -inf elsewhere");
}
