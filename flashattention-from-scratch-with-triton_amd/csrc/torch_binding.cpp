// Host-side binding of libmi355fa.so for PyTorch-ROCm: the launchers and the autograd function of
// My_FlashAttention_optimized.py (reference: code/My_FlashAttention_optimized.py:14-170) written against the C ABI of
// include/mi355fa.h.  PyTorch supplies device memory, the current stream and the autograd graph -- nothing else.
//
// Why this exists beside the ctypes binding (_mi355fa.py, still used by tools and by the tests that drive the C ABI
// directly): at the reference's small benchmark shapes (B=4, H=8, S=512) a fwd+bwd step is ~35 us of kernels, and a
// Python autograd.Function costs ~125 us of host time per step (Function.apply, ctx bookkeeping, the backward running
// on the autograd thread under the GIL, ctypes argument marshalling) against ~80 us for torch's own C++ SDPA.  Here the
// same sequence -- checks, torch::empty outputs, fa_fwd_strided / fa_bwd_dq_strided / fa_bwd_dkv_strided on the current
// stream -- runs without the interpreter.
//
// Built by csrc/Makefile with g++ (host code only; no device code here) into _mi355fa_torch.so next to libmi355fa.so.
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/extension.h>

#include <tuple>

#include "../../include/mi355fa.h"
#include "../../include/mi355fa_local.h"
#include "../../include/mi355fa_gqa.h"

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::tensor_list;

// The reference raises AssertionError on bad arguments (M:133-136); keep the exception type.
[[noreturn]] void assertion(const char* msg) {
  PyErr_SetString(PyExc_AssertionError, msg);
  throw pybind11::error_already_set();
}
#define FA_ASSERT(cond, msg) \
  do {                       \
    if (!(cond)) assertion(msg); \
  } while (0)

void check_rc(int rc, const char* what) {
  if (rc != 0) {
    std::string m = std::string(what) + " failed (code " + std::to_string(rc) + "): " + fa_last_error();
    throw std::runtime_error(m);
  }
}

// _mi355fa.strided_ok: can the kernels read `t` in place?
bool strided_ok(const Tensor& t) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) return false;
  if (t.is_contiguous()) return true;
  if (t.stride(3) != 1) return false;
  if (t.stride(2) < t.size(3)) return false;
  if (t.size(2) > 1 && t.stride(2) % 8) return false;
  if ((t.size(2) - 1) * t.stride(2) * 2 + 2 * t.size(3) > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 2; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % 8 != 0)) return false;
  return true;
}
Tensor in_place(const Tensor& t) { return strided_ok(t) ? t : t.clone(at::MemoryFormat::Contiguous); }

// element strides {batch, head, seq} for the C ABI, or nullptr for a contiguous tensor (_mi355fa.strides3)
struct Strides3 {
  long long v[3];
  const long long* ptr;
  explicit Strides3(const Tensor& t) {
    if (t.is_contiguous()) {
      ptr = nullptr;
      return;
    }
    v[0] = t.size(0) > 1 ? t.stride(0) : 0;
    v[1] = t.size(1) > 1 ? t.stride(1) : 0;
    v[2] = t.size(2) > 1 ? t.stride(2) : t.size(3);
    ptr = v;
  }
};

// Output for an input the kernels read in place: the input's own memory order (what empty_like gives a dense view --
// the reference allocates with empty_like too, M:24,71-73, but only after its .contiguous() copies), so a model that keeps
// [B, S, H, D] activations gets O and the gradients back in that order and never transposes.  Layouts the kernels cannot
// write (a broadcast stride, a head dim that does not stay innermost) get the contiguous tensor.
Tensor out_like(const Tensor& t) {
  if (!t.is_contiguous()) {
    Tensor o = at::empty_like(t);
    if (o.stride(3) == 1 && o.is_non_overlapping_and_dense() && strided_ok(o)) return o;
  }
  return torch::empty(t.sizes(), t.options());
}

int dtype_code(const Tensor& t) {
  if (t.scalar_type() == at::kHalf) return MI355FA_FP16;
  if (t.scalar_type() == at::kBFloat16) return MI355FA_BF16;
  assertion("dtype must be float16 or bfloat16");
}

void check_qkv(const Tensor& Q, const Tensor& K, const Tensor& V) {
  FA_ASSERT(Q.dim() == 4 && K.dim() == 4 && V.dim() == 4, "Q, K, V must be [B, H, S, D]");
  FA_ASSERT(K.size(0) == Q.size(0) && K.size(1) == Q.size(1),
            "K must have Q's batch and head counts (expand shared K/V heads)");
  FA_ASSERT(V.sizes() == K.sizes(), "K and V must have the same shape");
  FA_ASSERT(Q.size(3) == K.size(3), "Q, K, V must share the head dim");
  FA_ASSERT(Q.device() == K.device() && Q.device() == V.device(), "Q, K, V must be on the same device");
  FA_ASSERT(Q.scalar_type() == K.scalar_type() && Q.scalar_type() == V.scalar_type(), "Q, K, V must share their dtype");
}

void* current_stream(const Tensor& t) {
  return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

// mi355fa_opts for the general entry points (fa_*_ex): zeroed, sized, with the caller's dropout triple
mi355fa_opts make_opts(double p_drop, int64_t seed, int64_t offset) {
  FA_ASSERT(p_drop >= 0.0 && p_drop < 1.0, "dropout_p must be in [0, 1)");
  mi355fa_opts x{};
  x.size = sizeof(mi355fa_opts);
  x.p_drop = (float)p_drop;
  x.seed = (unsigned long long)seed;
  x.offset = (unsigned long long)offset;
  return x;
}

// flash_attention_forward (M:14-60): allocate O / LSE, enqueue.  Inputs: contiguous or strided_ok views, K and V sharing
// their sequence stride.  dropout_p > 0: attention dropout with the Philox mask of (seed, offset) (include/mi355fa.h).
// `win` (local_forward_launch): {window_left, window_right} of a sliding window (include/mi355fa_local.h) instead of
// `causal`; nullptr = the plain launch.
std::tuple<Tensor, Tensor> forward_impl(const Tensor& Q, const Tensor& K, const Tensor& V, bool causal, double p_drop,
                                        int64_t seed, int64_t offset, const int* win) {
  check_qkv(Q, K, V);
  FA_ASSERT(Q.is_cuda(), "Q, K, V must be device tensors");
  const int64_t B = Q.size(0), H = Q.size(1), Sq = Q.size(2), D = Q.size(3), Sk = K.size(2);
  const int dt = dtype_code(Q);
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out_like(Q);
  Tensor LSE = torch::empty({B, H, Sq}, Q.options().dtype(at::kFloat));
  Strides3 sq(Q), sk(K), sv(V), so(O);
  mi355fa_opts x = make_opts(p_drop, seed, offset);
  x.q_strides = sq.ptr;
  x.k_strides = sk.ptr;
  x.v_strides = sv.ptr;
  x.o_strides = so.ptr;
  const float scale = (float)(1.0 / std::sqrt((double)D));
  if (win)
    check_rc(fa_fwd_local(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), (float*)LSE.data_ptr(), (int)B, (int)H,
                          (int)Sq, (int)Sk, (int)D, dt, scale, win[0], win[1], &x, current_stream(Q)),
             "fa_fwd_local");
  else
    check_rc(fa_fwd_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), (float*)LSE.data_ptr(), (int)B, (int)H, (int)Sq,
                       (int)Sk, (int)D, dt, causal ? 1 : 0, scale, &x, current_stream(Q)),
             "fa_fwd");
  return {O, LSE};
}
std::tuple<Tensor, Tensor> forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, bool causal, double p_drop,
                                          int64_t seed, int64_t offset) {
  return forward_impl(Q, K, V, causal, p_drop, seed, offset, nullptr);
}

// flash_attention_backward (M:62-128): allocate dQ / dK / dV / delta, enqueue dQ (+delta) then dK/dV on the same stream
// (the dK/dV kernel reads the delta the dQ kernel wrote, K:376).  Dropout: the triple the forward was given.
// `win`: as forward_impl.
std::tuple<Tensor, Tensor, Tensor> backward_impl(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O_,
                                                 const Tensor& dO, const Tensor& LSE, bool causal, double p_drop,
                                                 int64_t seed, int64_t offset, const int* win) {
  check_qkv(Q, K, V);
  FA_ASSERT(Q.is_cuda(), "Q, K, V must be device tensors");
  FA_ASSERT(O_.sizes() == Q.sizes() && dO.sizes() == Q.sizes(), "O and dO must have Q's shape");
  FA_ASSERT(LSE.dim() == 3 && LSE.size(0) == Q.size(0) && LSE.size(1) == Q.size(1) && LSE.size(2) == Q.size(2),
            "LSE must be [B, H, S_q]");
  FA_ASSERT(O_.device() == Q.device() && dO.device() == Q.device() && LSE.device() == Q.device(),
            "O, dO, LSE must be on Q's device");
  FA_ASSERT(LSE.scalar_type() == at::kFloat && LSE.is_contiguous(), "LSE must be contiguous float32");
  const int64_t B = Q.size(0), H = Q.size(1), Sq = Q.size(2), D = Q.size(3), Sk = K.size(2);
  const int dt = dtype_code(Q);
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = in_place(O_);
  Tensor dQ, dK, dV;
  if (!Q.is_contiguous() || !K.is_contiguous() || !V.is_contiguous()) {  // each gradient in its input's memory order
    dQ = out_like(Q);
    dK = out_like(K);
    dV = out_like(V);
  } else if (Sq == Sk) {  // self-attention: one allocation for the three gradients (M:71-73 makes three)
    Tensor g = torch::empty({3, B, H, Sq, D}, Q.options());
    dQ = g.select(0, 0);
    dK = g.select(0, 1);
    dV = g.select(0, 2);
  } else {
    dQ = torch::empty({B, H, Sq, D}, Q.options());
    Tensor g = torch::empty({2, B, H, Sk, D}, Q.options());
    dK = g.select(0, 0);
    dV = g.select(0, 1);
  }
  // ONE scratch allocation: delta [B, H, S_q] fp32 and, bf16, behind it (256-byte aligned) the Q rows the dQ launch
  // multiplied, left for the dK/dV launch (mi355fa_opts.q_scaled) -- at the small end of the reference's grid a step is
  // host-bound and every allocation is ~1 us of it (profiles/r03_small_trace.txt)
  const int64_t delta_bytes = B * H * Sq * 4, qs_off = (delta_bytes + 255) & ~(int64_t)255;
  Tensor scratch = torch::empty({qs_off + (dt == MI355FA_BF16 ? B * H * Sq * D * 2 : 0)}, Q.options().dtype(at::kByte));
  float* delta = (float*)scratch.data_ptr();
  Strides3 sq(Q), sk(K), sv(V), so(O), sdo(dO), sdq(dQ), sdk(dK), sdv(dV);
  mi355fa_opts x = make_opts(p_drop, seed, offset);
  if (dt == MI355FA_BF16) x.q_scaled = (char*)scratch.data_ptr() + qs_off;
  x.q_strides = sq.ptr;
  x.k_strides = sk.ptr;
  x.v_strides = sv.ptr;
  x.o_strides = so.ptr;
  x.dout_strides = sdo.ptr;
  x.dq_strides = sdq.ptr;
  x.dk_strides = sdk.ptr;
  x.dv_strides = sdv.ptr;
  void* st = current_stream(Q);
  const float scale = (float)(1.0 / std::sqrt((double)D));
  if (win) {
    check_rc(fa_bwd_dq_local(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                             dQ.data_ptr(), delta, (int)B, (int)H, (int)Sq, (int)Sk, (int)D, dt, scale, win[0], win[1], &x, st),
             "fa_bwd_dq_local");
    check_rc(fa_bwd_dkv_local(Q.data_ptr(), K.data_ptr(), V.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                              (const float*)delta, dK.data_ptr(), dV.data_ptr(), (int)B, (int)H, (int)Sq, (int)Sk, (int)D, dt,
                              scale, win[0], win[1], &x, st),
             "fa_bwd_dkv_local");
    return {dQ, dK, dV};
  }
  check_rc(fa_bwd_dq_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                        dQ.data_ptr(), delta, (int)B, (int)H, (int)Sq, (int)Sk, (int)D, dt, causal ? 1 : 0,
                        scale, &x, st),
           "fa_bwd_dq");
  check_rc(fa_bwd_dkv_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                         (const float*)delta, dK.data_ptr(), dV.data_ptr(), (int)B, (int)H, (int)Sq, (int)Sk, (int)D,
                         dt, causal ? 1 : 0, scale, &x, st),
           "fa_bwd_dkv");
  return {dQ, dK, dV};
}
std::tuple<Tensor, Tensor, Tensor> backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O_,
                                                   const Tensor& dO, const Tensor& LSE, bool causal, double p_drop,
                                                   int64_t seed, int64_t offset) {
  return backward_impl(Q, K, V, O_, dO, LSE, causal, p_drop, seed, offset, nullptr);
}

// FlashAttentionFunction (M:130-166)
class FlashAttnFn : public torch::autograd::Function<FlashAttnFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& Q, const Tensor& K, const Tensor& V, bool is_causal) {
    FA_ASSERT(Q.is_cuda() && K.is_cuda() && V.is_cuda(), "Q, K, V must be device tensors");
    FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "dtype must be float16 or bfloat16");
    check_qkv(Q, K, V);
    FA_ASSERT(Q.size(3) == 64 || Q.size(3) == 128, "head dim must be 64 or 128");
    // no copy for views the kernels can read in place (M:138-140 copies every non-contiguous input)
    Tensor Q_ = in_place(Q), K_ = in_place(K), V_ = in_place(V);
    if (K_.size(2) > 1 && K_.stride(2) != V_.stride(2)) {  // the kernels use one row stride for the K/V pair
      K_ = K_.contiguous();
      V_ = V_.contiguous();
    }
    auto out = forward_launch(Q_, K_, V_, is_causal, 0.0, 0, 0);
    ctx->save_for_backward({Q_, K_, V_, std::get<0>(out), std::get<1>(out)});
    ctx->saved_data["is_causal"] = is_causal;
    return std::get<0>(out);
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto s = ctx->get_saved_variables();
    const bool causal = ctx->saved_data["is_causal"].toBool();
    Tensor dO = in_place(grads[0]);
    auto g = backward_launch(s[0], s[1], s[2], s[3], dO, s[4], causal, 0.0, 0, 0);
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor()};
  }
};

Tensor flash_attention(const Tensor& Q, const Tensor& K, const Tensor& V, bool is_causal) {
  return FlashAttnFn::apply(Q, K, V, is_causal);
}

// ---- variable-length sequences: packed [total, H, D] tensors + cu_seqlens (include/mi355fa.h, fa_*_varlen) ---------
void check_varlen(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& cu_q, const Tensor& cu_k) {
  FA_ASSERT(Q.dim() == 3 && K.dim() == 3 && V.dim() == 3, "varlen Q, K, V must be packed [total tokens, H, D]");
  FA_ASSERT(Q.is_cuda() && K.is_cuda() && V.is_cuda() && cu_q.is_cuda() && cu_k.is_cuda(), "varlen tensors must be device tensors");
  FA_ASSERT(K.sizes() == V.sizes(), "K and V must have the same shape");
  FA_ASSERT(Q.size(1) == K.size(1) && Q.size(2) == K.size(2), "Q, K, V must share heads and head dim");
  FA_ASSERT(Q.scalar_type() == K.scalar_type() && Q.scalar_type() == V.scalar_type(), "Q, K, V must share their dtype");
  FA_ASSERT(Q.device() == K.device() && Q.device() == V.device() && Q.device() == cu_q.device() && Q.device() == cu_k.device(),
            "all varlen tensors must be on the same device");
  FA_ASSERT(cu_q.scalar_type() == at::kInt && cu_k.scalar_type() == at::kInt && cu_q.dim() == 1 && cu_k.dim() == 1 &&
                cu_q.is_contiguous() && cu_k.is_contiguous() && cu_q.numel() == cu_k.numel() && cu_q.numel() >= 2,
            "cu_seqlens_q / cu_seqlens_k must be contiguous int32 vectors of batch + 1 entries");
  FA_ASSERT(Q.size(2) == 64 || Q.size(2) == 128, "head dim must be 64 or 128");
}
Tensor packed(const Tensor& t) {  // the varlen kernels read packed rows only: copy anything else
  return (t.is_contiguous() && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0) ? t : t.clone(at::MemoryFormat::Contiguous);
}

std::tuple<Tensor, Tensor> varlen_forward_launch(const Tensor& Q_, const Tensor& K_, const Tensor& V_, const Tensor& cu_q,
                                                 const Tensor& cu_k, int64_t max_q, int64_t max_k, bool causal, double p_drop,
                                                 int64_t seed, int64_t offset) {
  check_varlen(Q_, K_, V_, cu_q, cu_k);
  Tensor Q = packed(Q_), K = packed(K_), V = packed(V_);
  const int64_t Tq = Q.size(0), Tk = K.size(0), H = Q.size(1), D = Q.size(2), B = cu_q.numel() - 1;
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = torch::empty({Tq, H, D}, Q.options());
  Tensor LSE = torch::empty({H, Tq}, Q.options().dtype(at::kFloat));
  mi355fa_opts x = make_opts(p_drop, seed, offset);
  x.cu_seqlens_q = (const int*)cu_q.data_ptr();
  x.cu_seqlens_k = (const int*)cu_k.data_ptr();
  x.total_q = (int)Tq;
  x.total_k = (int)Tk;
  check_rc(fa_fwd_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), (float*)LSE.data_ptr(), (int)B, (int)H, (int)max_q,
                     (int)max_k, (int)D, dtype_code(Q), causal ? 1 : 0, (float)(1.0 / std::sqrt((double)D)), &x,
                     current_stream(Q)),
           "fa_fwd_varlen");
  return {O, LSE};
}

std::tuple<Tensor, Tensor, Tensor> varlen_backward_launch(const Tensor& Q_, const Tensor& K_, const Tensor& V_, const Tensor& O_,
                                                          const Tensor& dO_, const Tensor& LSE, const Tensor& cu_q,
                                                          const Tensor& cu_k, int64_t max_q, int64_t max_k, bool causal,
                                                          double p_drop, int64_t seed, int64_t offset) {
  check_varlen(Q_, K_, V_, cu_q, cu_k);
  FA_ASSERT(O_.sizes() == Q_.sizes() && dO_.sizes() == Q_.sizes(), "O and dO must have Q's shape");
  FA_ASSERT(LSE.dim() == 2 && LSE.size(0) == Q_.size(1) && LSE.size(1) == Q_.size(0) && LSE.scalar_type() == at::kFloat &&
                LSE.is_contiguous() && LSE.device() == Q_.device(),
            "LSE must be contiguous float32 [H, total_q]");
  Tensor Q = packed(Q_), K = packed(K_), V = packed(V_), O = packed(O_), dO = packed(dO_);
  const int64_t Tq = Q.size(0), Tk = K.size(0), H = Q.size(1), D = Q.size(2), B = cu_q.numel() - 1;
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor dQ = torch::empty({Tq, H, D}, Q.options());
  Tensor g = torch::empty({2, Tk, H, D}, Q.options());
  Tensor dK = g.select(0, 0), dV = g.select(0, 1);
  Tensor delta = torch::empty({H, Tq}, Q.options().dtype(at::kFloat));
  void* st = current_stream(Q);
  const float scale = (float)(1.0 / std::sqrt((double)D));
  const int dt = dtype_code(Q);
  mi355fa_opts x = make_opts(p_drop, seed, offset);
  Tensor qs;  // bf16: Q rows as the dQ launch multiplied them, for the dK/dV launch (mi355fa_opts.q_scaled)
  if (dt == MI355FA_BF16) {
    qs = torch::empty({Tq, H, D}, Q.options());
    x.q_scaled = qs.data_ptr();
  }
  x.cu_seqlens_q = (const int*)cu_q.data_ptr();
  x.cu_seqlens_k = (const int*)cu_k.data_ptr();
  x.total_q = (int)Tq;
  x.total_k = (int)Tk;
  check_rc(fa_bwd_dq_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                        dQ.data_ptr(), (float*)delta.data_ptr(), (int)B, (int)H, (int)max_q, (int)max_k, (int)D, dt,
                        causal ? 1 : 0, scale, &x, st),
           "fa_bwd_dq_varlen");
  check_rc(fa_bwd_dkv_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                         (const float*)delta.data_ptr(), dK.data_ptr(), dV.data_ptr(), (int)B, (int)H, (int)max_q, (int)max_k,
                         (int)D, dt, causal ? 1 : 0, scale, &x, st),
           "fa_bwd_dkv_varlen");
  return {dQ, dK, dV};
}

class FlashAttnVarlenFn : public torch::autograd::Function<FlashAttnVarlenFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& cu_q,
                        const Tensor& cu_k, int64_t max_q, int64_t max_k, bool is_causal, double p_drop, int64_t seed,
                        int64_t offset) {
    FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "dtype must be float16 or bfloat16");
    Tensor Q_ = packed(Q), K_ = packed(K), V_ = packed(V);
    auto out = varlen_forward_launch(Q_, K_, V_, cu_q, cu_k, max_q, max_k, is_causal, p_drop, seed, offset);
    ctx->save_for_backward({Q_, K_, V_, std::get<0>(out), std::get<1>(out), cu_q, cu_k});
    ctx->saved_data["is_causal"] = is_causal;
    ctx->saved_data["max_q"] = max_q;
    ctx->saved_data["max_k"] = max_k;
    ctx->saved_data["p"] = p_drop;
    ctx->saved_data["seed"] = seed;
    ctx->saved_data["offset"] = offset;
    return std::get<0>(out);
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto s = ctx->get_saved_variables();
    auto g = varlen_backward_launch(s[0], s[1], s[2], s[3], grads[0], s[4], s[5], s[6], ctx->saved_data["max_q"].toInt(),
                                    ctx->saved_data["max_k"].toInt(), ctx->saved_data["is_causal"].toBool(),
                                    ctx->saved_data["p"].toDouble(), ctx->saved_data["seed"].toInt(),
                                    ctx->saved_data["offset"].toInt());
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
            Tensor()};
  }
};

Tensor flash_attention_varlen(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& cu_q, const Tensor& cu_k,
                              int64_t max_q, int64_t max_k, bool is_causal, double p_drop, int64_t seed, int64_t offset) {
  return FlashAttnVarlenFn::apply(Q, K, V, cu_q, cu_k, max_q, max_k, is_causal, p_drop, seed, offset);
}

// ---- attention dropout (include/mi355fa.h): the plain launchers with a (p, seed, offset) triple; views read in place ----
class FlashAttnDropoutFn : public torch::autograd::Function<FlashAttnDropoutFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& Q, const Tensor& K, const Tensor& V, bool is_causal, double p_drop,
                        int64_t seed, int64_t offset) {
    FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "dtype must be float16 or bfloat16");
    FA_ASSERT(Q.dim() == 4 && (Q.size(3) == 64 || Q.size(3) == 128), "head dim must be 64 or 128");
    check_qkv(Q, K, V);
    Tensor Q_ = in_place(Q), K_ = in_place(K), V_ = in_place(V);
    if (K_.size(2) > 1 && K_.stride(2) != V_.stride(2)) {  // the kernels use one row stride for the K/V pair
      K_ = K_.contiguous();
      V_ = V_.contiguous();
    }
    auto out = forward_launch(Q_, K_, V_, is_causal, p_drop, seed, offset);
    ctx->save_for_backward({Q_, K_, V_, std::get<0>(out), std::get<1>(out)});
    ctx->saved_data["is_causal"] = is_causal;
    ctx->saved_data["p"] = p_drop;
    ctx->saved_data["seed"] = seed;
    ctx->saved_data["offset"] = offset;
    return std::get<0>(out);
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto s = ctx->get_saved_variables();
    auto g = backward_launch(s[0], s[1], s[2], s[3], in_place(grads[0]), s[4], ctx->saved_data["is_causal"].toBool(),
                             ctx->saved_data["p"].toDouble(), ctx->saved_data["seed"].toInt(),
                             ctx->saved_data["offset"].toInt());
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor flash_attention_dropout(const Tensor& Q, const Tensor& K, const Tensor& V, bool is_causal, double p_drop, int64_t seed,
                               int64_t offset) {
  return FlashAttnDropoutFn::apply(Q, K, V, is_causal, p_drop, seed, offset);
}

// ---- sliding-window (local) attention (include/mi355fa_local.h): the plain launchers with a window instead of `causal` ----
void check_window(int64_t window_left, int64_t window_right) {
  FA_ASSERT(window_left >= -1 && window_right >= -1, "window_left / window_right must be >= -1 (-1 = unbounded)");
  FA_ASSERT(window_left <= INT32_MAX && window_right <= INT32_MAX, "window_left / window_right must fit in int32");
}
std::tuple<Tensor, Tensor> local_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left,
                                                int64_t window_right) {
  check_window(window_left, window_right);
  const int win[2] = {(int)window_left, (int)window_right};
  return forward_impl(Q, K, V, false, 0.0, 0, 0, win);
}
std::tuple<Tensor, Tensor, Tensor> local_backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                         const Tensor& dO, const Tensor& LSE, int64_t window_left,
                                                         int64_t window_right) {
  check_window(window_left, window_right);
  const int win[2] = {(int)window_left, (int)window_right};
  return backward_impl(Q, K, V, O, dO, LSE, false, 0.0, 0, 0, win);
}

class FlashAttnLocalFn : public torch::autograd::Function<FlashAttnLocalFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left,
                        int64_t window_right) {
    FA_ASSERT(Q.is_cuda() && K.is_cuda() && V.is_cuda(), "Q, K, V must be device tensors");
    FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "dtype must be float16 or bfloat16");
    check_qkv(Q, K, V);
    FA_ASSERT(Q.size(3) == 64 || Q.size(3) == 128, "head dim must be 64 or 128");
    check_window(window_left, window_right);
    Tensor Q_ = in_place(Q), K_ = in_place(K), V_ = in_place(V);
    if (K_.size(2) > 1 && K_.stride(2) != V_.stride(2)) {  // the kernels use one row stride for the K/V pair
      K_ = K_.contiguous();
      V_ = V_.contiguous();
    }
    auto out = local_forward_launch(Q_, K_, V_, window_left, window_right);
    ctx->save_for_backward({Q_, K_, V_, std::get<0>(out), std::get<1>(out)});
    ctx->saved_data["window_left"] = window_left;
    ctx->saved_data["window_right"] = window_right;
    return std::get<0>(out);
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto s = ctx->get_saved_variables();
    auto g = local_backward_launch(s[0], s[1], s[2], s[3], in_place(grads[0]), s[4], ctx->saved_data["window_left"].toInt(),
                                   ctx->saved_data["window_right"].toInt());
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor()};
  }
};

Tensor flash_attention_local(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left, int64_t window_right) {
  return FlashAttnLocalFn::apply(Q, K, V, window_left, window_right);
}

// ---- grouped-query attention (include/mi355fa_gqa.h): K / V with H_kv = H / g heads, over a window ------------------
// Fixed length: Q [B, H, S_q, D], K and V [B, H_kv, S_k, D] (strided views read in place).  Varlen (cu_seqlens given):
// Q [total_q, H, D], K and V [total_k, H_kv, D].  dK / dV come back with K's / V's shape, summed over each group.
void check_gqa(const Tensor& Q, const Tensor& K, const Tensor& V, bool varlen) {
  const int64_t nd = varlen ? 3 : 4, hd = 1;   // dims; the heads are dim 1 in both layouts
  FA_ASSERT(Q.dim() == nd && K.dim() == nd && V.dim() == nd,
            varlen ? "varlen Q, K, V must be packed [total tokens, H, D]" : "Q, K, V must be [B, H, S, D]");
  FA_ASSERT(V.sizes() == K.sizes(), "K and V must have the same shape");
  FA_ASSERT(varlen || K.size(0) == Q.size(0), "K must have Q's batch size");
  FA_ASSERT(Q.size(nd - 1) == K.size(nd - 1), "Q, K, V must share the head dim");
  FA_ASSERT(K.size(hd) >= 1 && Q.size(hd) % K.size(hd) == 0, "Q's head count must be a multiple of K's (H % H_kv == 0)");
  FA_ASSERT(Q.is_cuda() && K.is_cuda() && V.is_cuda(), "Q, K, V must be device tensors");
  FA_ASSERT(Q.device() == K.device() && Q.device() == V.device(), "Q, K, V must be on the same device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "dtype must be float16 or bfloat16");
  FA_ASSERT(Q.scalar_type() == K.scalar_type() && Q.scalar_type() == V.scalar_type(), "Q, K, V must share their dtype");
  FA_ASSERT(Q.size(nd - 1) == 64 || Q.size(nd - 1) == 128, "head dim must be 64 or 128");
}
// cu_seqlens of a varlen GQA call, or {nullptr, nullptr}: the varlen fields of `x`
struct GqaSeq {
  const Tensor* cu_q;
  const Tensor* cu_k;
  int64_t max_q, max_k;
  bool varlen() const { return cu_q != nullptr; }
};
void set_varlen(mi355fa_opts* x, const GqaSeq& sq, const Tensor& Q, const Tensor& K) {
  FA_ASSERT(sq.cu_q->defined() && sq.cu_k->defined(), "cu_seqlens_q and cu_seqlens_k must be given together");
  const Tensor &cq = *sq.cu_q, &ck = *sq.cu_k;
  FA_ASSERT(cq.is_cuda() && ck.is_cuda() && cq.device() == Q.device() && ck.device() == Q.device(),
            "cu_seqlens must be on Q's device");
  FA_ASSERT(cq.scalar_type() == at::kInt && ck.scalar_type() == at::kInt && cq.dim() == 1 && ck.dim() == 1 &&
                cq.is_contiguous() && ck.is_contiguous() && cq.numel() == ck.numel() && cq.numel() >= 2,
            "cu_seqlens_q / cu_seqlens_k must be contiguous int32 vectors of batch + 1 entries");
  x->cu_seqlens_q = (const int*)cq.data_ptr();
  x->cu_seqlens_k = (const int*)ck.data_ptr();
  x->total_q = (int)Q.size(0);
  x->total_k = (int)K.size(0);
}

// Q, K, V as the kernels will read them: packed rows for varlen, in-place views otherwise (one row stride for K and V)
std::tuple<Tensor, Tensor, Tensor> gqa_inputs(const Tensor& Q, const Tensor& K, const Tensor& V, bool varlen) {
  if (varlen) return {packed(Q), packed(K), packed(V)};
  Tensor Q_ = in_place(Q), K_ = in_place(K), V_ = in_place(V);
  if (K_.size(2) > 1 && K_.stride(2) != V_.stride(2)) {
    K_ = K_.contiguous();
    V_ = V_.contiguous();
  }
  return {Q_, K_, V_};
}

std::tuple<Tensor, Tensor> gqa_forward_impl(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t wl, int64_t wr,
                                            const GqaSeq& sq) {
  const bool vl = sq.varlen();
  check_gqa(Q, K, V, vl);
  check_window(wl, wr);
  const int64_t H = Q.size(1), Hkv = K.size(1), D = Q.size(vl ? 2 : 3);
  const int dt = dtype_code(Q);
  c10::OptionalDeviceGuard guard(Q.device());
  mi355fa_opts x = make_opts(0.0, 0, 0);
  // varlen: packed (contiguous) tensors, so every Strides3 below is NULL, as the packed layout requires
  const Tensor O = vl ? torch::empty({Q.size(0), H, D}, Q.options()) : out_like(Q);
  const Tensor LSE = vl ? torch::empty({H, Q.size(0)}, Q.options().dtype(at::kFloat))
                        : torch::empty({Q.size(0), H, Q.size(2)}, Q.options().dtype(at::kFloat));
  Strides3 sq_(Q), sk_(K), sv_(V), so_(O);
  x.q_strides = sq_.ptr;
  x.k_strides = sk_.ptr;
  x.v_strides = sv_.ptr;
  x.o_strides = so_.ptr;
  int B = (int)Q.size(0), Sq = vl ? 0 : (int)Q.size(2), Sk = vl ? 0 : (int)K.size(2);
  if (vl) {
    set_varlen(&x, sq, Q, K);
    B = (int)sq.cu_q->numel() - 1;
    Sq = (int)sq.max_q;
    Sk = (int)sq.max_k;
  }
  check_rc(fa_fwd_gqa(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), (float*)LSE.data_ptr(), B, (int)H, (int)Hkv, Sq,
                      Sk, (int)D, dt, (float)(1.0 / std::sqrt((double)D)), (int)wl, (int)wr, &x, current_stream(Q)),
           "fa_fwd_gqa");
  return {O, LSE};
}

std::tuple<Tensor, Tensor, Tensor> gqa_backward_impl(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O_,
                                                     const Tensor& dO_, const Tensor& LSE, int64_t wl, int64_t wr,
                                                     const GqaSeq& sq) {
  const bool vl = sq.varlen();
  check_gqa(Q, K, V, vl);
  check_window(wl, wr);
  FA_ASSERT(O_.sizes() == Q.sizes() && dO_.sizes() == Q.sizes(), "O and dO must have Q's shape");
  FA_ASSERT(O_.device() == Q.device() && dO_.device() == Q.device() && LSE.device() == Q.device(),
            "O, dO, LSE must be on Q's device");
  FA_ASSERT(LSE.scalar_type() == at::kFloat && LSE.is_contiguous(), "LSE must be contiguous float32");
  const int64_t H = Q.size(1), Hkv = K.size(1), D = Q.size(vl ? 2 : 3);
  const int64_t rows = vl ? Q.size(0) : Q.size(0) * Q.size(2);   // query rows per head, summed over the batch
  FA_ASSERT(vl ? (LSE.dim() == 2 && LSE.size(0) == H && LSE.size(1) == Q.size(0))
               : (LSE.dim() == 3 && LSE.size(0) == Q.size(0) && LSE.size(1) == H && LSE.size(2) == Q.size(2)),
            vl ? "LSE must be [H, total_q]" : "LSE must be [B, H, S_q]");
  const int dt = dtype_code(Q);
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = vl ? packed(O_) : in_place(O_), dO = vl ? packed(dO_) : in_place(dO_);
  Tensor dQ, dK, dV;
  if (vl) {
    dQ = torch::empty(Q.sizes(), Q.options());
    Tensor g = torch::empty({2, K.size(0), Hkv, D}, Q.options());
    dK = g.select(0, 0);
    dV = g.select(0, 1);
  } else {
    dQ = out_like(Q);
    dK = out_like(K);
    dV = out_like(V);
  }
  // delta [H rows] fp32 and, bf16, the Q-sized q_scaled workspace behind it (256-byte aligned), as backward_impl
  const int64_t delta_bytes = H * rows * 4, qs_off = (delta_bytes + 255) & ~(int64_t)255;
  Tensor scratch = torch::empty({qs_off + (dt == MI355FA_BF16 ? H * rows * D * 2 : 0)}, Q.options().dtype(at::kByte));
  float* delta = (float*)scratch.data_ptr();
  mi355fa_opts x = make_opts(0.0, 0, 0);
  if (dt == MI355FA_BF16) x.q_scaled = (char*)scratch.data_ptr() + qs_off;
  Strides3 sq_(Q), sk_(K), sv_(V), so_(O), sdo(dO), sdq(dQ), sdk(dK), sdv(dV);   // all NULL for varlen (packed)
  x.q_strides = sq_.ptr;
  x.k_strides = sk_.ptr;
  x.v_strides = sv_.ptr;
  x.o_strides = so_.ptr;
  x.dout_strides = sdo.ptr;
  x.dq_strides = sdq.ptr;
  x.dk_strides = sdk.ptr;
  x.dv_strides = sdv.ptr;
  int B = (int)Q.size(0), Sq = vl ? 0 : (int)Q.size(2), Sk = vl ? 0 : (int)K.size(2);
  if (vl) {
    set_varlen(&x, sq, Q, K);
    B = (int)sq.cu_q->numel() - 1;
    Sq = (int)sq.max_q;
    Sk = (int)sq.max_k;
  }
  void* s = current_stream(Q);
  const float scale = (float)(1.0 / std::sqrt((double)D));
  check_rc(fa_bwd_dq_gqa(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                         dQ.data_ptr(), delta, B, (int)H, (int)Hkv, Sq, Sk, (int)D, dt, scale, (int)wl, (int)wr, &x, s),
           "fa_bwd_dq_gqa");
  check_rc(fa_bwd_dkv_gqa(Q.data_ptr(), K.data_ptr(), V.data_ptr(), dO.data_ptr(), (const float*)LSE.data_ptr(),
                          (const float*)delta, dK.data_ptr(), dV.data_ptr(), B, (int)H, (int)Hkv, Sq, Sk, (int)D, dt, scale,
                          (int)wl, (int)wr, &x, s),
           "fa_bwd_dkv_gqa");
  return {dQ, dK, dV};
}

GqaSeq gqa_seq(const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  FA_ASSERT(cu_q.has_value() == cu_k.has_value(), "cu_seqlens_q and cu_seqlens_k must be given together");
  if (!cu_q.has_value()) return GqaSeq{nullptr, nullptr, 0, 0};
  FA_ASSERT(max_q >= 1 && max_k >= 1, "varlen: max_seqlen_q and max_seqlen_k must be given (>= 1)");
  return GqaSeq{&*cu_q, &*cu_k, max_q, max_k};
}

// the launchers as the Python twin calls them (cu_seqlens None: fixed length)
std::tuple<Tensor, Tensor> gqa_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left,
                                              int64_t window_right, const c10::optional<Tensor>& cu_q,
                                              const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  return gqa_forward_impl(Q, K, V, window_left, window_right, gqa_seq(cu_q, cu_k, max_q, max_k));
}
std::tuple<Tensor, Tensor, Tensor> gqa_backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                       const Tensor& dO, const Tensor& LSE, int64_t window_left,
                                                       int64_t window_right, const c10::optional<Tensor>& cu_q,
                                                       const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  return gqa_backward_impl(Q, K, V, O, dO, LSE, window_left, window_right, gqa_seq(cu_q, cu_k, max_q, max_k));
}

class FlashAttnGqaFn : public torch::autograd::Function<FlashAttnGqaFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left,
                        int64_t window_right, const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k,
                        int64_t max_q, int64_t max_k) {
    // (cu_seqlens as optional inputs: autograd records the device of every Tensor input, an undefined one has none)
    const bool vl = cu_q.has_value();
    check_gqa(Q, K, V, vl);
    check_window(window_left, window_right);
    auto in = gqa_inputs(Q, K, V, vl);
    const GqaSeq sq = gqa_seq(cu_q, cu_k, max_q, max_k);
    auto out = gqa_forward_impl(std::get<0>(in), std::get<1>(in), std::get<2>(in), window_left, window_right, sq);
    ctx->save_for_backward({std::get<0>(in), std::get<1>(in), std::get<2>(in), std::get<0>(out), std::get<1>(out),
                            vl ? *cu_q : Tensor(), vl ? *cu_k : Tensor()});
    ctx->saved_data["window_left"] = window_left;
    ctx->saved_data["window_right"] = window_right;
    ctx->saved_data["max_q"] = max_q;
    ctx->saved_data["max_k"] = max_k;
    return std::get<0>(out);
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto s = ctx->get_saved_variables();
    const bool vl = s[5].defined();
    const GqaSeq sq = vl ? GqaSeq{&s[5], &s[6], ctx->saved_data["max_q"].toInt(), ctx->saved_data["max_k"].toInt()}
                         : GqaSeq{nullptr, nullptr, 0, 0};
    auto g = gqa_backward_impl(s[0], s[1], s[2], s[3], vl ? packed(grads[0]) : in_place(grads[0]), s[4],
                               ctx->saved_data["window_left"].toInt(), ctx->saved_data["window_right"].toInt(), sq);
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor flash_attention_gqa(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left, int64_t window_right,
                           const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k, int64_t max_q,
                           int64_t max_k) {
  gqa_seq(cu_q, cu_k, max_q, max_k);   // argument checks before autograd sees the call
  return FlashAttnGqaFn::apply(Q, K, V, window_left, window_right, cu_q, cu_k, max_q, max_k);
}

}  // namespace

PYBIND11_MODULE(_mi355fa_torch, m) {
  m.doc() = "C++ launchers and autograd function over libmi355fa.so (see My_FlashAttention_optimized.py)";
  m.def("flash_attention", &flash_attention, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("is_causal") = false);
  m.def("forward_launch", &forward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("is_causal"),
        pybind11::arg("dropout_p") = 0.0, pybind11::arg("seed") = 0, pybind11::arg("offset") = 0);
  m.def("backward_launch", &backward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("O"),
        pybind11::arg("dO"), pybind11::arg("LSE"), pybind11::arg("is_causal"), pybind11::arg("dropout_p") = 0.0,
        pybind11::arg("seed") = 0, pybind11::arg("offset") = 0);
  m.def("flash_attention_varlen", &flash_attention_varlen, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("cu_seqlens_q"), pybind11::arg("cu_seqlens_k"), pybind11::arg("max_seqlen_q"),
        pybind11::arg("max_seqlen_k"), pybind11::arg("is_causal") = false, pybind11::arg("dropout_p") = 0.0,
        pybind11::arg("seed") = 0, pybind11::arg("offset") = 0);
  m.def("varlen_forward_launch", &varlen_forward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("cu_seqlens_q"), pybind11::arg("cu_seqlens_k"), pybind11::arg("max_seqlen_q"),
        pybind11::arg("max_seqlen_k"), pybind11::arg("is_causal"), pybind11::arg("dropout_p") = 0.0, pybind11::arg("seed") = 0,
        pybind11::arg("offset") = 0);
  m.def("varlen_backward_launch", &varlen_backward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("O"), pybind11::arg("dO"), pybind11::arg("LSE"), pybind11::arg("cu_seqlens_q"),
        pybind11::arg("cu_seqlens_k"), pybind11::arg("max_seqlen_q"), pybind11::arg("max_seqlen_k"), pybind11::arg("is_causal"),
        pybind11::arg("dropout_p") = 0.0, pybind11::arg("seed") = 0, pybind11::arg("offset") = 0);
  m.def("flash_attention_dropout", &flash_attention_dropout, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("is_causal"), pybind11::arg("dropout_p"), pybind11::arg("seed"), pybind11::arg("offset") = 0);
  m.def("dropout_forward_launch", &forward_launch);    // the general launchers under their round-2 names
  m.def("dropout_backward_launch", &backward_launch);
  m.def("dropout_keep_scale", [](double p) { return (double)fa_dropout_keep_scale((float)p); });
  m.def("flash_attention_local", &flash_attention_local, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("window_left"), pybind11::arg("window_right") = 0);
  m.def("local_forward_launch", &local_forward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("window_left"), pybind11::arg("window_right") = 0);
  m.def("local_backward_launch", &local_backward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("O"), pybind11::arg("dO"), pybind11::arg("LSE"), pybind11::arg("window_left"),
        pybind11::arg("window_right") = 0);
  m.def("flash_attention_gqa", &flash_attention_gqa, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("gqa_forward_launch", &gqa_forward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("gqa_backward_launch", &gqa_backward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("O"), pybind11::arg("dO"), pybind11::arg("LSE"), pybind11::arg("window_left") = -1,
        pybind11::arg("window_right") = -1, pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("abi_version", []() { return fa_abi_version(); });
}
