// Host-side binding of libmi355fa.so for PyTorch-ROCm: the launchers and the autograd function of
// My_FlashAttention_optimized.py (reference: code/My_FlashAttention_optimized.py:14-170) written against the C ABI of
// include/mi355fa.h.  PyTorch supplies device memory, the current stream and the autograd graph -- nothing else.
//
// Why this exists beside the ctypes binding (_mi355fa.py, still used by tools and by the tests that drive the C ABI
// directly): at the reference's small benchmark shapes (B=4, H=8, S=512) a fwd+bwd step is ~35 us of kernels, and a
// Python autograd.Function costs ~125 us of host time per step (Function.apply, ctx bookkeeping, the backward running
// on the autograd thread under the GIL, ctypes argument marshalling) against ~80 us for torch's own C++ SDPA.  Here the
// same sequence -- checks, torch::empty outputs, the forward or the dQ and dK/dV launches on the current stream -- runs
// without the interpreter.
//
// Every public function describes its call as a `Call` and goes through one checker, one input preparation, one
// forward_impl / backward_impl and one autograd function, as fa_api.hip funnels every C entry point into one launch.
// The score-transform calls (soft cap, ALiBi, sinks) build theirs with scored() and set their one field.  The six decode
// functions describe theirs as a `Decode` (the transform, the cache format) and go through one kvcache_impl.
//
// Built by csrc/Makefile with g++ (host code only; no device code here) into _mi355fa_torch.so next to libmi355fa.so.
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/extension.h>

#include <array>
#include <cmath>
#include <tuple>

#include "../../include/mi355fa.h"
#include "../../include/mi355fa_local.h"
#include "../../include/mi355fa_gqa.h"
#include "../../include/mi355fa_kvcache.h"
#include "../../include/mi355fa_kvcache_fp8.h"
#include "../../include/mi355fa_softcap.h"
#include "../../include/mi355fa_alibi.h"
#include "../../include/mi355fa_sink.h"
#include "torch_binding_common.h"

namespace {

using torch::autograd::AutogradContext;
using torch::autograd::tensor_list;

// a plain return code: anything but 0 fails, a HIP error's positive code included (the common check_rc, for a workspace
// function's byte count, takes negative values only)
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

// element strides {batch, head, seq} of `t` for the C ABI, written to `v`, or nullptr for a contiguous or absent tensor
// (_mi355fa.strides3)
const long long* strides3(const Tensor* t, long long* v) {
  if (!t || t->is_contiguous()) return nullptr;
  v[0] = t->size(0) > 1 ? t->stride(0) : 0;
  v[1] = t->size(1) > 1 ? t->stride(1) : 0;
  v[2] = t->size(2) > 1 ? t->stride(2) : t->size(3);
  return v;
}

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

void* current_stream(const Tensor& t) {
  return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

// One call, whichever public function it came through.  The mask is `causal`, or the window (wl, wr) when `window`
// is set; `grouped` takes the K/V head count from K; cu_q / cu_k (undefined: fixed length) with max_q / max_k pack the
// batch into [total, H, D] rows; (p, seed, offset) is the dropout triple.  The C entry point follows from it:
// grouped -> fa_*_gqa (also when H_kv == H: flash_attention_gqa always calls them), a window -> fa_*_local, otherwise
// fa_*_ex, which picks the schedule family from the table.  softcap > 0 (a grouped call): fa_*_softcap.  slopes defined
// (a grouped call): fa_*_alibi with the fp32 ALiBi slopes, (H,) or (B, H).  sinks defined (a grouped call): fa_fwd_sink with
// the fp32 attention sinks (H,), the fa_bwd_*_gqa launches and, when the sinks want a gradient, fa_bwd_dsink.  scale > 0:
// the softmax scale, 0: 1/sqrt(D).
struct Call {
  bool causal = false, window = false, grouped = false;
  int64_t wl = -1, wr = -1;
  Tensor cu_q, cu_k;
  int64_t max_q = 0, max_k = 0;
  double p = 0.0;
  int64_t seed = 0, offset = 0;
  double softcap = 0.0, scale = 0.0;
  Tensor slopes;
  Tensor sinks;

  bool varlen() const { return cu_q.defined(); }
};

Call masked(bool causal, double p, int64_t seed, int64_t offset) {
  Call c;
  c.causal = causal;
  c.p = p;
  c.seed = seed;
  c.offset = offset;
  return c;
}
Call varlen(const Tensor& cu_q, const Tensor& cu_k, int64_t max_q, int64_t max_k, bool causal, double p, int64_t seed,
            int64_t offset) {
  Call c = masked(causal, p, seed, offset);
  c.cu_q = cu_q;
  c.cu_k = cu_k;
  c.max_q = max_q;
  c.max_k = max_k;
  return c;
}
Call windowed(int64_t wl, int64_t wr) {
  Call c;
  c.window = true;
  c.wl = wl;
  c.wr = wr;
  return c;
}
// cu_seqlens None: fixed length
Call grouped(int64_t wl, int64_t wr, const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k, int64_t max_q,
             int64_t max_k) {
  FA_ASSERT(cu_q.has_value() == cu_k.has_value(), "cu_seqlens_q and cu_seqlens_k must be given together");
  Call c = windowed(wl, wr);
  c.grouped = true;
  if (cu_q.has_value()) {
    FA_ASSERT(max_q >= 1 && max_k >= 1, "varlen: max_seqlen_q and max_seqlen_k must be given (>= 1)");
    c.cu_q = *cu_q;
    c.cu_k = *cu_k;
    c.max_q = max_q;
    c.max_k = max_k;
  }
  return c;
}
// grouped() for the score-transform calls (soft cap, ALiBi, sinks): the optional softmax scale (None: 1/sqrt(D)) checked
// and stored.  The caller sets its one field -- softcap (check_softcap first), slopes or sinks; slopes and sinks are
// checked against Q in check().
Call scored(int64_t wl, int64_t wr, const c10::optional<double>& scale, const c10::optional<Tensor>& cu_q,
            const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  FA_ASSERT(!scale.has_value() || (*scale > 0.0 && std::isfinite(*scale)), "softmax_scale must be finite and > 0");
  Call c = grouped(wl, wr, cu_q, cu_k, max_q, max_k);
  c.scale = scale.has_value() ? *scale : 0.0;
  return c;
}
double check_softcap(double softcap) {
  FA_ASSERT(softcap > 0.0 && std::isfinite(softcap), "softcap must be finite and > 0");
  return softcap;
}

// ALiBi slopes of a call with B sequences of H query heads: fp32, contiguous, (H,) or (B, H), no grad (there is no
// gradient for them), on Q's device -- checked before Q's own device checks.  Their values are never read on the host.
void check_slopes(const Tensor& s, int64_t B, int64_t H, const c10::Device& dev) {
  FA_ASSERT(s.scalar_type() == at::kFloat, "alibi_slopes must be float32");
  FA_ASSERT((s.dim() == 1 && s.size(0) == H) || (s.dim() == 2 && s.size(0) == B && s.size(1) == H),
            "alibi_slopes must have shape (H,) or (B, H)");
  FA_ASSERT(s.is_contiguous(), "alibi_slopes must be contiguous");
  FA_ASSERT(!s.requires_grad(), "alibi_slopes must not require grad: there is no gradient for the slopes");
  FA_ASSERT(s.is_cuda() && s.device() == dev, "alibi_slopes must be a device tensor on q's device");
}
// the C ABI's slopes_batch_stride: 0 for (H,), H for a contiguous (B, H)
long long slopes_stride(const Tensor& s) { return s.dim() == 2 ? (long long)s.size(1) : 0; }

// Attention sinks of a call with H query heads: fp32, contiguous, (H,), on Q's device -- checked before Q's own device
// checks.  They MAY require grad (the training call returns dz for them).  Their values are never read on the host.
void check_sinks(const Tensor& s, int64_t H, const c10::Device& dev) {
  FA_ASSERT(s.defined(), "sinks must be a tensor");
  FA_ASSERT(s.scalar_type() == at::kFloat, "sinks must be float32");
  FA_ASSERT(s.dim() == 1 && s.size(0) == H, "sinks must have shape (H,)");
  FA_ASSERT(s.is_contiguous(), "sinks must be contiguous");
  FA_ASSERT(s.is_cuda() && s.device() == dev, "sinks must be a device tensor on q's device");
}

// LSE (and delta): [B, H, S_q] fp32, or [H, total_q] for packed sequences
c10::SmallVector<int64_t, 3> lse_sizes(const Call& c, const Tensor& Q) {
  if (c.varlen()) return {Q.size(1), Q.size(0)};
  return {Q.size(0), Q.size(1), Q.size(2)};
}

// The checks of every entry point, run once per call before anything is allocated: shapes first, then devices and
// dtypes.  Fixed length: Q [B, H, S_q, D], K and V [B, H_kv, S_k, D]; varlen: Q [total_q, H, D], K and V
// [total_k, H_kv, D].  H_kv == H unless the call is grouped.  `assert_head_dim`: refuse D outside {64, 128} here; the
// fixed-length launchers leave that to the C ABI (RuntimeError), as they always have.
void check(const Call& c, const Tensor& Q, const Tensor& K, const Tensor& V, bool assert_head_dim) {
  const bool vl = c.varlen();
  const int64_t nd = vl ? 3 : 4;   // the heads are dim 1 in both layouts, the head dim is the last
  FA_ASSERT(Q.dim() == nd && K.dim() == nd && V.dim() == nd,
            vl ? "varlen Q, K, V must be packed [total tokens, H, D]" : "Q, K, V must be [B, H, S, D]");
  FA_ASSERT(c.grouped || ((vl || K.size(0) == Q.size(0)) && K.size(1) == Q.size(1)),
            "K must have Q's batch and head counts (expand shared K/V heads)");
  FA_ASSERT(V.sizes() == K.sizes(), "K and V must have the same shape");
  FA_ASSERT(vl || K.size(0) == Q.size(0), "K must have Q's batch size");
  FA_ASSERT(Q.size(nd - 1) == K.size(nd - 1), "Q, K, V must share the head dim");
  FA_ASSERT(K.size(1) >= 1 && Q.size(1) % K.size(1) == 0, "Q's head count must be a multiple of K's (H % H_kv == 0)");
  if (c.window) {
    FA_ASSERT(c.wl >= -1 && c.wr >= -1, "window_left / window_right must be >= -1 (-1 = unbounded)");
    FA_ASSERT(c.wl <= INT32_MAX && c.wr <= INT32_MAX, "window_left / window_right must fit in int32");
  }
  if (vl)
    FA_ASSERT(c.cu_q.scalar_type() == at::kInt && c.cu_k.scalar_type() == at::kInt && c.cu_q.dim() == 1 &&
                  c.cu_k.dim() == 1 && c.cu_q.is_contiguous() && c.cu_k.is_contiguous() &&
                  c.cu_q.numel() == c.cu_k.numel() && c.cu_q.numel() >= 2,
              "cu_seqlens_q / cu_seqlens_k must be contiguous int32 vectors of batch + 1 entries");
  FA_ASSERT(c.p >= 0.0 && c.p < 1.0, "dropout_p must be in [0, 1)");
  if (c.slopes.defined()) check_slopes(c.slopes, vl ? c.cu_q.numel() - 1 : Q.size(0), Q.size(1), Q.device());
  if (c.sinks.defined()) check_sinks(c.sinks, Q.size(1), Q.device());
  FA_ASSERT(Q.is_cuda() && K.is_cuda() && V.is_cuda(), "Q, K, V must be device tensors");
  FA_ASSERT(Q.device() == K.device() && Q.device() == V.device(), "Q, K, V must be on the same device");
  FA_ASSERT(!vl || (c.cu_q.device() == Q.device() && c.cu_k.device() == Q.device()), "cu_seqlens must be on Q's device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "dtype must be float16 or bfloat16");
  FA_ASSERT(Q.scalar_type() == K.scalar_type() && Q.scalar_type() == V.scalar_type(), "Q, K, V must share their dtype");
  FA_ASSERT(!assert_head_dim || Q.size(nd - 1) == 64 || Q.size(nd - 1) == 128, "head dim must be 64 or 128");
}

// A tensor as the kernels will read it: packed rows for varlen, otherwise in place where the kernels can address it
// (M:138-140 copies every non-contiguous input)
Tensor prepare(const Call& c, const Tensor& t) { return c.varlen() ? contiguous16(t) : in_place(t); }   // (the varlen kernels read packed rows only)
std::array<Tensor, 3> prepare_qkv(const Call& c, const Tensor& Q, const Tensor& K, const Tensor& V) {
  Tensor K_ = prepare(c, K), V_ = prepare(c, V);
  if (!c.varlen() && K_.size(2) > 1 && K_.stride(2) != V_.stride(2)) {  // the kernels use one row stride for the K/V pair
    K_ = K_.contiguous();
    V_ = V_.contiguous();
  }
  return {prepare(c, Q), K_, V_};
}

// The sizes the C ABI takes: varlen has B = sequences and S_q / S_k = max_seqlen_q / max_seqlen_k
struct Dims {
  int B, H, Hkv, Sq, Sk, D;
  float scale;
  Dims(const Call& c, const Tensor& Q, const Tensor& K)
      : B(c.varlen() ? (int)c.cu_q.numel() - 1 : (int)Q.size(0)),
        H((int)Q.size(1)),
        Hkv((int)K.size(1)),
        Sq(c.varlen() ? (int)c.max_q : (int)Q.size(2)),
        Sk(c.varlen() ? (int)c.max_k : (int)K.size(2)),
        D((int)Q.size(-1)),
        scale(c.scale > 0.0 ? (float)c.scale : (float)(1.0 / std::sqrt((double)D))) {}
};

// mi355fa_opts of one launch: the dropout triple, the packed-sequence fields, the strides of the tensors
// {Q, K, V, O, dO, dQ, dK, dV} (nullptr: not part of the launch) and the bf16 q_scaled workspace.  `x` points into
// `st`, so the struct is built where it is used and never copied.
struct Opts {
  mi355fa_opts x{};
  long long st[8][3];
  Opts(const Call& c, const std::array<const Tensor*, 8>& t, void* q_scaled) {
    x.size = sizeof(mi355fa_opts);
    x.p_drop = (float)c.p;
    x.seed = (unsigned long long)c.seed;
    x.offset = (unsigned long long)c.offset;
    x.q_scaled = q_scaled;
    const long long** f[8] = {&x.q_strides, &x.k_strides, &x.v_strides, &x.o_strides,
                              &x.dout_strides, &x.dq_strides, &x.dk_strides, &x.dv_strides};
    for (int i = 0; i < 8; ++i) *f[i] = strides3(t[i], st[i]);   // all nullptr for varlen (packed)
    if (c.varlen()) {
      x.cu_seqlens_q = (const int*)c.cu_q.data_ptr();
      x.cu_seqlens_k = (const int*)c.cu_k.data_ptr();
      x.total_q = (int)t[0]->size(0);
      x.total_k = (int)t[1]->size(0);
    }
  }
  Opts(const Opts&) = delete;
};

int dtype_code(const Tensor& t) { return t.scalar_type() == at::kHalf ? MI355FA_FP16 : MI355FA_BF16; }

// flash_attention_forward (M:14-60): allocate O / LSE, enqueue.  Q, K, V: checked and prepared.
std::tuple<Tensor, Tensor> forward_impl(const Call& c, const Tensor& Q, const Tensor& K, const Tensor& V) {
  const Dims d(c, Q, K);
  const int dt = dtype_code(Q);
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out_like(Q);
  Tensor LSE = torch::empty(lse_sizes(c, Q), Q.options().dtype(at::kFloat));
  Opts o(c, {&Q, &K, &V, &O}, nullptr);
  const void *q = Q.data_ptr(), *k = K.data_ptr(), *v = V.data_ptr();
  float* lse = (float*)LSE.data_ptr();
  void* st = current_stream(Q);
  if (c.sinks.defined())
    check_rc(fa_fwd_sink(q, k, v, O.data_ptr(), lse, d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt, d.scale,
                         (const float*)c.sinks.data_ptr(), (int)c.wl, (int)c.wr, &o.x, st),
             "fa_fwd_sink");
  else if (c.slopes.defined())
    check_rc(fa_fwd_alibi(q, k, v, O.data_ptr(), lse, d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt, d.scale,
                          (const float*)c.slopes.data_ptr(), slopes_stride(c.slopes), (int)c.wl, (int)c.wr, &o.x, st),
             "fa_fwd_alibi");
  else if (c.softcap > 0.0)
    check_rc(fa_fwd_softcap(q, k, v, O.data_ptr(), lse, d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt, d.scale, (float)c.softcap,
                            (int)c.wl, (int)c.wr, &o.x, st),
             "fa_fwd_softcap");
  else if (c.grouped)
    check_rc(fa_fwd_gqa(q, k, v, O.data_ptr(), lse, d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt, d.scale, (int)c.wl, (int)c.wr,
                        &o.x, st),
             "fa_fwd_gqa");
  else if (c.window)
    check_rc(fa_fwd_local(q, k, v, O.data_ptr(), lse, d.B, d.H, d.Sq, d.Sk, d.D, dt, d.scale, (int)c.wl, (int)c.wr, &o.x, st),
             "fa_fwd_local");
  else
    check_rc(fa_fwd_ex(q, k, v, O.data_ptr(), lse, d.B, d.H, d.Sq, d.Sk, d.D, dt, c.causal ? 1 : 0, d.scale, &o.x, st),
             "fa_fwd_ex");
  return {O, LSE};
}

// sizes of n tensors shaped like `t`, stacked along a new first dim
c10::SmallVector<int64_t, 5> stacked(int64_t n, const Tensor& t) {
  c10::SmallVector<int64_t, 5> s{n};
  s.append(t.sizes().begin(), t.sizes().end());
  return s;
}

// flash_attention_backward (M:62-128): allocate dQ / dK / dV / delta, enqueue dQ (+delta) then dK/dV on the same stream
// (the dK/dV kernel reads the delta the dQ kernel wrote, K:376).  All inputs checked and prepared.  A call with sinks is
// the grouped call on the sink forward's O / LSE; `dsinks` != nullptr then also enqueues fa_bwd_dsink on the same delta
// and returns dz, fp32 (H,), through it.
std::tuple<Tensor, Tensor, Tensor> backward_impl(const Call& c, const Tensor& Q, const Tensor& K, const Tensor& V,
                                                 const Tensor& O, const Tensor& dO, const Tensor& LSE, Tensor* dsinks = nullptr) {
  const Dims d(c, Q, K);
  const int dt = dtype_code(Q);
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor dQ, dK, dV;
  if (!Q.is_contiguous() || !K.is_contiguous() || !V.is_contiguous()) {  // each gradient in its input's memory order
    dQ = out_like(Q);
    dK = out_like(K);
    dV = out_like(V);
  } else if (Q.sizes() == K.sizes()) {  // one allocation for the three gradients (M:71-73 makes three)
    Tensor g = torch::empty(stacked(3, Q), Q.options());
    dQ = g.select(0, 0);
    dK = g.select(0, 1);
    dV = g.select(0, 2);
  } else {  // S_q != S_k, varlen or grouped K/V: one allocation for dK and dV
    dQ = torch::empty(Q.sizes(), Q.options());
    Tensor g = torch::empty(stacked(2, K), Q.options());
    dK = g.select(0, 0);
    dV = g.select(0, 1);
  }
  // ONE scratch allocation: delta (LSE's shape, fp32) and, bf16, behind it (256-byte aligned) the Q rows the dQ launch
  // multiplied, left for the dK/dV launch (mi355fa_opts.q_scaled) -- at the small end of the reference's grid a step is
  // host-bound and every allocation is ~1 us of it (profiles/r03_small_trace.txt)
  const int64_t delta_bytes = Q.numel() / d.D * 4, qs_off = (delta_bytes + 255) & ~(int64_t)255;
  Tensor scratch = torch::empty({qs_off + (dt == MI355FA_BF16 ? Q.numel() * 2 : 0)}, Q.options().dtype(at::kByte));
  float* delta = (float*)scratch.data_ptr();
  Opts o(c, {&Q, &K, &V, &O, &dO, &dQ, &dK, &dV}, dt == MI355FA_BF16 ? (char*)scratch.data_ptr() + qs_off : nullptr);
  const void *q = Q.data_ptr(), *k = K.data_ptr(), *v = V.data_ptr(), *o_ = O.data_ptr(), *dout = dO.data_ptr();
  const float* lse = (const float*)LSE.data_ptr();
  void* st = current_stream(Q);
  if (c.slopes.defined()) {
    const float* sl = (const float*)c.slopes.data_ptr();
    const long long sbs = slopes_stride(c.slopes);
    check_rc(fa_bwd_dq_alibi(q, k, v, o_, dout, lse, dQ.data_ptr(), delta, d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt, d.scale, sl,
                             sbs, (int)c.wl, (int)c.wr, &o.x, st),
             "fa_bwd_dq_alibi");
    check_rc(fa_bwd_dkv_alibi(q, k, v, dout, lse, delta, dK.data_ptr(), dV.data_ptr(), d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt,
                              d.scale, sl, sbs, (int)c.wl, (int)c.wr, &o.x, st),
             "fa_bwd_dkv_alibi");
  } else if (c.softcap > 0.0) {
    check_rc(fa_bwd_dq_softcap(q, k, v, o_, dout, lse, dQ.data_ptr(), delta, d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt, d.scale,
                               (float)c.softcap, (int)c.wl, (int)c.wr, &o.x, st),
             "fa_bwd_dq_softcap");
    check_rc(fa_bwd_dkv_softcap(q, k, v, dout, lse, delta, dK.data_ptr(), dV.data_ptr(), d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D,
                                dt, d.scale, (float)c.softcap, (int)c.wl, (int)c.wr, &o.x, st),
             "fa_bwd_dkv_softcap");
  } else if (c.grouped) {
    check_rc(fa_bwd_dq_gqa(q, k, v, o_, dout, lse, dQ.data_ptr(), delta, d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt, d.scale,
                           (int)c.wl, (int)c.wr, &o.x, st),
             "fa_bwd_dq_gqa");
    check_rc(fa_bwd_dkv_gqa(q, k, v, dout, lse, delta, dK.data_ptr(), dV.data_ptr(), d.B, d.H, d.Hkv, d.Sq, d.Sk, d.D, dt,
                            d.scale, (int)c.wl, (int)c.wr, &o.x, st),
             "fa_bwd_dkv_gqa");
    if (c.sinks.defined() && dsinks) {
      *dsinks = torch::empty({(int64_t)d.H}, Q.options().dtype(at::kFloat));
      check_rc(fa_bwd_dsink(lse, delta, (const float*)c.sinks.data_ptr(), (float*)dsinks->data_ptr(), d.B, d.H, d.Sq, &o.x, st),
               "fa_bwd_dsink");
    }
  } else if (c.window) {
    check_rc(fa_bwd_dq_local(q, k, v, o_, dout, lse, dQ.data_ptr(), delta, d.B, d.H, d.Sq, d.Sk, d.D, dt, d.scale, (int)c.wl,
                             (int)c.wr, &o.x, st),
             "fa_bwd_dq_local");
    check_rc(fa_bwd_dkv_local(q, k, v, dout, lse, delta, dK.data_ptr(), dV.data_ptr(), d.B, d.H, d.Sq, d.Sk, d.D, dt, d.scale,
                              (int)c.wl, (int)c.wr, &o.x, st),
             "fa_bwd_dkv_local");
  } else {
    check_rc(fa_bwd_dq_ex(q, k, v, o_, dout, lse, dQ.data_ptr(), delta, d.B, d.H, d.Sq, d.Sk, d.D, dt, c.causal ? 1 : 0,
                          d.scale, &o.x, st),
             "fa_bwd_dq_ex");
    check_rc(fa_bwd_dkv_ex(q, k, v, dout, lse, delta, dK.data_ptr(), dV.data_ptr(), d.B, d.H, d.Sq, d.Sk, d.D, dt,
                           c.causal ? 1 : 0, d.scale, &o.x, st),
             "fa_bwd_dkv_ex");
  }
  return {dQ, dK, dV};
}

// The launchers, as the Python launchers call them: check, prepare, launch
std::tuple<Tensor, Tensor> launch_forward(const Call& c, const Tensor& Q, const Tensor& K, const Tensor& V) {
  check(c, Q, K, V, c.varlen() || c.grouped);
  auto in = prepare_qkv(c, Q, K, V);
  return forward_impl(c, in[0], in[1], in[2]);
}
std::tuple<Tensor, Tensor, Tensor> launch_backward(const Call& c, const Tensor& Q, const Tensor& K, const Tensor& V,
                                                   const Tensor& O, const Tensor& dO, const Tensor& LSE, Tensor* dsinks = nullptr) {
  check(c, Q, K, V, c.varlen() || c.grouped);
  FA_ASSERT(O.sizes() == Q.sizes() && dO.sizes() == Q.sizes(), "O and dO must have Q's shape");
  FA_ASSERT(O.device() == Q.device() && dO.device() == Q.device() && LSE.device() == Q.device(),
            "O, dO, LSE must be on Q's device");
  FA_ASSERT(LSE.scalar_type() == at::kFloat && LSE.is_contiguous() && LSE.sizes().equals(lse_sizes(c, Q)),
            c.varlen() ? "LSE must be contiguous float32 [H, total_q]" : "LSE must be contiguous float32 [B, H, S_q]");
  auto in = prepare_qkv(c, Q, K, V);
  return backward_impl(c, in[0], in[1], in[2], prepare(c, O), prepare(c, dO), LSE, dsinks);
}

// FlashAttentionFunction (M:130-166), for every public function.  The call's scalars go into ONE saved_data entry:
// flash_attention at small shapes is host-bound.
class FlashAttnFn : public torch::autograd::Function<FlashAttnFn> {
 public:
  // `sinks` is c.sinks (nullopt unless the call has sinks): a tensor input of its own so that autograd can hand it dz
  static Tensor forward(AutogradContext* ctx, const Tensor& Q, const Tensor& K, const Tensor& V,
                        const c10::optional<Tensor>& sinks, const Call& c) {
    check(c, Q, K, V, true);
    auto in = prepare_qkv(c, Q, K, V);
    auto out = forward_impl(c, in[0], in[1], in[2]);
    ctx->save_for_backward({in[0], in[1], in[2], std::get<0>(out), std::get<1>(out), c.cu_q, c.cu_k, c.slopes, c.sinks});
    ctx->saved_data["call"] = std::make_tuple(c.causal, c.window, c.grouped, c.wl, c.wr, c.max_q, c.max_k, c.p, c.seed,
                                              c.offset, c.softcap, c.scale);
    return std::get<0>(out);
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto s = ctx->get_saved_variables();
    const auto& e = ctx->saved_data["call"].toTupleRef().elements();
    Call c;
    c.causal = e[0].toBool();
    c.window = e[1].toBool();
    c.grouped = e[2].toBool();
    c.wl = e[3].toInt();
    c.wr = e[4].toInt();
    c.cu_q = s[5];
    c.cu_k = s[6];
    c.slopes = s[7];   // undefined unless ALiBi; no gradient flows to it (the call is not a tensor input)
    c.max_q = e[5].toInt();
    c.max_k = e[6].toInt();
    c.p = e[7].toDouble();
    c.seed = e[8].toInt();
    c.offset = e[9].toInt();
    c.softcap = e[10].toDouble();
    c.scale = e[11].toDouble();
    c.sinks = s[8];    // undefined unless the call has sinks; dz only when they require grad (input 3)
    Tensor dz;
    auto g = backward_impl(c, s[0], s[1], s[2], s[3], prepare(c, grads[0]), s[4],
                           c.sinks.defined() && ctx->needs_input_grad(3) ? &dz : nullptr);
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), dz, Tensor()};
  }
};

Tensor apply_call(const Tensor& Q, const Tensor& K, const Tensor& V, const Call& c) {
  return FlashAttnFn::apply(Q, K, V, c.sinks.defined() ? c10::optional<Tensor>(c.sinks) : c10::nullopt, c);
}

// ---- the public functions: each describes its call ---------------------------------------------------------------------
Tensor flash_attention(const Tensor& Q, const Tensor& K, const Tensor& V, bool is_causal) {
  return apply_call(Q, K, V, masked(is_causal, 0.0, 0, 0));
}
// dropout_p > 0: attention dropout with the Philox mask of (seed, offset) (include/mi355fa.h); the backward is given the
// triple the forward was given.  Inputs: contiguous or strided_ok views.
std::tuple<Tensor, Tensor> forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, bool causal, double p_drop,
                                          int64_t seed, int64_t offset) {
  return launch_forward(masked(causal, p_drop, seed, offset), Q, K, V);
}
std::tuple<Tensor, Tensor, Tensor> backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                   const Tensor& dO, const Tensor& LSE, bool causal, double p_drop,
                                                   int64_t seed, int64_t offset) {
  return launch_backward(masked(causal, p_drop, seed, offset), Q, K, V, O, dO, LSE);
}

// variable-length sequences: packed [total, H, D] tensors + cu_seqlens (include/mi355fa.h, fa_*_varlen)
Tensor flash_attention_varlen(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& cu_q, const Tensor& cu_k,
                              int64_t max_q, int64_t max_k, bool is_causal, double p_drop, int64_t seed, int64_t offset) {
  return apply_call(Q, K, V, varlen(cu_q, cu_k, max_q, max_k, is_causal, p_drop, seed, offset));
}
std::tuple<Tensor, Tensor> varlen_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& cu_q,
                                                 const Tensor& cu_k, int64_t max_q, int64_t max_k, bool causal, double p_drop,
                                                 int64_t seed, int64_t offset) {
  return launch_forward(varlen(cu_q, cu_k, max_q, max_k, causal, p_drop, seed, offset), Q, K, V);
}
std::tuple<Tensor, Tensor, Tensor> varlen_backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                          const Tensor& dO, const Tensor& LSE, const Tensor& cu_q,
                                                          const Tensor& cu_k, int64_t max_q, int64_t max_k, bool causal,
                                                          double p_drop, int64_t seed, int64_t offset) {
  return launch_backward(varlen(cu_q, cu_k, max_q, max_k, causal, p_drop, seed, offset), Q, K, V, O, dO, LSE);
}

// attention dropout (include/mi355fa.h): the plain launchers with a (p, seed, offset) triple; views read in place
Tensor flash_attention_dropout(const Tensor& Q, const Tensor& K, const Tensor& V, bool is_causal, double p_drop, int64_t seed,
                               int64_t offset) {
  return apply_call(Q, K, V, masked(is_causal, p_drop, seed, offset));
}

// sliding-window (local) attention (include/mi355fa_local.h): a window instead of `causal`
Tensor flash_attention_local(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left, int64_t window_right) {
  return apply_call(Q, K, V, windowed(window_left, window_right));
}
std::tuple<Tensor, Tensor> local_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left,
                                                int64_t window_right) {
  return launch_forward(windowed(window_left, window_right), Q, K, V);
}
std::tuple<Tensor, Tensor, Tensor> local_backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                         const Tensor& dO, const Tensor& LSE, int64_t window_left,
                                                         int64_t window_right) {
  return launch_backward(windowed(window_left, window_right), Q, K, V, O, dO, LSE);
}

// grouped-query attention (include/mi355fa_gqa.h): K / V with H_kv = H / g heads, over a window.  dK / dV come back with
// K's / V's shape, summed over each group.  The cu_seqlens arguments are checked (grouped()) before autograd sees the call.
Tensor flash_attention_gqa(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left, int64_t window_right,
                           const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k, int64_t max_q,
                           int64_t max_k) {
  return apply_call(Q, K, V, grouped(window_left, window_right, cu_q, cu_k, max_q, max_k));
}
std::tuple<Tensor, Tensor> gqa_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t window_left,
                                              int64_t window_right, const c10::optional<Tensor>& cu_q,
                                              const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  return launch_forward(grouped(window_left, window_right, cu_q, cu_k, max_q, max_k), Q, K, V);
}
std::tuple<Tensor, Tensor, Tensor> gqa_backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                       const Tensor& dO, const Tensor& LSE, int64_t window_left,
                                                       int64_t window_right, const c10::optional<Tensor>& cu_q,
                                                       const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  return launch_backward(grouped(window_left, window_right, cu_q, cu_k, max_q, max_k), Q, K, V, O, dO, LSE);
}

// logit soft-capping (include/mi355fa_softcap.h): the GQA call with every score s replaced by softcap * tanh(s * scale /
// softcap); softmax_scale None: 1/sqrt(D).  Both checked (check_softcap(), scored()) before autograd sees the call.
Tensor flash_attention_softcap(const Tensor& Q, const Tensor& K, const Tensor& V, double softcap, int64_t window_left,
                               int64_t window_right, const c10::optional<double>& softmax_scale,
                               const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k, int64_t max_q,
                               int64_t max_k) {
  check_softcap(softcap);
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.softcap = softcap;
  return apply_call(Q, K, V, c);
}
std::tuple<Tensor, Tensor> softcap_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, double softcap,
                                                  int64_t window_left, int64_t window_right,
                                                  const c10::optional<double>& softmax_scale, const c10::optional<Tensor>& cu_q,
                                                  const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  check_softcap(softcap);
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.softcap = softcap;
  return launch_forward(c, Q, K, V);
}
std::tuple<Tensor, Tensor, Tensor> softcap_backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                           const Tensor& dO, const Tensor& LSE, double softcap,
                                                           int64_t window_left, int64_t window_right,
                                                           const c10::optional<double>& softmax_scale,
                                                           const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k,
                                                           int64_t max_q, int64_t max_k) {
  check_softcap(softcap);
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.softcap = softcap;
  return launch_backward(c, Q, K, V, O, dO, LSE);
}

// ALiBi (include/mi355fa_alibi.h): the GQA call with -slope_h |i - j| added to every score; softmax_scale None: 1/sqrt(D).
// The slopes are checked (check()) before anything is launched; autograd returns no gradient for them.
Tensor flash_attention_alibi(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& slopes, int64_t window_left,
                             int64_t window_right, const c10::optional<double>& softmax_scale, const c10::optional<Tensor>& cu_q,
                             const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.slopes = slopes;
  return apply_call(Q, K, V, c);
}
std::tuple<Tensor, Tensor> alibi_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& slopes,
                                                int64_t window_left, int64_t window_right,
                                                const c10::optional<double>& softmax_scale, const c10::optional<Tensor>& cu_q,
                                                const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.slopes = slopes;
  return launch_forward(c, Q, K, V);
}
std::tuple<Tensor, Tensor, Tensor> alibi_backward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O,
                                                         const Tensor& dO, const Tensor& LSE, const Tensor& slopes,
                                                         int64_t window_left, int64_t window_right,
                                                         const c10::optional<double>& softmax_scale,
                                                         const c10::optional<Tensor>& cu_q, const c10::optional<Tensor>& cu_k,
                                                         int64_t max_q, int64_t max_k) {
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.slopes = slopes;
  return launch_backward(c, Q, K, V, O, dO, LSE);
}

// Attention sinks (include/mi355fa_sink.h): the GQA call with sinks[h] in every row's softmax denominator; softmax_scale None:
// 1/sqrt(D).  The sinks are checked (check()) before anything is launched; they get dz when they require grad.
Tensor flash_attention_sink(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& sinks, int64_t window_left,
                            int64_t window_right, const c10::optional<double>& softmax_scale, const c10::optional<Tensor>& cu_q,
                            const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.sinks = sinks;
  return apply_call(Q, K, V, c);
}
std::tuple<Tensor, Tensor> sink_forward_launch(const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& sinks,
                                               int64_t window_left, int64_t window_right,
                                               const c10::optional<double>& softmax_scale, const c10::optional<Tensor>& cu_q,
                                               const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k) {
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.sinks = sinks;
  return launch_forward(c, Q, K, V);
}
// (dQ, dK, dV, dz); need_dsinks false: fa_bwd_dsink is not launched and dz is None
std::tuple<Tensor, Tensor, Tensor, c10::optional<Tensor>> sink_backward_launch(
    const Tensor& Q, const Tensor& K, const Tensor& V, const Tensor& O, const Tensor& dO, const Tensor& LSE, const Tensor& sinks,
    int64_t window_left, int64_t window_right, const c10::optional<double>& softmax_scale, const c10::optional<Tensor>& cu_q,
    const c10::optional<Tensor>& cu_k, int64_t max_q, int64_t max_k, bool need_dsinks) {
  Call c = scored(window_left, window_right, softmax_scale, cu_q, cu_k, max_q, max_k);
  c.sinks = sinks;
  Tensor dz;
  auto g = launch_backward(c, Q, K, V, O, dO, LSE, need_dsinks ? &dz : nullptr);
  return {std::get<0>(g), std::get<1>(g), std::get<2>(g), dz.defined() ? c10::optional<Tensor>(dz) : c10::nullopt};
}

// decoding over a padded KV cache (include/mi355fa_kvcache.h, _kvcache_fp8.h): inference only, no autograd.  The caches
// are read -- and, with k_new / v_new, written -- in place; O, LSE and the split workspace come from the caching
// allocator, and nothing here synchronises or reads cache_seqlens, so a step can be captured in a graph.
//
// One decode call, whichever of the six pybind functions it came through: at most one score transform (softcap > 0,
// slopes defined, sinks defined) and the cache format.  fp8: torch.float8_e4m3fn caches with one fp32 dequantisation
// factor per (sequence, K/V head), shape (B, H_kv) or (H_kv,), None = 1; k_new / v_new (q's dtype) are quantised on the
// append.  The C entry point follows from it: fa_fwd_kvcache[_softcap | _alibi | _sink], fa_fwd_kvcache_fp8[_sink].
struct Decode {
  double softcap = 0.0;
  Tensor slopes, sinks;
  bool fp8 = false;
  c10::optional<Tensor> k_descale, v_descale;
};

// strided_ok for a cache of 1-byte elements: read in place when its strides are multiples of 16
bool fp8_strided_ok(const Tensor& t) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) return false;
  if (t.is_contiguous()) return true;
  if (t.stride(3) != 1 || t.stride(2) < t.size(3)) return false;
  if (t.size(2) > 1 && t.stride(2) % 16) return false;
  if ((t.size(2) - 1) * t.stride(2) + t.size(3) > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 2; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % 16 != 0)) return false;
  return true;
}
void check_descale(const c10::optional<Tensor>& d, const char* what, int64_t B, int64_t Hkv, const c10::Device& dev) {
  if (!d.has_value()) return;
  FA_ASSERT(d->scalar_type() == at::kFloat, (std::string(what) + " must be float32").c_str());
  FA_ASSERT((d->dim() == 1 && d->size(0) == Hkv) || (d->dim() == 2 && d->size(0) == B && d->size(1) == Hkv),
            (std::string(what) + " must have shape (B, H_kv) or (H_kv,)").c_str());
  FA_ASSERT(d->is_contiguous() && !d->requires_grad(), (std::string(what) + " must be contiguous and must not require grad").c_str());
  FA_ASSERT(d->is_cuda() && d->device() == dev, (std::string(what) + " must be a device tensor on q's device").c_str());
}

// softmax_scale <= 0: 1/sqrt(D).  The two cache formats keep their own wording where it differed (q's dtype, the
// function a "no backward" refusal names); a 16-bit cache must also have q's dtype.
std::tuple<Tensor, Tensor> kvcache_impl(const Decode& dc, const Tensor& Q, const Tensor& Kc, const Tensor& Vc,
                                        const Tensor& seqlens, const c10::optional<Tensor>& k_new,
                                        const c10::optional<Tensor>& v_new, int64_t window_left, int64_t window_right,
                                        double softmax_scale) {
  const bool fp8 = dc.fp8;
  FA_ASSERT(Q.dim() == 4 && Kc.dim() == 4 && Vc.dim() == 4, "q must be [B, H, S_q, D], the caches [B, H_kv, S_cache, D]");
  FA_ASSERT(!fp8 || (Kc.scalar_type() == at::kFloat8_e4m3fn && Vc.scalar_type() == at::kFloat8_e4m3fn),
            "k_cache and v_cache must be torch.float8_e4m3fn (OCP e4m3; fnuz, e5m2, uint8 and 16-bit caches are not accepted)");
  FA_ASSERT(Kc.sizes() == Vc.sizes(), "k_cache and v_cache must have the same shape");
  FA_ASSERT(Kc.size(0) == Q.size(0) && Kc.size(3) == Q.size(3), "the caches must have q's batch size and head dim");
  FA_ASSERT(Kc.size(1) >= 1 && Q.size(1) % Kc.size(1) == 0, "q's head count must be a multiple of the caches' (H % H_kv == 0)");
  FA_ASSERT(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  FA_ASSERT(window_left >= -1 && window_right >= -1, "window_left / window_right must be >= -1 (-1 = unbounded)");
  FA_ASSERT(window_left <= INT32_MAX && window_right <= INT32_MAX, "window_left / window_right must fit in int32");
  if (dc.slopes.defined()) check_slopes(dc.slopes, Q.size(0), Q.size(1), Q.device());
  if (dc.sinks.defined()) {
    check_sinks(dc.sinks, Q.size(1), Q.device());
    FA_ASSERT(!dc.sinks.requires_grad(), fp8 ? "flash_attention_kvcache_fp8_sink has no backward: sinks must not require grad"
                                             : "flash_attention_kvcache_sink has no backward: sinks must not require grad");
  }
  FA_ASSERT(Q.is_cuda() && Kc.is_cuda() && Vc.is_cuda() && seqlens.is_cuda(), "q, the caches and cache_seqlens must be device tensors");
  FA_ASSERT(Kc.device() == Q.device() && Vc.device() == Q.device() && seqlens.device() == Q.device(), "all tensors must be on q's device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16,
            fp8 ? "q's dtype must be float16 or bfloat16" : "dtype must be float16 or bfloat16");
  FA_ASSERT(fp8 || (Kc.scalar_type() == Q.scalar_type() && Vc.scalar_type() == Q.scalar_type()), "q and the caches must share their dtype");
  FA_ASSERT(Q.size(3) == 64 || Q.size(3) == 128 || Q.size(3) == 256,   // (the decode kernels also exist at D = 256)
            "head dim must be 64 or 128");
  FA_ASSERT(seqlens.scalar_type() == at::kInt && seqlens.dim() == 1 && seqlens.numel() == Q.size(0) && seqlens.is_contiguous(),
            "cache_seqlens must be a contiguous int32 vector of B entries");
  FA_ASSERT(!Q.requires_grad() && !Kc.requires_grad() && !Vc.requires_grad(),
            fp8 ? "flash_attention_kvcache_fp8 has no backward: q, k_cache and v_cache must not require grad"
                : "flash_attention_kvcache has no backward: q, k_cache and v_cache must not require grad");
  // fp8: one batch stride serves both descale vectors: a (H_kv,) vector beside a (B, H_kv) one is expanded
  Tensor Kd, Vd;
  long long dstride = 0;
  if (fp8) {
    check_descale(dc.k_descale, "k_descale", Kc.size(0), Kc.size(1), Q.device());
    check_descale(dc.v_descale, "v_descale", Kc.size(0), Kc.size(1), Q.device());
    if (dc.k_descale.has_value()) Kd = *dc.k_descale;
    if (dc.v_descale.has_value()) Vd = *dc.v_descale;
    if ((Kd.defined() && Kd.dim() == 2) || (Vd.defined() && Vd.dim() == 2)) {
      dstride = Kc.size(1);
      if (Kd.defined() && Kd.dim() == 1) Kd = Kd.expand({Kc.size(0), Kc.size(1)}).contiguous();
      if (Vd.defined() && Vd.dim() == 1) Vd = Vd.expand({Kc.size(0), Kc.size(1)}).contiguous();
    }
  }
  bool (*const cache_ok)(const Tensor&) = fp8 ? fp8_strided_ok : strided_ok;
  Tensor Kn, Vn;
  int S_new = 0;
  if (k_new.has_value()) {
    FA_ASSERT(k_new->dim() == 4 && k_new->sizes() == v_new->sizes() && k_new->size(0) == Kc.size(0) &&
                  k_new->size(1) == Kc.size(1) && k_new->size(3) == Kc.size(3) && k_new->size(2) >= 1,
              "k_new and v_new must be [B, H_kv, S_new, D] with S_new >= 1");
    FA_ASSERT(k_new->device() == Q.device() && v_new->device() == Q.device() && k_new->scalar_type() == Q.scalar_type() &&
                  v_new->scalar_type() == Q.scalar_type(),
              "k_new and v_new must be on q's device with q's dtype");
    // the append writes the caches themselves: they must be addressable in place
    FA_ASSERT(cache_ok(Kc) && cache_ok(Vc) && (Kc.size(2) == 1 || Kc.stride(2) == Vc.stride(2)),
              "with k_new / v_new the caches must be readable in place (16-byte rows, unit head-dim stride, one row stride)");
    Kn = contiguous16(*k_new);
    Vn = contiguous16(*v_new);
    S_new = (int)k_new->size(2);
  }
  Tensor K = cache_ok(Kc) ? Kc : Kc.clone(at::MemoryFormat::Contiguous);
  Tensor V = cache_ok(Vc) ? Vc : Vc.clone(at::MemoryFormat::Contiguous);
  if (K.size(2) > 1 && K.stride(2) != V.stride(2)) {   // one row stride for the K/V pair (only without an append)
    K = K.contiguous();
    V = V.contiguous();
  }
  Tensor Qp = in_place(Q);
  const int B = (int)Q.size(0), H = (int)Q.size(1), Hkv = (int)K.size(1), Sq = (int)Q.size(2), Sc = (int)K.size(2),
            D = (int)Q.size(3);
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)D));
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = out_like(Qp);
  Tensor LSE = torch::empty({B, H, Sq}, Q.options().dtype(at::kFloat));
  const long long ws_bytes = (fp8 ? fa_fwd_kvcache_fp8_workspace_bytes : fa_fwd_kvcache_workspace_bytes)(B, H, Hkv, Sq, Sc, S_new, D);
  check_rc(ws_bytes, fp8 ? "fa_fwd_kvcache_fp8_workspace_bytes" : "fa_fwd_kvcache_workspace_bytes");
  Tensor ws = torch::empty({std::max<long long>(ws_bytes, 1)}, Q.options().dtype(at::kByte));
  Call c;
  Opts o(c, {&Qp, &K, &V, &O}, nullptr);
  // Every entry point takes (inputs, [descales,] outputs, workspace, sizes, dtype(s), scale, <its transform's own
  // arguments>, window, opts, stream): the common arguments are spelled here, once per cache format.
  const void *q = Qp.data_ptr(), *kn = S_new ? Kn.data_ptr() : nullptr, *vn = S_new ? Vn.data_ptr() : nullptr;
  void *k = K.data_ptr(), *v = V.data_ptr();   // the append writes them
  const int* sl = (const int*)seqlens.data_ptr();
  float* lse = (float*)LSE.data_ptr();
  const int dt = dtype_code(Q), wl = (int)window_left, wr = (int)window_right;
  void* st = current_stream(Q);
  auto run = [&](const char* what, auto entry, auto... mod) {
    check_rc(entry(q, k, v, kn, vn, sl, O.data_ptr(), lse, ws.data_ptr(), ws_bytes, B, H, Hkv, Sq, Sc, S_new, D, dt, scale,
                   mod..., wl, wr, &o.x, st),
             what);
  };
  auto run_fp8 = [&](const char* what, auto entry, auto... mod) {
    check_rc(entry(q, k, v, kn, vn, sl, Kd.defined() ? (const float*)Kd.data_ptr() : nullptr,
                   Vd.defined() ? (const float*)Vd.data_ptr() : nullptr, dstride, O.data_ptr(), lse, ws.data_ptr(), ws_bytes,
                   B, H, Hkv, Sq, Sc, S_new, D, dt, MI355FA_KV_FP8_E4M3, scale, mod..., wl, wr, &o.x, st),
             what);
  };
  const float* sinks = dc.sinks.defined() ? (const float*)dc.sinks.data_ptr() : nullptr;
  if (fp8 && sinks)
    run_fp8("fa_fwd_kvcache_fp8_sink", fa_fwd_kvcache_fp8_sink, sinks);
  else if (fp8)
    run_fp8("fa_fwd_kvcache_fp8", fa_fwd_kvcache_fp8);
  else if (sinks)
    run("fa_fwd_kvcache_sink", fa_fwd_kvcache_sink, sinks);
  else if (dc.slopes.defined())
    run("fa_fwd_kvcache_alibi", fa_fwd_kvcache_alibi, (const float*)dc.slopes.data_ptr(), slopes_stride(dc.slopes));
  else if (dc.softcap > 0.0)
    run("fa_fwd_kvcache_softcap", fa_fwd_kvcache_softcap, (float)dc.softcap);
  else
    run("fa_fwd_kvcache", fa_fwd_kvcache);
  return {O, LSE};
}

// ---- the six decode functions: each describes its call ---------------------------------------------------------------
std::tuple<Tensor, Tensor> kvcache_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                           const c10::optional<Tensor>& k_new, const c10::optional<Tensor>& v_new,
                                           int64_t window_left, int64_t window_right, double softmax_scale) {
  return kvcache_impl(Decode{}, Q, Kc, Vc, seqlens, k_new, v_new, window_left, window_right, softmax_scale);
}
std::tuple<Tensor, Tensor> kvcache_softcap_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                                   double softcap, const c10::optional<Tensor>& k_new,
                                                   const c10::optional<Tensor>& v_new, int64_t window_left,
                                                   int64_t window_right, double softmax_scale) {
  Decode dc;
  dc.softcap = check_softcap(softcap);
  return kvcache_impl(dc, Q, Kc, Vc, seqlens, k_new, v_new, window_left, window_right, softmax_scale);
}
std::tuple<Tensor, Tensor> kvcache_alibi_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                                 const Tensor& slopes, const c10::optional<Tensor>& k_new,
                                                 const c10::optional<Tensor>& v_new, int64_t window_left, int64_t window_right,
                                                 double softmax_scale) {
  Decode dc;
  dc.slopes = slopes;
  return kvcache_impl(dc, Q, Kc, Vc, seqlens, k_new, v_new, window_left, window_right, softmax_scale);
}
// The two sink functions check the sinks in front of everything else, q's rank included (no head count then: -1)
Decode sink_decode(const Tensor& sinks, const Tensor& Q) {
  check_sinks(sinks, Q.dim() == 4 ? Q.size(1) : -1, Q.device());
  Decode dc;
  dc.sinks = sinks;
  return dc;
}
std::tuple<Tensor, Tensor> kvcache_sink_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                                const Tensor& sinks, const c10::optional<Tensor>& k_new,
                                                const c10::optional<Tensor>& v_new, int64_t window_left, int64_t window_right,
                                                double softmax_scale) {
  return kvcache_impl(sink_decode(sinks, Q), Q, Kc, Vc, seqlens, k_new, v_new, window_left, window_right, softmax_scale);
}
std::tuple<Tensor, Tensor> kvcache_fp8_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                               const c10::optional<Tensor>& k_descale, const c10::optional<Tensor>& v_descale,
                                               const c10::optional<Tensor>& k_new, const c10::optional<Tensor>& v_new,
                                               int64_t window_left, int64_t window_right, double softmax_scale) {
  Decode dc;
  dc.fp8 = true;
  dc.k_descale = k_descale;
  dc.v_descale = v_descale;
  return kvcache_impl(dc, Q, Kc, Vc, seqlens, k_new, v_new, window_left, window_right, softmax_scale);
}
std::tuple<Tensor, Tensor> kvcache_fp8_sink_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                                    const Tensor& sinks, const c10::optional<Tensor>& k_descale,
                                                    const c10::optional<Tensor>& v_descale, const c10::optional<Tensor>& k_new,
                                                    const c10::optional<Tensor>& v_new, int64_t window_left,
                                                    int64_t window_right, double softmax_scale) {
  Decode dc = sink_decode(sinks, Q);
  dc.fp8 = true;
  dc.k_descale = k_descale;
  dc.v_descale = v_descale;
  return kvcache_impl(dc, Q, Kc, Vc, seqlens, k_new, v_new, window_left, window_right, softmax_scale);
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
  m.def("kvcache_forward", &kvcache_forward, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("cache_seqlens"), pybind11::arg("k_new") = pybind11::none(), pybind11::arg("v_new") = pybind11::none(),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = 0.0);
  m.def("flash_attention_softcap", &flash_attention_softcap, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("softcap"), pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1,
        pybind11::arg("softmax_scale") = pybind11::none(), pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("softcap_forward_launch", &softcap_forward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("softcap"), pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1,
        pybind11::arg("softmax_scale") = pybind11::none(), pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("softcap_backward_launch", &softcap_backward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("O"), pybind11::arg("dO"), pybind11::arg("LSE"), pybind11::arg("softcap"),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = pybind11::none(),
        pybind11::arg("cu_seqlens_q") = pybind11::none(), pybind11::arg("cu_seqlens_k") = pybind11::none(),
        pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("kvcache_softcap_forward", &kvcache_softcap_forward, pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("cache_seqlens"), pybind11::arg("softcap"),
        pybind11::arg("k_new") = pybind11::none(), pybind11::arg("v_new") = pybind11::none(),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = 0.0);
  m.def("flash_attention_alibi", &flash_attention_alibi, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("alibi_slopes"), pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1,
        pybind11::arg("softmax_scale") = pybind11::none(), pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("alibi_forward_launch", &alibi_forward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("alibi_slopes"), pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1,
        pybind11::arg("softmax_scale") = pybind11::none(), pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("alibi_backward_launch", &alibi_backward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("O"), pybind11::arg("dO"), pybind11::arg("LSE"), pybind11::arg("alibi_slopes"),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = pybind11::none(),
        pybind11::arg("cu_seqlens_q") = pybind11::none(), pybind11::arg("cu_seqlens_k") = pybind11::none(),
        pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("kvcache_alibi_forward", &kvcache_alibi_forward, pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("cache_seqlens"), pybind11::arg("alibi_slopes"),
        pybind11::arg("k_new") = pybind11::none(), pybind11::arg("v_new") = pybind11::none(),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = 0.0);
  m.def("kvcache_fp8_forward", &kvcache_fp8_forward, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("cache_seqlens"), pybind11::arg("k_descale") = pybind11::none(), pybind11::arg("v_descale") = pybind11::none(),
        pybind11::arg("k_new") = pybind11::none(), pybind11::arg("v_new") = pybind11::none(),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = 0.0);
  m.def("flash_attention_sink", &flash_attention_sink, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("sinks"), pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1,
        pybind11::arg("softmax_scale") = pybind11::none(), pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("sink_forward_launch", &sink_forward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("sinks"), pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1,
        pybind11::arg("softmax_scale") = pybind11::none(), pybind11::arg("cu_seqlens_q") = pybind11::none(),
        pybind11::arg("cu_seqlens_k") = pybind11::none(), pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0);
  m.def("sink_backward_launch", &sink_backward_launch, pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"),
        pybind11::arg("O"), pybind11::arg("dO"), pybind11::arg("LSE"), pybind11::arg("sinks"),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = pybind11::none(),
        pybind11::arg("cu_seqlens_q") = pybind11::none(), pybind11::arg("cu_seqlens_k") = pybind11::none(),
        pybind11::arg("max_seqlen_q") = 0, pybind11::arg("max_seqlen_k") = 0, pybind11::arg("need_dsinks") = true);
  m.def("kvcache_sink_forward", &kvcache_sink_forward, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("cache_seqlens"), pybind11::arg("sinks"), pybind11::arg("k_new") = pybind11::none(),
        pybind11::arg("v_new") = pybind11::none(), pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1,
        pybind11::arg("softmax_scale") = 0.0);
  m.def("kvcache_fp8_sink_forward", &kvcache_fp8_sink_forward, pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("cache_seqlens"), pybind11::arg("sinks"),
        pybind11::arg("k_descale") = pybind11::none(), pybind11::arg("v_descale") = pybind11::none(),
        pybind11::arg("k_new") = pybind11::none(), pybind11::arg("v_new") = pybind11::none(),
        pybind11::arg("window_left") = -1, pybind11::arg("window_right") = -1, pybind11::arg("softmax_scale") = 0.0);
  m.def("abi_version", []() { return fa_abi_version(); });
}
