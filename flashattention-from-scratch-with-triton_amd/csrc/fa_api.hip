// C ABI of libmi355fa.so (declared in include/mi355fa.h and include/mi355fa_local.h): argument checks, then enqueue.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>

#include "../../include/mi355fa.h"
#include "../../include/mi355fa_local.h"
#include "../../include/mi355fa_gqa.h"
#include "../../include/mi355fa_kvcache.h"
#include "../../include/mi355fa_softcap.h"
#include "../../include/mi355fa_alibi.h"
#include "../../include/mi355fa_kvcache_fp8.h"
#include "../../include/mi355fa_kvcache_fp4.h"
#include "../../include/mi355fa_sink.h"
#include "../../include/mi355fa_paged.h"
#include "../../include/mi355fa_ragged.h"
#include "../../include/mi355fa_ragged_fp4.h"
#include "../../include/mi355fa_kvcache_fp8_token.h"
#include "fa_decode.h"
#include "fa_kernels.h"
#include "fa_quant_softcap.h"

namespace fa {
// 0 = selection table of fa_kernels.h.  Written only by fa_debug_force_impl() (tests, A/B tools, the tuner); relaxed
// atomics so that a thread flipping them while another launches is a benign race, not undefined behaviour.
std::atomic<int> g_force_fwd{0}, g_force_dq{0}, g_force_dkv{0};
// 0 = the split formula of fa_decode.hip; written only by fa_debug_kvcache_splits() (tests, tools/decode_bench.py)
std::atomic<int> g_force_kvsplits{0};
}

namespace {

thread_local char g_err[256] = "";
void* g_dbg = nullptr;  // set by fa_debug_set_buffer(); read by -DFA_STAMPS builds only

int fail(int code, const char* fmt, const char* what) {
  snprintf(g_err, sizeof(g_err), fmt, what);
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
  return (int)e;
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// the softmax scale: finite and > 0.  The fp16 kernels keep a running MAXIMUM of the raw scores and fold the scale in
// afterwards (fa_fwd_body.inc), which is the wrong extreme for a negative scale; 0 divides by zero in their deferred
// rescale threshold; NaN / inf poison every row.  Tested on the bits: this file is built with -fno-honor-nans, under which
// a floating-point comparison may assume its operand is not NaN.
int check_scale(const char* fn, float scale) {
  uint32_t u;
  memcpy(&u, &scale, sizeof(u));
  const bool negative_or_zero = (u >> 31) != 0 || (u & 0x7fffffffu) == 0;
  const bool nan_or_inf = ((u >> 23) & 0xffu) == 0xffu;
  if (negative_or_zero || nan_or_inf) return fail(MI355FA_ERR_SHAPE, "%s: scale must be finite and > 0", fn);
  return 0;
}

// the soft cap (include/mi355fa_softcap.h): finite and > 0, tested on the bits as the scale
int check_softcap(const char* fn, float softcap) {
  uint32_t u;
  memcpy(&u, &softcap, sizeof(u));
  const bool negative_or_zero = (u >> 31) != 0 || (u & 0x7fffffffu) == 0;
  const bool nan_or_inf = ((u >> 23) & 0xffu) == 0xffu;
  if (negative_or_zero || nan_or_inf) return fail(MI355FA_ERR_SOFTCAP, "%s: softcap must be finite and > 0", fn);
  return 0;
}

// decode: the KV-cache decode calls, whose kernels also exist at D = 256 (fa_decode_body.inc); the text for any other head
// dim is the one every call gives
int check_common(const char* fn, int B, int H, int Sq, int Sk, int D, int dtype, bool decode = false) {
  if (B < 1 || H < 1 || Sq < 1 || Sk < 1) return fail(MI355FA_ERR_SHAPE, "%s: B, H, S_q, S_k must be >= 1", fn);
  if (D != 64 && D != 128 && !(decode && D == 256)) return fail(MI355FA_ERR_HEAD_DIM, "%s: head dim must be 64 or 128", fn);
  if (dtype != MI355FA_FP16 && dtype != MI355FA_BF16) return fail(MI355FA_ERR_DTYPE, "%s: dtype must be 0 (fp16) or 1 (bf16)", fn);
  // one (batch, head) slice is addressed with 32-bit buffer offsets
  const long long lim = (1ll << 31) - 1;
  if ((long long)Sq * D * 2 > lim || (long long)Sk * D * 2 > lim)
    return fail(MI355FA_ERR_SHAPE, "%s: one (batch, head) slice exceeds 2^31 bytes", fn);
  if ((long long)B * H * ((Sq > Sk ? Sq : Sk) + 127) / 128 > lim)
    return fail(MI355FA_ERR_SHAPE, "%s: too many tiles for one launch", fn);
  return 0;
}

// element strides {batch, head, seq} of a [B, H, S, D] input (NULL = contiguous) -> byte layout
// An OUTPUT (B, extent of the batch dim, given): no broadcast strides -- every (batch, head, row) must be its own memory.
int make_layout(const char* fn, const long long* st, int H, int S, int D, fa::TensorLayout* out, int out_B = 0) {
  if (!st) {
    *out = fa::contiguous_layout(H, S, D);
    return 0;
  }
  if (out_B && ((out_B > 1 && st[0] == 0) || (H > 1 && st[1] == 0)))
    return fail(MI355FA_ERR_STRIDE, "%s: an output cannot have a zero batch / head stride", fn);
  // batch / head strides may be 0 (an expanded K/V shared by several heads, MQA / GQA style); rows must not overlap
  for (int i = 0; i < 3; ++i)
    if (st[i] < 0 || (st[i] & 7) != 0)
      return fail(MI355FA_ERR_STRIDE, "%s: strides must be non-negative multiples of 8 elements", fn);
  if (st[2] < D) return fail(MI355FA_ERR_STRIDE, "%s: the sequence stride must be at least D elements", fn);
  if (((long long)S - 1) * st[2] * 2 + 2ll * D > (1ll << 31) - 1)
    return fail(MI355FA_ERR_STRIDE, "%s: one strided (batch, head) slice exceeds 2^31 bytes", fn);
  *out = fa::TensorLayout{st[0] * 2, st[1] * 2, (int)(st[2] * 2)};
  return 0;
}

// packed [total tokens, H, D] rows (varlen): no batch stride (the cu_seqlens arrays place each sequence), head stride D
fa::TensorLayout packed_layout(int H, int D) { return fa::TensorLayout{0, (long long)D * 2, H * D * 2}; }

int check_varlen(const char* fn, const int* cu_q, const int* cu_k, int batch, int H, int total_q, int total_k, int max_q,
                 int max_k, int D, int dtype) {
  if (!cu_q || !cu_k) return fail(MI355FA_ERR_NULL, "%s: NULL cu_seqlens", fn);
  // max_seqlen is an UPPER bound of the sequence lengths (it sizes the grid; a static bound above the token count is fine)
  if (total_q < 1 || total_k < 1) return fail(MI355FA_ERR_SHAPE, "%s: total tokens must be >= 1", fn);
  if (max_q < 1 || max_k < 1 || batch < 1) return fail(MI355FA_ERR_SHAPE, "%s: batch and max_seqlen must be >= 1", fn);
  // 32-bit buffer offsets are used INSIDE one sequence (rows are H*D*2 bytes apart); the packed tensors may be larger
  if ((long long)max_q * H * D * 2 > (1ll << 31) - 1 || (long long)max_k * H * D * 2 > (1ll << 31) - 1)
    return fail(MI355FA_ERR_SHAPE, "%s: one packed sequence exceeds 2^31 bytes", fn);
  return check_common(fn, batch, H, max_q, max_k, D, dtype);
}

// dropout state of a launch: p is quantised to multiples of 1/256 (include/mi355fa.h); p = 0 -> thresh 0 = plain kernels
int make_dropout(const char* fn, float p_drop, unsigned long long seed, unsigned long long offset, fa::DropoutParams* out) {
  if (!(p_drop >= 0.f) || p_drop >= 1.f) return fail(MI355FA_ERR_SHAPE, "%s: dropout probability must be in [0, 1)", fn);
  unsigned thresh = (unsigned)(p_drop * 256.f + 0.5f);
  if (thresh > 255u) thresh = 255u;
  if (p_drop > 0.f && thresh == 0u)   // never a silent "no dropout"
    return fail(MI355FA_ERR_SHAPE, "%s: dropout probability below 1/512 quantises to 0 (p is kept in 1/256 steps): pass 0 or >= 1/512", fn);
  // the Philox counter has one free 32-bit word for the offset; folding offset[63:32] into the key would make
  // (seed, offset) pairs that differ only there collide
  if (offset >> 32) return fail(MI355FA_ERR_SHAPE, "%s: the dropout offset must be below 2^32", fn);
  out->thresh = thresh;
  out->seed_lo = (unsigned)seed;
  out->seed_hi = (unsigned)(seed >> 32);
  out->offset = (unsigned)offset;
  out->rp = 256.f / (256.f - (float)thresh);
  return 0;
}

}  // namespace

// (fa_debug_poison below)  One wave per SIMD, every register of the wave written, the workgroup's LDS filled.
__global__ __launch_bounds__(256, 1) void fa_poison_kernel() {
  extern __shared__ __attribute__((aligned(16))) char poison_smem[];
  const unsigned nan2 = 0x7FC07FC0u;
  for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) ((unsigned*)poison_smem)[i] = nan2;
#define FA_P4(n) "v_mov_b32 v" #n ", %0\n\tv_accvgpr_write_b32 a" #n ", %0\n\t"
#define FA_P16(a, b, c, d) FA_P4(a) FA_P4(b) FA_P4(c) FA_P4(d)
  // v8 .. v255 and a0 .. a255 (v0 .. v7 stay with the compiler: the loop above and the kernel's few addresses)
  asm volatile(
      FA_P16(8, 9, 10, 11) FA_P16(12, 13, 14, 15) FA_P16(16, 17, 18, 19) FA_P16(20, 21, 22, 23) FA_P16(24, 25, 26, 27) FA_P16(28, 29, 30, 31)
      FA_P16(32, 33, 34, 35) FA_P16(36, 37, 38, 39) FA_P16(40, 41, 42, 43) FA_P16(44, 45, 46, 47) FA_P16(48, 49, 50, 51) FA_P16(52, 53, 54, 55)
      FA_P16(56, 57, 58, 59) FA_P16(60, 61, 62, 63) FA_P16(64, 65, 66, 67) FA_P16(68, 69, 70, 71) FA_P16(72, 73, 74, 75) FA_P16(76, 77, 78, 79)
      FA_P16(80, 81, 82, 83) FA_P16(84, 85, 86, 87) FA_P16(88, 89, 90, 91) FA_P16(92, 93, 94, 95) FA_P16(96, 97, 98, 99) FA_P16(100, 101, 102, 103)
      FA_P16(104, 105, 106, 107) FA_P16(108, 109, 110, 111) FA_P16(112, 113, 114, 115) FA_P16(116, 117, 118, 119) FA_P16(120, 121, 122, 123)
      FA_P16(124, 125, 126, 127) FA_P16(128, 129, 130, 131) FA_P16(132, 133, 134, 135) FA_P16(136, 137, 138, 139) FA_P16(140, 141, 142, 143)
      FA_P16(144, 145, 146, 147) FA_P16(148, 149, 150, 151) FA_P16(152, 153, 154, 155) FA_P16(156, 157, 158, 159) FA_P16(160, 161, 162, 163)
      FA_P16(164, 165, 166, 167) FA_P16(168, 169, 170, 171) FA_P16(172, 173, 174, 175) FA_P16(176, 177, 178, 179) FA_P16(180, 181, 182, 183)
      FA_P16(184, 185, 186, 187) FA_P16(188, 189, 190, 191) FA_P16(192, 193, 194, 195) FA_P16(196, 197, 198, 199) FA_P16(200, 201, 202, 203)
      FA_P16(204, 205, 206, 207) FA_P16(208, 209, 210, 211) FA_P16(212, 213, 214, 215) FA_P16(216, 217, 218, 219) FA_P16(220, 221, 222, 223)
      FA_P16(224, 225, 226, 227) FA_P16(228, 229, 230, 231) FA_P16(232, 233, 234, 235) FA_P16(236, 237, 238, 239) FA_P16(240, 241, 242, 243)
      FA_P16(244, 245, 246, 247) FA_P16(248, 249, 250, 251) FA_P16(252, 253, 254, 255)
      "v_accvgpr_write_b32 a0, %0\n\tv_accvgpr_write_b32 a1, %0\n\tv_accvgpr_write_b32 a2, %0\n\tv_accvgpr_write_b32 a3, %0\n\t"
      "v_accvgpr_write_b32 a4, %0\n\tv_accvgpr_write_b32 a5, %0\n\tv_accvgpr_write_b32 a6, %0\n\tv_accvgpr_write_b32 a7, %0"
      :: "v"(nan2)
      : "memory"
#define FA_C(n) , "v" #n, "a" #n
#define FA_C8(n) FA_C(n##0) FA_C(n##1) FA_C(n##2) FA_C(n##3) FA_C(n##4) FA_C(n##5) FA_C(n##6) FA_C(n##7) FA_C(n##8) FA_C(n##9)
        , "v8", "v9", "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9"
        FA_C8(1) FA_C8(2) FA_C8(3) FA_C8(4) FA_C8(5) FA_C8(6) FA_C8(7) FA_C8(8) FA_C8(9) FA_C8(10) FA_C8(11) FA_C8(12) FA_C8(13) FA_C8(14)
        FA_C8(15) FA_C8(16) FA_C8(17) FA_C8(18) FA_C8(19) FA_C8(20) FA_C8(21) FA_C8(22) FA_C8(23) FA_C8(24)
        FA_C(250) FA_C(251) FA_C(252) FA_C(253) FA_C(254) FA_C(255));
#undef FA_C8
#undef FA_C
#undef FA_P16
#undef FA_P4
  __syncthreads();
}

extern "C" {

int fa_abi_version(void) { return MI355FA_ABI_VERSION; }

// Not part of the public header: pin the schedule family per kernel (0 = automatic rule); tests and A/B tools.
void fa_debug_force_impl(int fwd, int dq, int dkv) {
  fa::g_force_fwd.store(fwd, std::memory_order_relaxed);
  fa::g_force_dq.store(dq, std::memory_order_relaxed);
  fa::g_force_dkv.store(dkv, std::memory_order_relaxed);
}

// Not part of the public header: which schedule family a contiguous launch of this shape takes (kernel 0 = forward,
// 1 = dQ, 2 = dK/dV), after the generated table (fa_table.h), the validity fallbacks and any forced override.
int fa_debug_pick(int kernel, int D, int dtype, int causal, int B, int H, int S_q, int S_k) {
  if (kernel == 0) return fa::pick_fwd_impl(fa::g_force_fwd, D, dtype, B, H, S_q, S_k, causal != 0, true);
  if (kernel == 1) return fa::pick_dq_impl(fa::g_force_dq, D, dtype, B, H, S_q, S_k, causal != 0);
  return fa::pick_dkv_impl(fa::g_force_dkv, D, dtype, B, H, S_q, S_k, causal != 0);
}

// Not part of the public header: the family launch_fwd / launch_bwd_dq / launch_bwd_dkv take for any launch -- fa_debug_pick
// plus a packed batch (varlen; S_q / S_k = the longest sequences) and dropout.  `contiguous` is accepted and ignored: no
// family's choice depends on views any more, and the argument stays because callers bind this function with 11 ints.
int fa_debug_pick_ex(int kernel, int D, int dtype, int causal, int B, int H, int S_q, int S_k, int varlen, int contiguous,
                     int dropout) {
  (void)contiguous;
  if (kernel == 0) return fa::fwd_family(D, dtype, B, H, S_q, S_k, causal != 0, varlen != 0, dropout != 0);
  if (kernel == 1) return fa::dq_family(D, dtype, B, H, S_q, S_k, causal != 0, varlen != 0, dropout != 0);
  return fa::dkv_family(D, dtype, B, H, S_q, S_k, causal != 0, varlen != 0, dropout != 0);
}

// Not part of the public header: the work-list division of the persistent kernels (fa_kernels.h FastDiv) evaluated on the
// host exactly as the device evaluates it -- multiplier and shift from make_fastdiv(d), quotient = (mulhi(m, n) + n) >> l --
// so that a CPU test can sweep it against n / d.
int fa_debug_fastdiv(int n, int d) {
  const fa::FastDiv f = fa::make_fastdiv(d);
  const unsigned hi = (unsigned)(((unsigned long long)f.m * (unsigned)n) >> 32);
  return (int)((hi + (unsigned)n) >> f.l);
}

// Not part of the public header: diagnostic hook used by tools/stamps*.py with -DFA_STAMPS builds; in the product library the
// family-4 forward counts, in the buffer's first word, the passes that took their exact second attempt (tests).
void fa_debug_set_buffer(void* p) { g_dbg = p; }

// Not part of the public header: fill every CU's LDS (160 KiB) and every vector / accumulator register a workgroup of the
// family-4 kernels can own with NaN patterns (0x7FC07FC0: a NaN as fp32, as two bf16 and as two fp16).  Tests and
// tools/race_check.py launch it between kernels: a kernel that reads LDS or a register it has not written -- a missing
// wait on an LDS-DMA piece, an accumulator that is not zeroed -- otherwise finds what the PREVIOUS launch left there,
// which in a test that repeats one launch is exactly the right data.
int fa_debug_poison(void* stream) {
  return (int)fa::launch_kernel<fa_poison_kernel>(2048, 256, 160 * 1024, (hipStream_t)stream);
}

// Not part of the public header: pin the split count of fa_fwd_kvcache (and of fa_fwd_kvcache_workspace_bytes) to n;
// 0 = the formula (fa_decode.hip kvcache_splits).  Tests and tools/decode_bench.py.
void fa_debug_kvcache_splits(int n) { fa::g_force_kvsplits.store(n > 0 ? n : 0, std::memory_order_relaxed); }

const char* fa_last_error(void) { return g_err; }

int fa_supported(int D, int dtype) {
  return (D == 64 || D == 128) && (dtype == MI355FA_FP16 || dtype == MI355FA_BF16);
}

// ---- the one implementation: every public entry point below fills an mi355fa_opts and lands here -------------------
// `fn` = the public name, for the error text.  Fixed-length: [B, H, S, D] tensors, optional per-tensor strides.  Varlen
// (opts->cu_seqlens_q != NULL): packed [total, H, D] tensors, B = batch, S_q / S_k = max_seqlen_q / max_seqlen_k.
// Dropout (opts->p_drop > 0) composes with both.  `win` (fa_kernels.h ScoreMod; every entry point but the plain, _ex and
// dropout ones): the sliding window and the score transforms on top of it, launched through launch_*_mod; NULL = the
// plain / causal kernels.  The sink backward launches are the _gqa ones.
// the attention sinks (include/mi355fa_sink.h): a 4-byte aligned device pointer to H floats.  The values are never read here.
static int check_sinks(const char* fn, const float* sinks) {
  if (!sinks) return fail(MI355FA_ERR_NULL, "%s: sinks is NULL", fn);
  if (reinterpret_cast<uintptr_t>(sinks) & 3u) return fail(MI355FA_ERR_ALIGN, "%s: sinks must be 4-byte aligned", fn);
  return 0;
}

// the ALiBi slopes (include/mi355fa_alibi.h): a 4-byte aligned device pointer, stride 0 (H,) or >= H (B, H), every index
// b * stride + h inside int (the kernels index with int).  The values are never read here.
static int check_alibi(const char* fn, const float* slopes, long long stride, int B, int H) {
  if (!slopes) return fail(MI355FA_ERR_NULL, "%s: alibi_slopes is NULL", fn);
  if (reinterpret_cast<uintptr_t>(slopes) & 3u) return fail(MI355FA_ERR_ALIGN, "%s: alibi_slopes must be 4-byte aligned", fn);
  if (stride < 0 || (stride > 0 && stride < (long long)H))
    return fail(MI355FA_ERR_ALIBI, "%s: slopes_batch_stride must be 0 (shape (H,)) or >= H (shape (B, H))", fn);
  if (stride > 0 && (long long)(B > 1 ? B - 1 : 0) * stride + H > 0x7fffffffLL)
    return fail(MI355FA_ERR_ALIBI, "%s: slopes_batch_stride too large: (B - 1) * stride + H must stay below 2^31", fn);
  return 0;
}

// H / H_kv of a GQA call (checked before the window and everything else)
static int make_group(const char* fn, int H, int H_kv, fa::ScoreMod* w) {
  if (H_kv < 1 || (H >= 1 && H % H_kv != 0))
    return fail(MI355FA_ERR_GROUP, "%s: H_kv must be >= 1 and divide H", fn);
  w->group = H >= 1 ? H / H_kv : 1;   // H < 1 is refused with the other shape checks
  return 0;
}
// heads of K, V, dK and dV
static int kv_heads(int H, const fa::ScoreMod* win) { return (win && win->group) ? H / win->group : H; }

// window_left / window_right as the caller gives them (-1 = unbounded) -> the kernels' form
static int make_window(const char* fn, int left, int right, fa::ScoreMod* w) {
  if (left < -1 || right < -1) return fail(MI355FA_ERR_WINDOW, "%s: window_left / window_right must be >= -1", fn);
  // sequences are below 2^24 rows (one slice is below 2^31 bytes): 2^30 is unbounded and keeps i +- w inside int
  w->wl = (left < 0 || left > fa::kWindowUnbounded) ? fa::kWindowUnbounded : left;
  w->wr = (right < 0 || right > fa::kWindowUnbounded) ? fa::kWindowUnbounded : right;
  return 0;
}

static int refuse_window_dropout(const char* fn, const fa::ScoreMod* win, const mi355fa_opts& x) {
  if (win && x.p_drop != 0.f)
    return fail(MI355FA_ERR_SHAPE, win->softcap > 0.f ? "%s: dropout is not supported with softcap"
                                   : win->slopes    ? "%s: dropout is not supported with ALiBi"
                                   : win->sinks     ? "%s: dropout is not supported with attention sinks"
                                   : win->group     ? "%s: dropout is not supported with grouped-query attention"
                                                    : "%s: dropout is not supported with a sliding window", fn);
  return 0;
}

static int read_opts(const char* fn, const mi355fa_opts* in, mi355fa_opts* o) {
  *o = mi355fa_opts{};
  if (!in) return 0;
  if (in->size != sizeof(mi355fa_opts))
    return fail(MI355FA_ERR_SHAPE, "%s: mi355fa_opts.size does not match this library (set it to sizeof(mi355fa_opts))", fn);
  *o = *in;
  if ((o->cu_seqlens_q == nullptr) != (o->cu_seqlens_k == nullptr))
    return fail(MI355FA_ERR_NULL, "%s: cu_seqlens_q and cu_seqlens_k must be given together", fn);
  if (o->cu_seqlens_q && (o->q_strides || o->k_strides || o->v_strides || o->o_strides || o->dout_strides || o->dq_strides ||
                          o->dk_strides || o->dv_strides))
    return fail(MI355FA_ERR_STRIDE, "%s: packed variable-length tensors take no strides", fn);
  return 0;
}

static int fwd_impl(const char* fn, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int S_q,
                    int S_k, int D, int dtype, int causal, float scale, const mi355fa_opts* opts, void* stream,
                    const fa::ScoreMod* win = nullptr) {
  if (!q || !k || !v || !o || !lse) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if (int rc = check_scale(fn, scale)) return rc;
  mi355fa_opts x;
  if (int rc = read_opts(fn, opts, &x)) return rc;
  if (x.cu_seqlens_q) {
    if (int rc = check_varlen(fn, x.cu_seqlens_q, x.cu_seqlens_k, B, H, x.total_q, x.total_k, S_q, S_k, D, dtype)) return rc;
  } else if (int rc = check_common(fn, B, H, S_q, S_k, D, dtype)) {
    return rc;
  }
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(o) || misaligned(lse))
    return fail(MI355FA_ERR_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  fa::FwdParams p{q, k, v, o, lse, B, H, S_q, S_k, scale, 0, g_dbg, 0};
  const int Hk = kv_heads(H, win);
  if (x.cu_seqlens_q) {
    p.lq = p.lo = packed_layout(H, D);
    p.lk = p.lv = packed_layout(Hk, D);
    p.lse_sb = 0;
    p.lse_sh = x.total_q;
    p.vl = fa::VarLen{x.cu_seqlens_q, x.cu_seqlens_k};
  } else {
    if (int rc = make_layout(fn, x.q_strides, H, S_q, D, &p.lq)) return rc;
    if (int rc = make_layout(fn, x.k_strides, Hk, S_k, D, &p.lk)) return rc;
    if (int rc = make_layout(fn, x.v_strides, Hk, S_k, D, &p.lv)) return rc;
    if (p.lk.rs != p.lv.rs) return fail(MI355FA_ERR_STRIDE, "%s: K and V must share their sequence stride", fn);
    if (int rc = make_layout(fn, x.o_strides, H, S_q, D, &p.lo, B)) return rc;
    p.lse_sb = (long long)H * S_q;
    p.lse_sh = S_q;
  }
  if (int rc = make_dropout(fn, x.p_drop, x.seed, x.offset, &p.drop)) return rc;
  if (int rc = refuse_window_dropout(fn, win, x)) return rc;
  hipError_t e = win ? fa::launch_fwd_mod(p, D, dtype, *win, (hipStream_t)stream)
                     : fa::launch_fwd(p, D, dtype, causal != 0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, fn);
  return 0;
}

// the layouts, sequence table and dropout state shared by the two backward launches
// (Hk: heads of K, V, dK and dV -- H except for grouped-query attention)
static int bwd_fill(const char* fn, fa::BwdParams* p, const mi355fa_opts& x, int B, int H, int S_q, int S_k, int D, int dtype,
                    int Hk) {
  if (x.cu_seqlens_q) {
    if (int rc = check_varlen(fn, x.cu_seqlens_q, x.cu_seqlens_k, B, H, x.total_q, x.total_k, S_q, S_k, D, dtype)) return rc;
    p->lq = p->ldo = p->lo = p->ldq = packed_layout(H, D);
    p->lk = p->lv = p->ldk = p->ldv = packed_layout(Hk, D);
    p->lse_sb = 0;
    p->lse_sh = x.total_q;
    p->vl = fa::VarLen{x.cu_seqlens_q, x.cu_seqlens_k};
  } else {
    if (int rc = check_common(fn, B, H, S_q, S_k, D, dtype)) return rc;
    if (int rc = make_layout(fn, x.q_strides, H, S_q, D, &p->lq)) return rc;
    if (int rc = make_layout(fn, x.k_strides, Hk, S_k, D, &p->lk)) return rc;
    if (int rc = make_layout(fn, x.v_strides, Hk, S_k, D, &p->lv)) return rc;
    if (int rc = make_layout(fn, x.dout_strides, H, S_q, D, &p->ldo)) return rc;
    if (p->lk.rs != p->lv.rs) return fail(MI355FA_ERR_STRIDE, "%s: K and V must share their sequence stride", fn);
    if (int rc = make_layout(fn, x.o_strides, H, S_q, D, &p->lo)) return rc;
    if (int rc = make_layout(fn, x.dq_strides, H, S_q, D, &p->ldq, B)) return rc;
    if (int rc = make_layout(fn, x.dk_strides, Hk, S_k, D, &p->ldk, B)) return rc;
    if (int rc = make_layout(fn, x.dv_strides, Hk, S_k, D, &p->ldv, B)) return rc;
    p->lse_sb = (long long)H * S_q;
    p->lse_sh = S_q;
  }
  return make_dropout(fn, x.p_drop, x.seed, x.offset, &p->drop);
}

static int dq_impl(const char* fn, const void* q, const void* k, const void* v, const void* o, const void* dout,
                   const float* lse, void* dq, float* delta, int B, int H, int S_q, int S_k, int D, int dtype, int causal,
                   float scale, const mi355fa_opts* opts, void* stream, const fa::ScoreMod* win = nullptr) {
  if (!q || !k || !v || !o || !dout || !lse || !dq || !delta) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if (int rc = check_scale(fn, scale)) return rc;
  mi355fa_opts x;
  if (int rc = read_opts(fn, opts, &x)) return rc;
  fa::BwdParams p{q, k, v, o, dout, lse, delta, dq, nullptr, nullptr, B, H, S_q, S_k, scale, 0, g_dbg, 0};
  if (int rc = bwd_fill(fn, &p, x, B, H, S_q, S_k, D, dtype, kv_heads(H, win))) return rc;
  if (int rc = refuse_window_dropout(fn, win, x)) return rc;
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(o) || misaligned(dout) || misaligned(lse) ||
      misaligned(dq) || misaligned(delta) || misaligned(x.q_scaled))
    return fail(MI355FA_ERR_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  if (x.q_scaled && dtype == MI355FA_BF16) {  // workspace the dK/dV launch will read instead of Q (fa_kernels.h BwdParams::qs)
    p.qs = x.q_scaled;
    p.lqs = x.cu_seqlens_q ? packed_layout(H, D) : fa::contiguous_layout(H, S_q, D);
  }
  hipError_t e = win ? fa::launch_bwd_dq_mod(p, D, dtype, *win, (hipStream_t)stream)
                     : fa::launch_bwd_dq(p, D, dtype, causal != 0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, fn);
  return 0;
}

static int dkv_impl(const char* fn, const void* q, const void* k, const void* v, const void* dout, const float* lse,
                    const float* delta, void* dk, void* dv, int B, int H, int S_q, int S_k, int D, int dtype, int causal,
                    float scale, const mi355fa_opts* opts, void* stream, const fa::ScoreMod* win = nullptr) {
  if (!q || !k || !v || !dout || !lse || !delta || !dk || !dv) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if (int rc = check_scale(fn, scale)) return rc;
  mi355fa_opts x;
  if (int rc = read_opts(fn, opts, &x)) return rc;
  fa::BwdParams p{q, k, v, nullptr, dout, lse, const_cast<float*>(delta), nullptr, dk, dv, B, H, S_q, S_k, scale, 0, g_dbg, 0};
  if (int rc = bwd_fill(fn, &p, x, B, H, S_q, S_k, D, dtype, kv_heads(H, win))) return rc;
  if (int rc = refuse_window_dropout(fn, win, x)) return rc;
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(dout) || misaligned(lse) || misaligned(delta) ||
      misaligned(dk) || misaligned(dv) || misaligned(x.q_scaled))
    return fail(MI355FA_ERR_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  if (x.q_scaled && dtype == MI355FA_BF16) {  // the rows the dQ launch wrote: Q * scale * log2e as the forward rounded it
    p.q = x.q_scaled;
    p.lq = x.cu_seqlens_q ? packed_layout(H, D) : fa::contiguous_layout(H, S_q, D);
    p.q_prescaled = 1;
  }
  hipError_t e = win ? fa::launch_bwd_dkv_mod(p, D, dtype, *win, (hipStream_t)stream)
                     : fa::launch_bwd_dkv(p, D, dtype, causal != 0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, fn);
  return 0;
}

static mi355fa_opts base_opts() {
  mi355fa_opts x{};
  x.size = sizeof(mi355fa_opts);
  return x;
}

// ---- general, composable entry points ------------------------------------------------------------------------------
int fa_fwd_ex(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int S_q, int S_k, int D,
              int dtype, int causal, float scale, const mi355fa_opts* opts, void* stream) {
  return fwd_impl("fa_fwd_ex", q, k, v, o, lse, B, H, S_q, S_k, D, dtype, causal, scale, opts, stream);
}
int fa_bwd_dq_ex(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                 float* delta, int B, int H, int S_q, int S_k, int D, int dtype, int causal, float scale,
                 const mi355fa_opts* opts, void* stream) {
  return dq_impl("fa_bwd_dq_ex", q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, causal, scale, opts, stream);
}
int fa_bwd_dkv_ex(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                  void* dk, void* dv, int B, int H, int S_q, int S_k, int D, int dtype, int causal, float scale,
                  const mi355fa_opts* opts, void* stream) {
  return dkv_impl("fa_bwd_dkv_ex", q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, causal, scale, opts, stream);
}

// ---- the reference's three launches (contiguous [B, H, S, D]) ------------------------------------------------------
int fa_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int S_q, int S_k, int D,
           int dtype, int causal, float scale, void* stream) {
  return fwd_impl("fa_fwd", q, k, v, o, lse, B, H, S_q, S_k, D, dtype, causal, scale, nullptr, stream);
}
int fa_bwd_dq(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
              float* delta, int B, int H, int S_q, int S_k, int D, int dtype, int causal, float scale, void* stream) {
  return dq_impl("fa_bwd_dq", q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, causal, scale, nullptr, stream);
}
int fa_bwd_dkv(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
               void* dk, void* dv, int B, int H, int S_q, int S_k, int D, int dtype, int causal, float scale,
               void* stream) {
  return dkv_impl("fa_bwd_dkv", q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, causal, scale, nullptr, stream);
}

// ---- strided tensors ------------------------------------------------------------------------------------------------
int fa_fwd_strided(const void* q, const long long* q_strides, const void* k, const long long* k_strides, const void* v,
                   const long long* v_strides, void* o, const long long* o_strides, float* lse, int B, int H, int S_q,
                   int S_k, int D, int dtype, int causal, float scale, void* stream) {
  mi355fa_opts x = base_opts();
  x.q_strides = q_strides;
  x.k_strides = k_strides;
  x.v_strides = v_strides;
  x.o_strides = o_strides;
  return fwd_impl("fa_fwd", q, k, v, o, lse, B, H, S_q, S_k, D, dtype, causal, scale, &x, stream);
}
int fa_bwd_dq_strided(const void* q, const long long* q_strides, const void* k, const long long* k_strides,
                      const void* v, const long long* v_strides, const void* o, const long long* o_strides,
                      const void* dout, const long long* dout_strides, const float* lse, void* dq,
                      const long long* dq_strides, float* delta, int B, int H, int S_q, int S_k, int D, int dtype,
                      int causal, float scale, void* stream) {
  mi355fa_opts x = base_opts();
  x.q_strides = q_strides;
  x.k_strides = k_strides;
  x.v_strides = v_strides;
  x.o_strides = o_strides;
  x.dout_strides = dout_strides;
  x.dq_strides = dq_strides;
  return dq_impl("fa_bwd_dq", q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, causal, scale, &x, stream);
}
int fa_bwd_dkv_strided(const void* q, const long long* q_strides, const void* k, const long long* k_strides,
                       const void* v, const long long* v_strides, const void* dout, const long long* dout_strides,
                       const float* lse, const float* delta, void* dk, const long long* dk_strides, void* dv,
                       const long long* dv_strides, int B, int H, int S_q, int S_k, int D, int dtype, int causal,
                       float scale, void* stream) {
  mi355fa_opts x = base_opts();
  x.q_strides = q_strides;
  x.k_strides = k_strides;
  x.v_strides = v_strides;
  x.dout_strides = dout_strides;
  x.dk_strides = dk_strides;
  x.dv_strides = dv_strides;
  return dkv_impl("fa_bwd_dkv", q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, causal, scale, &x, stream);
}

// ---- variable-length ("varlen"): packed [total, H, D] tensors + cu_seqlens (include/mi355fa.h) ------------------------
static mi355fa_opts varlen_opts(const int* cu_q, const int* cu_k, int total_q, int total_k) {
  mi355fa_opts x = base_opts();
  x.cu_seqlens_q = cu_q;
  x.cu_seqlens_k = cu_k;
  x.total_q = total_q;
  x.total_k = total_k;
  return x;
}
int fa_fwd_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const int* cu_seqlens_q,
                  const int* cu_seqlens_k, int batch, int H, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k,
                  int D, int dtype, int causal, float scale, void* stream) {
  if (!cu_seqlens_q || !cu_seqlens_k) return fail(MI355FA_ERR_NULL, "%s: NULL cu_seqlens", "fa_fwd_varlen");
  const mi355fa_opts x = varlen_opts(cu_seqlens_q, cu_seqlens_k, total_q, total_k);
  return fwd_impl("fa_fwd_varlen", q, k, v, o, lse, batch, H, max_seqlen_q, max_seqlen_k, D, dtype, causal, scale, &x, stream);
}
int fa_bwd_dq_varlen(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                     float* delta, const int* cu_seqlens_q, const int* cu_seqlens_k, int batch, int H, int total_q,
                     int total_k, int max_seqlen_q, int max_seqlen_k, int D, int dtype, int causal, float scale,
                     void* stream) {
  if (!cu_seqlens_q || !cu_seqlens_k) return fail(MI355FA_ERR_NULL, "%s: NULL cu_seqlens", "fa_bwd_dq_varlen");
  const mi355fa_opts x = varlen_opts(cu_seqlens_q, cu_seqlens_k, total_q, total_k);
  return dq_impl("fa_bwd_dq_varlen", q, k, v, o, dout, lse, dq, delta, batch, H, max_seqlen_q, max_seqlen_k, D, dtype, causal,
                 scale, &x, stream);
}
int fa_bwd_dkv_varlen(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                      void* dk, void* dv, const int* cu_seqlens_q, const int* cu_seqlens_k, int batch, int H, int total_q,
                      int total_k, int max_seqlen_q, int max_seqlen_k, int D, int dtype, int causal, float scale,
                      void* stream) {
  if (!cu_seqlens_q || !cu_seqlens_k) return fail(MI355FA_ERR_NULL, "%s: NULL cu_seqlens", "fa_bwd_dkv_varlen");
  const mi355fa_opts x = varlen_opts(cu_seqlens_q, cu_seqlens_k, total_q, total_k);
  return dkv_impl("fa_bwd_dkv_varlen", q, k, v, dout, lse, delta, dk, dv, batch, H, max_seqlen_q, max_seqlen_k, D, dtype,
                  causal, scale, &x, stream);
}

// ---- attention dropout (include/mi355fa.h): contiguous [B, H, S, D] tensors as fa_fwd / fa_bwd_* ----------------------
float fa_dropout_keep_scale(float p_drop) {   // 1 / (1 - p) for the quantised p the kernels use
  fa::DropoutParams d;
  if (make_dropout("fa_dropout_keep_scale", p_drop, 0, 0, &d)) return 0.f;
  return d.rp;
}
static mi355fa_opts dropout_opts(float p_drop, unsigned long long seed, unsigned long long offset) {
  mi355fa_opts x = base_opts();
  x.p_drop = p_drop;
  x.seed = seed;
  x.offset = offset;
  return x;
}
int fa_fwd_dropout(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int S_q, int S_k, int D,
                   int dtype, int causal, float scale, float p_drop, unsigned long long seed, unsigned long long offset,
                   void* stream) {
  const mi355fa_opts x = dropout_opts(p_drop, seed, offset);
  return fwd_impl("fa_fwd_dropout", q, k, v, o, lse, B, H, S_q, S_k, D, dtype, causal, scale, &x, stream);
}
int fa_bwd_dq_dropout(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                      float* delta, int B, int H, int S_q, int S_k, int D, int dtype, int causal, float scale, float p_drop,
                      unsigned long long seed, unsigned long long offset, void* stream) {
  const mi355fa_opts x = dropout_opts(p_drop, seed, offset);
  return dq_impl("fa_bwd_dq_dropout", q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, causal, scale, &x, stream);
}
int fa_bwd_dkv_dropout(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                       void* dk, void* dv, int B, int H, int S_q, int S_k, int D, int dtype, int causal, float scale,
                       float p_drop, unsigned long long seed, unsigned long long offset, void* stream) {
  const mi355fa_opts x = dropout_opts(p_drop, seed, offset);
  return dkv_impl("fa_bwd_dkv_dropout", q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, causal, scale, &x, stream);
}

// ---- sliding-window (local) attention (include/mi355fa_local.h): the _ex forms with a window instead of `causal` ---------
int fa_fwd_local(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int S_q, int S_k, int D,
                 int dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  fa::ScoreMod w;
  if (int rc = make_window("fa_fwd_local", window_left, window_right, &w)) return rc;
  return fwd_impl("fa_fwd_local", q, k, v, o, lse, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dq_local(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    void* dq, float* delta, int B, int H, int S_q, int S_k, int D, int dtype, float scale, int window_left,
                    int window_right, const mi355fa_opts* opts, void* stream) {
  fa::ScoreMod w;
  if (int rc = make_window("fa_bwd_dq_local", window_left, window_right, &w)) return rc;
  return dq_impl("fa_bwd_dq_local", q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dkv_local(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                     void* dk, void* dv, int B, int H, int S_q, int S_k, int D, int dtype, float scale, int window_left,
                     int window_right, const mi355fa_opts* opts, void* stream) {
  fa::ScoreMod w;
  if (int rc = make_window("fa_bwd_dkv_local", window_left, window_right, &w)) return rc;
  return dkv_impl("fa_bwd_dkv_local", q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}

// ---- grouped-query attention (include/mi355fa_gqa.h): the _local forms with H_kv K/V heads ---------------------------
int fa_fwd_gqa(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q, int S_k,
               int D, int dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  fa::ScoreMod w;
  if (int rc = make_group("fa_fwd_gqa", H, H_kv, &w)) return rc;
  if (int rc = make_window("fa_fwd_gqa", window_left, window_right, &w)) return rc;
  return fwd_impl("fa_fwd_gqa", q, k, v, o, lse, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dq_gqa(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                  float* delta, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale, int window_left,
                  int window_right, const mi355fa_opts* opts, void* stream) {
  fa::ScoreMod w;
  if (int rc = make_group("fa_bwd_dq_gqa", H, H_kv, &w)) return rc;
  if (int rc = make_window("fa_bwd_dq_gqa", window_left, window_right, &w)) return rc;
  return dq_impl("fa_bwd_dq_gqa", q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dkv_gqa(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                   void* dk, void* dv, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                   int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  fa::ScoreMod w;
  if (int rc = make_group("fa_bwd_dkv_gqa", H, H_kv, &w)) return rc;
  if (int rc = make_window("fa_bwd_dkv_gqa", window_left, window_right, &w)) return rc;
  return dkv_impl("fa_bwd_dkv_gqa", q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}

// ---- decoding attention over a padded KV cache (include/mi355fa_kvcache.h) ------------------------------------------
// The shape checks shared by fa_fwd_kvcache and fa_fwd_kvcache_workspace_bytes; *nsplit = the launch's split count.
// (fmt: the cache format, whose split rule it is)
static int kvcache_shape(const char* fn, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype,
                         fa::KvFormat fmt, int* nsplit) {
  fa::ScoreMod w;
  if (int rc = make_group(fn, H, H_kv, &w)) return rc;
  if (S_new < 0) return fail(MI355FA_ERR_SHAPE, "%s: S_new must be >= 0", fn);
  if (int rc = check_common(fn, B, H, S_q, S_cache, D, dtype, true)) return rc;
  if ((long long)H * S_q > (1 << 24) || (long long)B * H * S_q * D > (1ll << 40))
    return fail(MI355FA_ERR_SHAPE, "%s: too many query rows for one launch", fn);
  const int forced = fa::g_force_kvsplits.load(std::memory_order_relaxed);
  *nsplit = fa::kvcache_splits((long long)B * H_kv * fa::decode_row_blocks(w.group, S_q), S_cache, D, fmt, forced);
  if ((long long)B * H_kv * ((long long)w.group * S_q + 31) / 32 * *nsplit > (1ll << 31) - 1)
    return fail(MI355FA_ERR_SHAPE, "%s: too many workgroups for one launch", fn);
  return 0;
}

// FP8 caches (include/mi355fa_kvcache_fp8.h): the dequantisation factors of a call, and the byte layout of a cache of
// 1-byte elements (strides in elements = bytes, multiples of 16: every row starts on a 16-byte boundary)
struct KvFp8 {
  const float *k_descale, *v_descale;
  long long bstride;
};
// The byte layout of a [.., H, S, rowb] tensor of bytes -- an e4m3 or MXFP4 cache, or a scale tensor -- from its byte strides
// {batch | page, head, row} (NULL = contiguous): multiples of `gran`, the row stride at least the row.  bad_gran / bad_row:
// the tensor's own words for the two refusals.
static int make_layout_bytes(const char* fn, const long long* st, int H, int S, int rowb, int gran, const char* bad_gran,
                             const char* bad_row, fa::TensorLayout* out) {
  if (!st) {
    *out = fa::TensorLayout{(long long)H * S * rowb, (long long)S * rowb, rowb};
    return 0;
  }
  for (int i = 0; i < 3; ++i)
    if (st[i] < 0 || st[i] % gran != 0) return fail(MI355FA_ERR_STRIDE, bad_gran, fn);
  if (st[2] < rowb) return fail(MI355FA_ERR_STRIDE, bad_row, fn);
  if (((long long)S - 1) * st[2] + rowb > (1ll << 31) - 1)
    return fail(MI355FA_ERR_STRIDE, "%s: one strided (batch, head) slice exceeds 2^31 bytes", fn);
  *out = fa::TensorLayout{st[0], st[1], (int)st[2]};
  return 0;
}
static int make_layout_fp8(const char* fn, const long long* st, int H, int S, int D, fa::TensorLayout* out) {
  return make_layout_bytes(fn, st, H, S, D, 16, "%s: fp8 cache strides must be non-negative multiples of 16 elements (bytes)",
                           "%s: the sequence stride must be at least D elements", out);
}

// MXFP4 caches (include/mi355fa_kvcache_fp4.h): the scale tensors of a call and their byte strides (NULL = contiguous), and
// the byte layout of a cache (rowb = D / 2, strides multiples of 16) or of a scale tensor (rowb = D / 32, multiples of it).
struct KvFp4 {
  void *k_scale, *v_scale;
  const long long *k_scale_strides, *v_scale_strides;
};
static int make_layout_fp4(const char* fn, bool scales, const long long* st, int H, int S, int D, fa::TensorLayout* out) {
  return scales ? make_layout_bytes(fn, st, H, S, D / 32, D / 32,
                                    "%s: the scale strides must be non-negative multiples of D / 32 bytes",
                                    "%s: the scale row stride must be at least D / 32 bytes", out)
                : make_layout_bytes(fn, st, H, S, D / 2, 16, "%s: the MXFP4 cache strides must be non-negative multiples of 16 bytes",
                                    "%s: the MXFP4 cache row stride must be at least D / 2 bytes", out);
}

// Per-token-scaled e4m3 caches (include/mi355fa_kvcache_fp8_token.h): the fp32 row scales of a call and their ELEMENT strides
// {batch | page, head, row} (NULL = contiguous [.., H, S]), any non-negative ones, -> the byte layout the kernels take.
struct KvFp8Token {
  float *k_scale, *v_scale;
  const long long *k_scale_strides, *v_scale_strides;
};
// (the refusals of these calls carry the offending value: texts of their own, beside the recorded ones of the older calls)
static int fail_value(int code, const char* fmt, const char* fn, long long value) {
  snprintf(g_err, sizeof(g_err), fmt, fn, value);
  return code;
}
static int make_layout_token_scales(const char* fn, const long long* st, int H, int S, fa::TensorLayout* out) {
  if (!st) {
    *out = fa::TensorLayout{(long long)H * S * 4, (long long)S * 4, 4};
    return 0;
  }
  for (int i = 0; i < 3; ++i)
    if (st[i] < 0 || st[i] > (1ll << 40))
      return fail_value(MI355FA_ERR_STRIDE, "%s: the scale strides must be non-negative element strides (got %lld)", fn, st[i]);
  if (((long long)S - 1) * st[2] * 4 + 4 > (1ll << 31) - 1)
    return fail_value(MI355FA_ERR_STRIDE, "%s: one strided (batch, head) slice of the scales exceeds 2^31 bytes (row stride %lld elements)",
                      fn, st[2]);
  *out = fa::TensorLayout{st[0] * 4, st[1] * 4, (int)(st[2] * 4)};
  return 0;
}

// A paged cache (include/mi355fa_paged.h), its own arguments already checked (check_paged): S_cache of the call is
// max_pages * page_size, the caches are the pools and their strides {page, head, row}.
struct KvPaged {
  const int* table;
  long long stride;
  int num_pages, page_size, max_pages;
};

// Packed variable-length queries (include/mi355fa_ragged.h): q / o are [total_q, H, D], S_q of the call is unused, and S_new
// is 1 with k_new / v_new (every query row brings its key) and 0 without.
struct KvRagged {
  const int* cu;
  int total_q;
};
// q_strides / o_strides of a packed call, {ignored, head, row} in elements (NULL = contiguous), -> the byte layout
static int make_layout_ragged(const char* fn, const long long* st, int H, int D, bool output, fa::TensorLayout* out) {
  if (!st) {
    *out = fa::TensorLayout{0, (long long)D * 2, H * D * 2};
    return 0;
  }
  if (st[1] < 0 || st[2] < D || (st[1] & 7) != 0 || (st[2] & 7) != 0 || st[2] * 2 > 0x7fffffffLL || st[1] * 2 > 0x7fffffffLL ||
      (output && H > 1 && st[1] == 0))
    return fail(MI355FA_ERR_RAGGED,
                "%s: the head and row strides of packed q / o must be multiples of 8 elements (16-byte rows), the row stride at "
                "least D, both below 2^30, and an output's head stride non-zero", fn);
  *out = fa::TensorLayout{0, st[1] * 2, (int)(st[2] * 2)};
  return 0;
}
// The shape checks shared by fa_fwd_kvcache_ragged and its workspace function; *nsplit = the launch's split count, *nb_max
// the bound on the step's 32-row blocks the grid is sized by.
static int ragged_shape(const char* fn, int total_q, int B, int H, int H_kv, int S_cache, int D, int dtype,
                        fa::KvFormat fmt, int* nsplit, long long* nb_max) {
  fa::ScoreMod w;
  if (int rc = make_group(fn, H, H_kv, &w)) return rc;
  if (total_q < 1 || B < 1) return fail(MI355FA_ERR_RAGGED, "%s: total_q and B must be >= 1", fn);
  if (int rc = check_common(fn, B, H, total_q, S_cache, D, dtype, true)) return rc;
  if ((long long)H * total_q > (1 << 24) || B > (1 << 24))
    return fail(MI355FA_ERR_RAGGED, "%s: too many query rows or sequences for one launch (H * total_q and B are at most 2^24)", fn);
  *nb_max = fa::ragged_nb_max(w.group, total_q, B);
  *nsplit = fa::kvcache_splits(*nb_max * H_kv, S_cache, D, fmt, fa::g_force_kvsplits.load(std::memory_order_relaxed));
  if (*nb_max * H_kv * *nsplit > (1ll << 31) - 1) return fail(MI355FA_ERR_SHAPE, "%s: too many workgroups for one launch", fn);
  return 0;
}
// The launch a shape comes to: its split count, (packed queries) the bound on its row blocks, and the bytes of its
// workspace -- the plan of a packed step at the head, the partials behind it.
struct KvWork {
  int nsplit = 1;
  long long nb_max = 0, ws_bytes = 0;
};
// the shape checks a decode call shares with its workspace function (rg != NULL: packed queries, S_q and S_new unused)
static int decode_work(const char* fn, const KvRagged* rg, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D,
                       int dtype, fa::KvFormat fmt, KvWork* k) {
  if (rg) {
    if (int rc = ragged_shape(fn, rg->total_q, B, H, H_kv, S_cache, D, dtype, fmt, &k->nsplit, &k->nb_max)) return rc;
    k->ws_bytes = fa::ragged_plan_bytes(k->nb_max) + fa::kvcache_ws_bytes(k->nsplit, 1, H, rg->total_q, D);
  } else {
    if (int rc = kvcache_shape(fn, B, H, H_kv, S_q, S_cache, S_new, D, dtype, fmt, &k->nsplit)) return rc;
    k->ws_bytes = fa::kvcache_ws_bytes(k->nsplit, B, H, S_q, D);
  }
  return 0;
}
// a workspace function, after the checks of its own: the refusal of the shape, or the bytes
static long long workspace_bytes(const char* fn, const KvRagged* rg, int B, int H, int H_kv, int S_q, int S_cache, int S_new,
                                 int D, fa::KvFormat fmt) {
  KvWork k;
  if (int rc = decode_work(fn, rg, B, H, H_kv, S_q, S_cache, S_new, D, MI355FA_FP16, fmt, &k)) return rc;
  return k.ws_bytes;
}

// What a decode call has beside its tensors and its shape; an entry point fills what it offers.
//   softcap > 0 (fa_fwd_kvcache_softcap; already checked): the soft-capped attention kernel
//   slopes      (fa_fwd_kvcache_alibi): the ALiBi attention kernel, slopes and stride checked in kvcache_impl
//   sinks       (fa_fwd_kvcache_sink, _fp8_sink, _fp4; already checked): the sink form of the format's kernel
//   fmt         kE4M3 (fa_fwd_kvcache_fp8): e4m3 caches with the descales f8, the quantising append and the fp8 attention
//               kernel; kMXFP4 (fa_fwd_kvcache_fp4): MXFP4 caches with the scale tensors f4
//   paged       (fa_fwd_kvcache_paged, _fp4_paged): any of them over a pool of pages
//   rg          (fa_fwd_kvcache_ragged, _fp4_ragged, with paged): packed variable-length queries
struct KvCall {
  float softcap = 0.f;
  const float* slopes = nullptr;
  long long slopes_bstride = 0;
  const float* sinks = nullptr;
  fa::KvFormat fmt = fa::KvFormat::k16;
  KvFp8 f8{};
  KvFp4 f4{};
  KvFp8Token ft{};   // fmt kE4M3Token (fa_fwd_kvcache_fp8_token and its paged and packed forms): the row scales
  const KvPaged* paged = nullptr;
  const KvRagged* rg = nullptr;
};
static int kvcache_impl(const char* fn, const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                        const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                        int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, int window_left,
                        int window_right, const mi355fa_opts* opts, void* stream, const KvCall& c) {
  const KvPaged* paged = c.paged;
  const KvRagged* rg = c.rg;
  const KvFp8* f8 = c.fmt == fa::KvFormat::kE4M3 ? &c.f8 : nullptr;
  const KvFp4* f4 = c.fmt == fa::KvFormat::kMXFP4 ? &c.f4 : nullptr;
  const KvFp8Token* ft = c.fmt == fa::KvFormat::kE4M3Token ? &c.ft : nullptr;
  if (!q || !k_cache || !v_cache || !cache_seqlens || !o) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if (f4 && (!f4->k_scale || !f4->v_scale)) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if (ft && (!ft->k_scale || !ft->v_scale)) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if ((k_new == nullptr) != (v_new == nullptr)) return fail(MI355FA_ERR_NULL, "%s: k_new and v_new must be given together", fn);
  if (!k_new && S_new > 0) return fail(MI355FA_ERR_NULL, "%s: S_new > 0 needs k_new and v_new", fn);
  if (k_new && S_new < 1) return fail(MI355FA_ERR_SHAPE, "%s: k_new / v_new given with S_new < 1", fn);
  if (int rc = check_scale(fn, scale)) return rc;
  mi355fa_opts x;
  if (int rc = read_opts(fn, opts, &x)) return rc;
  if (x.cu_seqlens_q || x.p_drop != 0.f || x.q_scaled || x.dout_strides || x.dq_strides || x.dk_strides || x.dv_strides)
    return fail(MI355FA_ERR_SHAPE, "%s: opts may carry the q, k, v and o strides only (no cu_seqlens, dropout or q_scaled)", fn);
  KvWork k;
  if (int rc = decode_work(fn, rg, B, H, H_kv, S_q, S_cache, S_new, D, dtype, c.fmt, &k)) return rc;
  if (f8) {
    if (f8->bstride != 0 && (f8->bstride < (long long)H_kv || (long long)(B - 1) * f8->bstride + H_kv > 0x7fffffffLL))
      return fail(MI355FA_ERR_SHAPE, "%s: descale_bstride must be 0 (shape (H_kv,)) or >= H_kv (shape (B, H_kv))", fn);
    if ((reinterpret_cast<uintptr_t>(f8->k_descale) | reinterpret_cast<uintptr_t>(f8->v_descale)) & 3u)
      return fail(MI355FA_ERR_ALIGN, "%s: k_descale / v_descale must be 4-byte aligned", fn);
  }
  fa::ScoreMod w;
  if (int rc = make_window(fn, window_left, window_right, &w)) return rc;
  if (c.slopes) {
    if (int rc = check_alibi(fn, c.slopes, c.slopes_bstride, B, H)) return rc;
  }
  fa::DecodeParams p{};
  if (rg) {
    if (int rc = make_layout_ragged(fn, x.q_strides, H, D, false, &p.lq)) return rc;
    if (int rc = make_layout_ragged(fn, x.o_strides, H, D, true, &p.lo)) return rc;
  } else if (int rc = make_layout(fn, x.q_strides, H, S_q, D, &p.lq)) {
    return rc;
  }
  const int slice_rows = paged ? paged->page_size : S_cache;   // rows of one (sequence | page, head) slice of the caches
  fa::DecodeFp4 d4{};
  fa::DecodeFp8Token dt{};
  if (f4) {
    if (int rc = make_layout_fp4(fn, false, x.k_strides, H_kv, slice_rows, D, &p.lk)) return rc;
    if (int rc = make_layout_fp4(fn, false, x.v_strides, H_kv, slice_rows, D, &p.lv)) return rc;
    if (int rc = make_layout_fp4(fn, true, f4->k_scale_strides, H_kv, slice_rows, D, &d4.lks)) return rc;
    if (int rc = make_layout_fp4(fn, true, f4->v_scale_strides, H_kv, slice_rows, D, &d4.lvs)) return rc;
    if ((reinterpret_cast<uintptr_t>(f4->k_scale) | reinterpret_cast<uintptr_t>(f4->v_scale)) % (unsigned)(D / 32))
      return fail(MI355FA_ERR_ALIGN, "%s: k_scale / v_scale must be aligned to their row of D / 32 bytes", fn);
    d4.ks = (unsigned char*)f4->k_scale;
    d4.vs = (unsigned char*)f4->v_scale;
  } else if (f8 || ft) {
    if (int rc = make_layout_fp8(fn, x.k_strides, H_kv, slice_rows, D, &p.lk)) return rc;
    if (int rc = make_layout_fp8(fn, x.v_strides, H_kv, slice_rows, D, &p.lv)) return rc;
    if (ft) {
      if (int rc = make_layout_token_scales(fn, ft->k_scale_strides, H_kv, slice_rows, &dt.lks)) return rc;
      if (int rc = make_layout_token_scales(fn, ft->v_scale_strides, H_kv, slice_rows, &dt.lvs)) return rc;
      if ((reinterpret_cast<uintptr_t>(ft->k_scale) | reinterpret_cast<uintptr_t>(ft->v_scale)) & 3u)
        return fail_value(MI355FA_ERR_ALIGN, "%s: k_scale / v_scale must be 4-byte aligned (k_scale | v_scale ends in %lld)", fn,
                          (long long)((reinterpret_cast<uintptr_t>(ft->k_scale) | reinterpret_cast<uintptr_t>(ft->v_scale)) & 3u));
      dt.ks = ft->k_scale;
      dt.vs = ft->v_scale;
    }
  } else {
    if (int rc = make_layout(fn, x.k_strides, H_kv, slice_rows, D, &p.lk)) return rc;
    if (int rc = make_layout(fn, x.v_strides, H_kv, slice_rows, D, &p.lv)) return rc;
  }
  if (p.lk.rs != p.lv.rs) return fail(MI355FA_ERR_STRIDE, "%s: K and V must share their sequence stride", fn);
  if (!rg)
    if (int rc = make_layout(fn, x.o_strides, H, S_q, D, &p.lo, B)) return rc;
  if (rg && (reinterpret_cast<uintptr_t>(rg->cu) & 3u)) return fail(MI355FA_ERR_ALIGN, "%s: cu_seqlens_q must be 4-byte aligned", fn);
  if (misaligned(q) || misaligned(k_cache) || misaligned(v_cache) || misaligned(k_new) || misaligned(v_new) ||
      misaligned(o) || misaligned(lse) || misaligned(workspace) || (reinterpret_cast<uintptr_t>(cache_seqlens) & 3u))
    return fail(MI355FA_ERR_ALIGN, "%s: pointers must be 16-byte aligned (cache_seqlens 4-byte)", fn);
  if (k.ws_bytes > 0 && (!workspace || workspace_bytes < k.ws_bytes))
    return fail(MI355FA_ERR_WORKSPACE, "%s: workspace smaller than fa_fwd_kvcache_workspace_bytes()", fn);
  p.q = q;
  p.kc = k_cache;
  p.vc = v_cache;
  p.k_new = k_new;
  p.v_new = v_new;
  p.seqlens = cache_seqlens;
  p.o = o;
  p.lse = lse;
  p.ws = (float*)workspace;
  p.B = B;
  p.H = H;
  p.Hkv = H_kv;
  p.group = H / H_kv;
  p.Sq = S_q;
  p.Scache = S_cache;
  p.Snew = S_new;
  p.D = D;
  p.scale = scale;
  p.wl = w.wl;
  p.wr = w.wr;
  p.nsplit = k.nsplit;
  fa::DecodeMod m;
  m.fmt = c.fmt;
  if (f8) {
    m.kds = f8->k_descale;
    m.vds = f8->v_descale;
    m.ds_bstride = (int)f8->bstride;
    m.softcap = c.softcap;   // (fa_fwd_kvcache_quant_softcap and its forms alone: every other e4m3 call refuses a cap)
  } else {
    m.softcap = c.softcap;
    m.slopes = c.slopes;
    m.slopes_bstride = (int)c.slopes_bstride;
  }
  m.sinks = c.sinks;
  if (f4) m.fp4 = &d4;
  if (ft) m.tok = &dt;
  fa::DecodePaging pg{};
  if (paged) {
    pg = fa::DecodePaging{paged->table, (int)paged->stride, paged->page_size, paged->num_pages,
                          fa::make_fastdiv(paged->page_size / 32)};
    m.pg = &pg;
  }
  fa::DecodeRagged rd{};
  if (rg) {   // the plan at the head of the workspace, the partials behind it
    rd = fa::DecodeRagged{rg->cu, rg->total_q, (int*)workspace, (int)k.nb_max};
    p.ws = (float*)((char*)workspace + fa::ragged_plan_bytes(k.nb_max));
    p.Sq = 0;
    m.rg = &rd;
  }
  if (hipError_t e = fa::launch_decode(p, dtype, (hipStream_t)stream, m))
    return hip_fail(e, fn);
  return 0;
}

long long fa_fwd_kvcache_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D) {
  return workspace_bytes("fa_fwd_kvcache_workspace_bytes", nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fa::KvFormat::k16);
}
int fa_fwd_kvcache(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                   const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H,
                   int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, int window_left,
                   int window_right, const mi355fa_opts* opts, void* stream) {
  return kvcache_impl("fa_fwd_kvcache", q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes,
                      B, H, H_kv, S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, KvCall{});
}

// ---- FP8 (e4m3) KV caches (include/mi355fa_kvcache_fp8.h) ---------------------------------------------------------------
long long fa_fwd_kvcache_fp8_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D) {
  return workspace_bytes("fa_fwd_kvcache_fp8_workspace_bytes", nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fa::KvFormat::kE4M3);
}
int fa_fwd_kvcache_fp8(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                       const int* cache_seqlens, const float* k_descale, const float* v_descale,
                       long long descale_bstride, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                       int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, int kv_dtype, float scale,
                       int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_fp8";
  if (kv_dtype != MI355FA_KV_FP8_E4M3) return fail(MI355FA_ERR_DTYPE, "%s: kv_dtype must be MI355FA_KV_FP8_E4M3", fn);
  KvCall c;
  c.fmt = fa::KvFormat::kE4M3;
  c.f8 = KvFp8{k_descale, v_descale, descale_bstride};
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}

// ---- logit soft-capping (include/mi355fa_softcap.h): the _gqa and kvcache forms with a cap after the scale ----------
int fa_fwd_softcap(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q,
                   int S_k, int D, int dtype, float scale, float softcap, int window_left, int window_right,
                   const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_softcap";
  fa::ScoreMod w;
  if (int rc = make_group(fn, H, H_kv, &w)) return rc;
  if (int rc = make_window(fn, window_left, window_right, &w)) return rc;
  if (int rc = check_softcap(fn, softcap)) return rc;
  w.softcap = softcap;
  return fwd_impl(fn, q, k, v, o, lse, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dq_softcap(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                      void* dq, float* delta, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                      float softcap, int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_bwd_dq_softcap";
  fa::ScoreMod w;
  if (int rc = make_group(fn, H, H_kv, &w)) return rc;
  if (int rc = make_window(fn, window_left, window_right, &w)) return rc;
  if (int rc = check_softcap(fn, softcap)) return rc;
  w.softcap = softcap;
  return dq_impl(fn, q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dkv_softcap(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                       void* dk, void* dv, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                       float softcap, int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_bwd_dkv_softcap";
  fa::ScoreMod w;
  if (int rc = make_group(fn, H, H_kv, &w)) return rc;
  if (int rc = make_window(fn, window_left, window_right, &w)) return rc;
  if (int rc = check_softcap(fn, softcap)) return rc;
  w.softcap = softcap;
  return dkv_impl(fn, q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_fwd_kvcache_softcap(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                           const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes,
                           int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale,
                           float softcap, int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_softcap";
  if (int rc = check_softcap(fn, softcap)) return rc;
  KvCall c;
  c.softcap = softcap;
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}

// ---- ALiBi (include/mi355fa_alibi.h): the _gqa and kvcache forms with the slopes after the scale ------------------------
static int make_alibi(const char* fn, int B, int H, int H_kv, int window_left, int window_right, const float* slopes,
                      long long stride, fa::ScoreMod* w) {
  if (int rc = make_group(fn, H, H_kv, w)) return rc;
  if (int rc = make_window(fn, window_left, window_right, w)) return rc;
  if (int rc = check_alibi(fn, slopes, stride, B, H)) return rc;
  w->slopes = slopes;
  w->slopes_bstride = (int)stride;
  return 0;
}
int fa_fwd_alibi(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q,
                 int S_k, int D, int dtype, float scale, const float* alibi_slopes, long long slopes_batch_stride,
                 int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_alibi";
  fa::ScoreMod w;
  if (int rc = make_alibi(fn, B, H, H_kv, window_left, window_right, alibi_slopes, slopes_batch_stride, &w)) return rc;
  return fwd_impl(fn, q, k, v, o, lse, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dq_alibi(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    void* dq, float* delta, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                    const float* alibi_slopes, long long slopes_batch_stride, int window_left, int window_right,
                    const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_bwd_dq_alibi";
  fa::ScoreMod w;
  if (int rc = make_alibi(fn, B, H, H_kv, window_left, window_right, alibi_slopes, slopes_batch_stride, &w)) return rc;
  return dq_impl(fn, q, k, v, o, dout, lse, dq, delta, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_bwd_dkv_alibi(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                     void* dk, void* dv, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                     const float* alibi_slopes, long long slopes_batch_stride, int window_left, int window_right,
                     const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_bwd_dkv_alibi";
  fa::ScoreMod w;
  if (int rc = make_alibi(fn, B, H, H_kv, window_left, window_right, alibi_slopes, slopes_batch_stride, &w)) return rc;
  return dkv_impl(fn, q, k, v, dout, lse, delta, dk, dv, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
int fa_fwd_kvcache_alibi(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                         const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                         int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale,
                         const float* alibi_slopes, long long slopes_batch_stride, int window_left, int window_right,
                         const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_alibi";
  if (!alibi_slopes) return fail(MI355FA_ERR_NULL, "%s: alibi_slopes is NULL", fn);
  KvCall c;
  c.slopes = alibi_slopes;
  c.slopes_bstride = slopes_batch_stride;
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}

// ---- attention sinks (include/mi355fa_sink.h): the _gqa and kvcache forms with the sinks after the scale ----------------
int fa_fwd_sink(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q, int S_k,
                int D, int dtype, float scale, const float* sinks, int window_left, int window_right,
                const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_sink";
  fa::ScoreMod w;
  if (int rc = make_group(fn, H, H_kv, &w)) return rc;
  if (int rc = make_window(fn, window_left, window_right, &w)) return rc;
  if (int rc = check_sinks(fn, sinks)) return rc;
  w.sinks = sinks;
  return fwd_impl(fn, q, k, v, o, lse, B, H, S_q, S_k, D, dtype, 0, scale, opts, stream, &w);
}
// dsinks[h] = -sum_{b, i} exp(sinks[h] - lse[b, h, i]) * delta[b, h, i] over the rows fa_bwd_dq_gqa wrote delta for
int fa_bwd_dsink(const float* lse, const float* delta, const float* sinks, float* dsinks, int B, int H, int S_q,
                 const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_bwd_dsink";
  if (!lse || !delta || !dsinks) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if (int rc = check_sinks(fn, sinks)) return rc;
  mi355fa_opts x;
  if (int rc = read_opts(fn, opts, &x)) return rc;
  if (B < 1 || H < 1 || S_q < 1) return fail(MI355FA_ERR_SHAPE, "%s: B, H, S_q must be >= 1", fn);
  if (x.cu_seqlens_q && x.total_q < 1) return fail(MI355FA_ERR_SHAPE, "%s: total tokens must be >= 1", fn);
  if (misaligned(lse) || misaligned(delta)) return fail(MI355FA_ERR_ALIGN, "%s: lse and delta must be 16-byte aligned", fn);
  if (reinterpret_cast<uintptr_t>(dsinks) & 3u) return fail(MI355FA_ERR_ALIGN, "%s: dsinks must be 4-byte aligned", fn);
  // the LSE / delta layouts of fwd_impl and bwd_fill: [B, H, S_q], or [H, total_q] for packed sequences
  const hipError_t e = x.cu_seqlens_q
                           ? fa::launch_bwd_dsink(lse, delta, sinks, dsinks, H, 1, x.total_q, 0, x.total_q, (hipStream_t)stream)
                           : fa::launch_bwd_dsink(lse, delta, sinks, dsinks, H, B, S_q, (long long)H * S_q, S_q, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, fn);
  return 0;
}
int fa_fwd_kvcache_sink(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                        const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                        int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, const float* sinks,
                        int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_sink";
  if (int rc = check_sinks(fn, sinks)) return rc;
  KvCall c;
  c.sinks = sinks;
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}
int fa_fwd_kvcache_fp8_sink(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                            const int* cache_seqlens, const float* k_descale, const float* v_descale,
                            long long descale_bstride, void* o, float* lse, void* workspace, long long workspace_bytes,
                            int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, int kv_dtype,
                            float scale, const float* sinks, int window_left, int window_right, const mi355fa_opts* opts,
                            void* stream) {
  const char* fn = "fa_fwd_kvcache_fp8_sink";
  if (kv_dtype != MI355FA_KV_FP8_E4M3) return fail(MI355FA_ERR_DTYPE, "%s: kv_dtype must be MI355FA_KV_FP8_E4M3", fn);
  if (int rc = check_sinks(fn, sinks)) return rc;
  KvCall c;
  c.sinks = sinks;
  c.fmt = fa::KvFormat::kE4M3;
  c.f8 = KvFp8{k_descale, v_descale, descale_bstride};
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}


// ---- paged KV caches (include/mi355fa_paged.h): every decode variant over a pool of pages and a block table --------------
// The page geometry: page_size a positive multiple of the kernels' 32-key tile, the counts >= 1, and S_cache =
// max_pages_per_seq * page_size inside int (kvcache_shape bounds it further).
static int check_paged_shape(const char* fn, int num_pages, int page_size, int max_pages, int* S_cache) {
  if (page_size < 32 || page_size % 32 != 0)
    return fail(MI355FA_ERR_PAGED, "%s: page_size must be a positive multiple of 32", fn);
  if (num_pages < 1 || max_pages < 1) return fail(MI355FA_ERR_PAGED, "%s: num_pages and max_pages_per_seq must be >= 1", fn);
  if ((long long)max_pages * page_size > 0x7fffffffLL)
    return fail(MI355FA_ERR_PAGED, "%s: max_pages_per_seq * page_size must stay below 2^31", fn);
  *S_cache = max_pages * page_size;
  return 0;
}
// cache_dtype of the calls that take 16-bit and e4m3 pools -> the format (checked after the page geometry)
static int paged_format(const char* fn, int cache_dtype, fa::KvFormat* fmt) {
  if (cache_dtype != MI355FA_PAGED_CACHE_16BIT && cache_dtype != MI355FA_PAGED_CACHE_FP8_E4M3)
    return fail(MI355FA_ERR_DTYPE, "%s: cache_dtype must be MI355FA_PAGED_CACHE_16BIT or MI355FA_PAGED_CACHE_FP8_E4M3", fn);
  *fmt = cache_dtype == MI355FA_PAGED_CACHE_FP8_E4M3 ? fa::KvFormat::kE4M3 : fa::KvFormat::k16;
  return 0;
}
// The block table of a call, in two steps (cache_dtype, where a call has one, is checked between them): the pointer and the
// page geometry it indexes, then its row stride and its alignment.
static int check_block_table(const char* fn, const int* block_table, int num_pages, int page_size, int max_pages, int* S_cache) {
  if (!block_table) return fail(MI355FA_ERR_NULL, "%s: block_table is NULL", fn);
  return check_paged_shape(fn, num_pages, page_size, max_pages, S_cache);
}
static int check_block_table_stride(const char* fn, const int* block_table, long long stride, int max_pages) {
  if (stride < (long long)max_pages || stride > 0x7fffffffLL)
    return fail(MI355FA_ERR_PAGED, "%s: block_table_stride must be at least max_pages_per_seq (and below 2^31)", fn);
  if (reinterpret_cast<uintptr_t>(block_table) & 3u) return fail(MI355FA_ERR_ALIGN, "%s: block_table must be 4-byte aligned", fn);
  return 0;
}
long long fa_fwd_kvcache_paged_workspace_bytes(int B, int H, int H_kv, int S_q, int max_pages_per_seq, int page_size,
                                               int S_new, int D, int cache_dtype) {
  const char* fn = "fa_fwd_kvcache_paged_workspace_bytes";
  int S_cache = 0;
  fa::KvFormat fmt;
  if (int rc = check_paged_shape(fn, 1, page_size, max_pages_per_seq, &S_cache)) return rc;
  if (int rc = paged_format(fn, cache_dtype, &fmt)) return rc;
  return workspace_bytes(fn, nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fmt);
}
// fa_fwd_kvcache_paged, and fa_fwd_kvcache_ragged (rg != NULL: include/mi355fa_ragged.h) over the same pools and mods
static int paged_impl(const char* fn, const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                      const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace,
                      long long workspace_bytes, int B, int H, int H_kv, int S_q, int num_pages, int page_size,
                      int max_pages_per_seq, long long block_table_stride, int S_new, int D, int dtype, int cache_dtype,
                      float scale, int window_left, int window_right, const mi355fa_paged_mods* mods,
                      const mi355fa_opts* opts, void* stream, const KvRagged* rg = nullptr) {
  int S_cache = 0;
  KvCall c;
  if (int rc = check_block_table(fn, block_table, num_pages, page_size, max_pages_per_seq, &S_cache)) return rc;
  if (int rc = paged_format(fn, cache_dtype, &c.fmt)) return rc;
  if (int rc = check_block_table_stride(fn, block_table, block_table_stride, max_pages_per_seq)) return rc;
  // the transform and the cache format: what the padded entry points offer, each member checked as there
  const mi355fa_paged_mods m = mods ? *mods : mi355fa_paged_mods{};
  const bool fp8 = c.fmt == fa::KvFormat::kE4M3;
  uint32_t cap_bits;
  memcpy(&cap_bits, &m.softcap, sizeof(cap_bits));
  const bool capped = cap_bits != 0;   // (on the bits: NaN and -0.0 are "given", and refused by check_softcap)
  if ((int)capped + (m.alibi_slopes != nullptr) + (m.sinks != nullptr) > 1)
    return fail(MI355FA_ERR_PAGED, "%s: at most one of softcap, alibi_slopes and sinks may be given", fn);
  if (fp8 && (capped || m.alibi_slopes))
    return fail(MI355FA_ERR_PAGED, "%s: an fp8 cache takes sinks only (no softcap, no alibi_slopes)", fn);
  if (!fp8 && (m.k_descale || m.v_descale || m.descale_bstride != 0))
    return fail(MI355FA_ERR_PAGED, "%s: k_descale / v_descale belong to an fp8 cache", fn);
  if (capped)
    if (int rc = check_softcap(fn, m.softcap)) return rc;
  if (m.sinks)
    if (int rc = check_sinks(fn, m.sinks)) return rc;
  const KvPaged paged{block_table, block_table_stride, num_pages, page_size, max_pages_per_seq};
  c.softcap = capped ? m.softcap : 0.f;
  c.slopes = m.alibi_slopes;
  c.slopes_bstride = m.slopes_batch_stride;
  c.sinks = m.sinks;
  c.f8 = KvFp8{m.k_descale, m.v_descale, m.descale_bstride};
  c.paged = &paged;
  c.rg = rg;
  return kvcache_impl(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv, S_q,
                      S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}
int fa_fwd_kvcache_paged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                         const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace,
                         long long workspace_bytes, int B, int H, int H_kv, int S_q, int num_pages, int page_size,
                         int max_pages_per_seq, long long block_table_stride, int S_new, int D, int dtype, int cache_dtype,
                         float scale, int window_left, int window_right, const mi355fa_paged_mods* mods,
                         const mi355fa_opts* opts, void* stream) {
  return paged_impl("fa_fwd_kvcache_paged", q, k_pool, v_pool, k_new, v_new, cache_seqlens, block_table, o, lse, workspace,
                    workspace_bytes, B, H, H_kv, S_q, num_pages, page_size, max_pages_per_seq, block_table_stride, S_new, D,
                    dtype, cache_dtype, scale, window_left, window_right, mods, opts, stream);
}

// ---- MXFP4 KV caches (include/mi355fa_kvcache_fp4.h): padded and paged --------------------------------------------------
// what the two calls and their workspace functions check first: the format, and the head dims that have an MXFP4 kernel
static int check_fp4(const char* fn, int D, int kv_dtype) {
  if (kv_dtype != MI355FA_KV_MXFP4) return fail(MI355FA_ERR_DTYPE, "%s: kv_dtype must be MI355FA_KV_MXFP4", fn);
  if (D != 64 && D != 128) return fail(MI355FA_ERR_SHAPE, "%s: an MXFP4 cache takes head dim 64 or 128", fn);
  return 0;
}
long long fa_fwd_kvcache_fp4_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D) {
  const char* fn = "fa_fwd_kvcache_fp4_workspace_bytes";
  if (int rc = check_fp4(fn, D, MI355FA_KV_MXFP4)) return rc;
  return workspace_bytes(fn, nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fa::KvFormat::kMXFP4);
}
int fa_fwd_kvcache_fp4(const void* q, void* k_cache, void* v_cache, void* k_scale, void* v_scale, const void* k_new,
                       const void* v_new, const int* cache_seqlens, const long long* k_scale_strides,
                       const long long* v_scale_strides, const float* sinks, void* o, float* lse, void* workspace,
                       long long workspace_bytes, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype,
                       int kv_dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_fp4";
  if (int rc = check_fp4(fn, D, kv_dtype)) return rc;
  if (sinks)
    if (int rc = check_sinks(fn, sinks)) return rc;
  KvCall c;
  c.sinks = sinks;
  c.fmt = fa::KvFormat::kMXFP4;
  c.f4 = KvFp4{k_scale, v_scale, k_scale_strides, v_scale_strides};
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}
long long fa_fwd_kvcache_fp4_paged_workspace_bytes(int B, int H, int H_kv, int S_q, int max_pages_per_seq, int page_size,
                                                   int S_new, int D) {
  const char* fn = "fa_fwd_kvcache_fp4_paged_workspace_bytes";
  int S_cache = 0;
  if (int rc = check_fp4(fn, D, MI355FA_KV_MXFP4)) return rc;
  if (int rc = check_paged_shape(fn, 1, page_size, max_pages_per_seq, &S_cache)) return rc;
  return workspace_bytes(fn, nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fa::KvFormat::kMXFP4);
}
int fa_fwd_kvcache_fp4_paged(const void* q, void* k_pool, void* v_pool, void* k_scale, void* v_scale, const void* k_new,
                             const void* v_new, const int* cache_seqlens, const int* block_table,
                             const long long* k_scale_strides, const long long* v_scale_strides, const float* sinks, void* o,
                             float* lse, void* workspace, long long workspace_bytes, int B, int H, int H_kv, int S_q,
                             int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride, int S_new,
                             int D, int dtype, int kv_dtype, float scale, int window_left, int window_right,
                             const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_fp4_paged";
  if (int rc = check_fp4(fn, D, kv_dtype)) return rc;
  int S_cache = 0;
  if (int rc = check_block_table(fn, block_table, num_pages, page_size, max_pages_per_seq, &S_cache)) return rc;
  if (int rc = check_block_table_stride(fn, block_table, block_table_stride, max_pages_per_seq)) return rc;
  if (sinks)
    if (int rc = check_sinks(fn, sinks)) return rc;
  const KvPaged paged{block_table, block_table_stride, num_pages, page_size, max_pages_per_seq};
  KvCall c;
  c.sinks = sinks;
  c.fmt = fa::KvFormat::kMXFP4;
  c.f4 = KvFp4{k_scale, v_scale, k_scale_strides, v_scale_strides};
  c.paged = &paged;
  return kvcache_impl(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv, S_q,
                      S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}

// ---- packed variable-length queries over a paged cache (include/mi355fa_ragged.h) ----------------------------------------
long long fa_fwd_kvcache_ragged_workspace_bytes(int total_q, int B, int H, int H_kv, int max_pages_per_seq, int page_size,
                                                int D, int cache_dtype) {
  const char* fn = "fa_fwd_kvcache_ragged_workspace_bytes";
  int S_cache = 0;
  fa::KvFormat fmt;
  if (int rc = check_paged_shape(fn, 1, page_size, max_pages_per_seq, &S_cache)) return rc;
  if (int rc = paged_format(fn, cache_dtype, &fmt)) return rc;
  const KvRagged rg{nullptr, total_q};
  return workspace_bytes(fn, &rg, B, H, H_kv, 0, S_cache, 0, D, fmt);
}
// Not part of the public header: the plan kernel of fa_fwd_kvcache_ragged alone, into `plan` (the head of a workspace of
// fa_fwd_kvcache_ragged_workspace_bytes).  tools/ragged_bench.py times it.
int fa_debug_ragged_plan(const int* cu_seqlens_q, int* plan, int total_q, int B, int H, int H_kv, void* stream) {
  const char* fn = "fa_debug_ragged_plan";
  fa::ScoreMod w;
  if (int rc = make_group(fn, H, H_kv, &w)) return rc;
  if (!cu_seqlens_q || !plan) return fail(MI355FA_ERR_NULL, "%s: NULL pointer", fn);
  if (total_q < 1 || B < 1 || H < 1 || (long long)H * total_q > (1 << 24) || B > (1 << 24))
    return fail(MI355FA_ERR_RAGGED, "%s: total_q, B and H must be >= 1, H * total_q and B at most 2^24", fn);
  const fa::DecodeRagged rd{cu_seqlens_q, total_q, plan, (int)fa::ragged_nb_max(w.group, total_q, B)};
  if (hipError_t e = fa::launch_ragged_plan(cu_seqlens_q, B, w.group, rd, (hipStream_t)stream)) return hip_fail(e, fn);
  return 0;
}
int fa_fwd_kvcache_ragged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                          const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* o, float* lse,
                          void* workspace, long long workspace_bytes, int total_q, int B, int H, int H_kv, int num_pages,
                          int page_size, int max_pages_per_seq, long long block_table_stride, int D, int dtype,
                          int cache_dtype, float scale, int window_left, int window_right, const mi355fa_paged_mods* mods,
                          const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_ragged";
  if (!cu_seqlens_q) return fail(MI355FA_ERR_NULL, "%s: cu_seqlens_q is NULL", fn);
  if (total_q < 1 || B < 1) return fail(MI355FA_ERR_RAGGED, "%s: total_q and B must be >= 1", fn);
  const KvRagged rg{cu_seqlens_q, total_q};
  return paged_impl(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, block_table, o, lse, workspace, workspace_bytes, B, H,
                    H_kv, 0, num_pages, page_size, max_pages_per_seq, block_table_stride, k_new || v_new ? 1 : 0, D, dtype,
                    cache_dtype, scale, window_left, window_right, mods, opts, stream, &rg);
}

// ---- packed variable-length queries over paged MXFP4 pools (include/mi355fa_ragged_fp4.h) --------------------------------
// The format and the head dims of the packed MXFP4 call: its own check, since this is the one MXFP4 call with a D = 256 kernel
// (check_fp4 keeps the two rectangular calls' refusal).
static int check_fp4_ragged(const char* fn, int D, int kv_dtype) {
  if (kv_dtype != MI355FA_KV_MXFP4) return fail(MI355FA_ERR_DTYPE, "%s: kv_dtype must be MI355FA_KV_MXFP4", fn);
  if (D != 64 && D != 128 && D != 256) {   // (with the value: the call's own text, beside the recorded ones of the older calls)
    snprintf(g_err, sizeof(g_err), "%s: packed queries over an MXFP4 cache take head dim 64, 128 or 256 (got %d)", fn, D);
    return MI355FA_ERR_SHAPE;
  }
  return 0;
}
long long fa_fwd_kvcache_fp4_ragged_workspace_bytes(int total_q, int B, int H, int H_kv, int max_pages_per_seq, int page_size,
                                                    int D) {
  const char* fn = "fa_fwd_kvcache_fp4_ragged_workspace_bytes";
  int S_cache = 0;
  if (int rc = check_fp4_ragged(fn, D, MI355FA_KV_MXFP4)) return rc;
  if (int rc = check_paged_shape(fn, 1, page_size, max_pages_per_seq, &S_cache)) return rc;
  const KvRagged rg{nullptr, total_q};
  return workspace_bytes(fn, &rg, B, H, H_kv, 0, S_cache, 0, D, fa::KvFormat::kMXFP4);
}
int fa_fwd_kvcache_fp4_ragged(const void* q, void* k_pool, void* v_pool, void* k_scale, void* v_scale, const void* k_new,
                              const void* v_new, const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table,
                              const long long* k_scale_strides, const long long* v_scale_strides, const float* sinks, void* o,
                              float* lse, void* workspace, long long workspace_bytes, int total_q, int B, int H, int H_kv,
                              int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride, int D,
                              int dtype, int kv_dtype, float scale, int window_left, int window_right,
                              const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_fp4_ragged";
  if (!cu_seqlens_q) return fail(MI355FA_ERR_NULL, "%s: cu_seqlens_q is NULL", fn);
  if (total_q < 1 || B < 1) return fail(MI355FA_ERR_RAGGED, "%s: total_q and B must be >= 1", fn);
  if (int rc = check_fp4_ragged(fn, D, kv_dtype)) return rc;
  int S_cache = 0;
  if (int rc = check_block_table(fn, block_table, num_pages, page_size, max_pages_per_seq, &S_cache)) return rc;
  if (int rc = check_block_table_stride(fn, block_table, block_table_stride, max_pages_per_seq)) return rc;
  if (sinks)
    if (int rc = check_sinks(fn, sinks)) return rc;
  const KvPaged paged{block_table, block_table_stride, num_pages, page_size, max_pages_per_seq};
  const KvRagged rg{cu_seqlens_q, total_q};
  KvCall c;
  c.sinks = sinks;
  c.fmt = fa::KvFormat::kMXFP4;
  c.f4 = KvFp4{k_scale, v_scale, k_scale_strides, v_scale_strides};
  c.paged = &paged;
  c.rg = &rg;
  return kvcache_impl(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv, 0,
                      S_cache, k_new || v_new ? 1 : 0, D, dtype, scale, window_left, window_right, opts, stream, c);
}

// ---- per-token-scaled e4m3 KV caches (include/mi355fa_kvcache_fp8_token.h): padded, paged and packed ----------------------
// The head dims with a kernel: 64 and 128, and 256 for packed queries; D = 256 on the two rectangular calls is refused with
// MI355FA_ERR_SHAPE as the MXFP4 calls refuse it, every other head dim by the decode calls' shared check (MI355FA_ERR_HEAD_DIM).
static int check_fp8_token(const char* fn, int D, bool packed) {
  if (D == 256 && !packed)
    return fail_value(MI355FA_ERR_SHAPE,
                      "%s: a per-token-scaled cache takes head dim %lld with packed queries only (fa_fwd_kvcache_fp8_token_ragged)", fn, D);
  return 0;
}
long long fa_fwd_kvcache_fp8_token_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D) {
  const char* fn = "fa_fwd_kvcache_fp8_token_workspace_bytes";
  if (int rc = check_fp8_token(fn, D, false)) return rc;
  return workspace_bytes(fn, nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fa::KvFormat::kE4M3Token);
}
int fa_fwd_kvcache_fp8_token(const void* q, void* k_cache, void* v_cache, float* k_scale, float* v_scale, const void* k_new,
                             const void* v_new, const int* cache_seqlens, const long long* k_scale_strides,
                             const long long* v_scale_strides, const float* sinks, void* o, float* lse, void* workspace,
                             long long workspace_bytes, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D,
                             int dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts,
                             void* stream) {
  const char* fn = "fa_fwd_kvcache_fp8_token";
  if (int rc = check_fp8_token(fn, D, false)) return rc;
  if (sinks)
    if (int rc = check_sinks(fn, sinks)) return rc;
  KvCall c;
  c.sinks = sinks;
  c.fmt = fa::KvFormat::kE4M3Token;
  c.ft = KvFp8Token{k_scale, v_scale, k_scale_strides, v_scale_strides};
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}
long long fa_fwd_kvcache_fp8_token_paged_workspace_bytes(int B, int H, int H_kv, int S_q, int max_pages_per_seq, int page_size,
                                                         int S_new, int D) {
  const char* fn = "fa_fwd_kvcache_fp8_token_paged_workspace_bytes";
  int S_cache = 0;
  if (int rc = check_fp8_token(fn, D, false)) return rc;
  if (int rc = check_paged_shape(fn, 1, page_size, max_pages_per_seq, &S_cache)) return rc;
  return workspace_bytes(fn, nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fa::KvFormat::kE4M3Token);
}
int fa_fwd_kvcache_fp8_token_paged(const void* q, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const void* k_new,
                                   const void* v_new, const int* cache_seqlens, const int* block_table,
                                   const long long* k_scale_strides, const long long* v_scale_strides, const float* sinks,
                                   void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H, int H_kv,
                                   int S_q, int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride,
                                   int S_new, int D, int dtype, float scale, int window_left, int window_right,
                                   const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_fp8_token_paged";
  if (int rc = check_fp8_token(fn, D, false)) return rc;
  int S_cache = 0;
  if (int rc = check_block_table(fn, block_table, num_pages, page_size, max_pages_per_seq, &S_cache)) return rc;
  if (int rc = check_block_table_stride(fn, block_table, block_table_stride, max_pages_per_seq)) return rc;
  if (sinks)
    if (int rc = check_sinks(fn, sinks)) return rc;
  const KvPaged paged{block_table, block_table_stride, num_pages, page_size, max_pages_per_seq};
  KvCall c;
  c.sinks = sinks;
  c.fmt = fa::KvFormat::kE4M3Token;
  c.ft = KvFp8Token{k_scale, v_scale, k_scale_strides, v_scale_strides};
  c.paged = &paged;
  return kvcache_impl(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv, S_q,
                      S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}
long long fa_fwd_kvcache_fp8_token_ragged_workspace_bytes(int total_q, int B, int H, int H_kv, int max_pages_per_seq,
                                                          int page_size, int D) {
  const char* fn = "fa_fwd_kvcache_fp8_token_ragged_workspace_bytes";
  int S_cache = 0;
  if (int rc = check_fp8_token(fn, D, true)) return rc;
  if (int rc = check_paged_shape(fn, 1, page_size, max_pages_per_seq, &S_cache)) return rc;
  const KvRagged rg{nullptr, total_q};
  return workspace_bytes(fn, &rg, B, H, H_kv, 0, S_cache, 0, D, fa::KvFormat::kE4M3Token);
}
int fa_fwd_kvcache_fp8_token_ragged(const void* q, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const void* k_new,
                                    const void* v_new, const int* cu_seqlens_q, const int* cache_seqlens,
                                    const int* block_table, const long long* k_scale_strides,
                                    const long long* v_scale_strides, const float* sinks, void* o, float* lse, void* workspace,
                                    long long workspace_bytes, int total_q, int B, int H, int H_kv, int num_pages,
                                    int page_size, int max_pages_per_seq, long long block_table_stride, int D, int dtype,
                                    float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_fp8_token_ragged";
  if (!cu_seqlens_q) return fail(MI355FA_ERR_NULL, "%s: cu_seqlens_q is NULL", fn);
  if (total_q < 1 || B < 1) return fail(MI355FA_ERR_RAGGED, "%s: total_q and B must be >= 1", fn);
  if (int rc = check_fp8_token(fn, D, true)) return rc;
  int S_cache = 0;
  if (int rc = check_block_table(fn, block_table, num_pages, page_size, max_pages_per_seq, &S_cache)) return rc;
  if (int rc = check_block_table_stride(fn, block_table, block_table_stride, max_pages_per_seq)) return rc;
  if (sinks)
    if (int rc = check_sinks(fn, sinks)) return rc;
  const KvPaged paged{block_table, block_table_stride, num_pages, page_size, max_pages_per_seq};
  const KvRagged rg{cu_seqlens_q, total_q};
  KvCall c;
  c.sinks = sinks;
  c.fmt = fa::KvFormat::kE4M3Token;
  c.ft = KvFp8Token{k_scale, v_scale, k_scale_strides, v_scale_strides};
  c.paged = &paged;
  c.rg = &rg;
  return kvcache_impl(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv, 0,
                      S_cache, k_new || v_new ? 1 : 0, D, dtype, scale, window_left, window_right, opts, stream, c);
}

}  // extern "C"

// ---- soft-capped decoding over the quantised caches (include_quant/mi355fa_kvcache_quant_softcap.h) -----------------------------
// The entry points and their own refusal texts are fa_api_quant_softcap.hip's; here is what they share with every decode call
// (fa_quant_softcap.h): the checks above in the order of the format's own call, and kvcache_impl.
namespace fa {
int api_fail_value(int code, const char* fmt, const char* fn, long long value) { return fail_value(code, fmt, fn, value); }

int kvcache_quant_softcap(const char* fn, const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                          const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H,
                          int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, int window_left,
                          int window_right, const mi355fa_opts* opts, void* stream, const QuantSoftcapCall& a) {
  if (a.packed) {
    if (!a.cu) return fail(MI355FA_ERR_NULL, "%s: cu_seqlens_q is NULL", fn);
    if (a.total_q < 1 || B < 1) return fail(MI355FA_ERR_RAGGED, "%s: total_q and B must be >= 1", fn);
  }
  if (int rc = check_softcap(fn, a.softcap)) return rc;
  if (a.paged) {
    if (int rc = check_block_table(fn, a.block_table, a.num_pages, a.page_size, a.max_pages, &S_cache)) return rc;
    if (int rc = check_block_table_stride(fn, a.block_table, a.block_table_stride, a.max_pages)) return rc;
  }
  const KvPaged paged{a.block_table, a.block_table_stride, a.num_pages, a.page_size, a.max_pages};
  const KvRagged rg{a.cu, a.total_q};
  KvCall c;
  c.softcap = a.softcap;
  c.fmt = a.fmt;
  c.f8 = KvFp8{a.k_descale, a.v_descale, a.descale_bstride};
  c.f4 = KvFp4{a.k_scale, a.v_scale, a.k_scale_strides, a.v_scale_strides};
  c.ft = KvFp8Token{(float*)a.k_scale, (float*)a.v_scale, a.k_scale_strides, a.v_scale_strides};
  if (a.paged) c.paged = &paged;
  if (a.packed) c.rg = &rg;
  return kvcache_impl(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H, H_kv,
                      a.packed ? 0 : S_q, S_cache, a.packed ? (k_new || v_new ? 1 : 0) : S_new, D, dtype, scale, window_left,
                      window_right, opts, stream, c);
}

long long kvcache_quant_softcap_workspace(const char* fn, KvFormat fmt, bool paged, bool packed, int total_q, int B, int H,
                                          int H_kv, int S_q, int S_cache, int max_pages, int page_size, int S_new, int D) {
  if (paged)
    if (int rc = check_paged_shape(fn, 1, page_size, max_pages, &S_cache)) return rc;
  const KvRagged rg{nullptr, total_q};
  return packed ? workspace_bytes(fn, &rg, B, H, H_kv, 0, S_cache, 0, D, fmt)
                : workspace_bytes(fn, nullptr, B, H, H_kv, S_q, S_cache, S_new, D, fmt);
}
}  // namespace fa
