// MLA (multi-head latent attention) decoding over a paged latent cache: include_mla/mi355fa_kvcache_mla.h.
//
// DeepSeek-V2 / V3 / R1 and Kimi-K2 cache ONE row of 576 values per token -- 512 latent dims and 64 RoPE dims -- that all H
// query heads share.  In the absorbed decode form a query head has those 576 dims, the key of a token is its whole row and
// its value is the first 512 values of the same row: D_qk = 576, D_v = 512, H_kv = 1, and K and V are the same bytes.
//
//   fa_kvcache_append_paged_kernel<MLA, T>  kv_new rows -> cache rows seqlens[b] + j through the table  (first, same stream)
//   fa_decode_paged_kernel<MLA, T>          one workgroup per (sequence, 32-row block of the H * S_q rows, split)
//   fa_decode_combine_kernel<512, T>        nsplit > 1: the shared combine kernel (fa_decode_combine.inc) at the latent width
// (overloads of the decode kernels' names by their template parameters: the MLA tag is a type, which no other overload takes
// first.)
//
// The attention kernel is built from what fa_decode_body.inc has and has measured.  The MFMA rows are the H * S_q (query, head)
// rows, query-major (row = i * H + head: the body's mapping with g = H and one K/V head), so a latent byte is read once per 32
// rows.  All four waves work on the SAME 32-key tile and wave w owns a quarter of the head dim: latent columns
// [128 w, 128 w + 128) and RoPE columns [512 + 16 w, 512 + 16 w + 16).  Per wave and tile:
//   K = V  lane (r, h) loads key r's nine 16-byte pieces straight into the MFMA A layout -- eight of the latent quarter, one of
//          the RoPE slice --, prefetched one tile ahead.  The eight latent pieces go from the same registers into the wave's
//          swizzled 32 x 128 LDS tile (lds_off<128>, chunk 2 ks + h): there is no second global load for V.
//   S^T    the wave's partial = 9 MFMA k-steps against the Q fragments gathered once at the same columns.
//   exchange  each wave writes its partial to an LDS slot chosen by step parity, and behind ONE workgroup barrier all four
//          waves add the four partials as (p0 + p1) + (p2 + p3): the same bits in every wave, so one m, l and P per row.  It is
//          the D = 256 exchange (two slots per wave) widened from pairs to four, and its ordering argument carries over: the
//          write of step k + 2 into the slot of step k follows the barrier of step k + 1, which a wave joins only once its
//          reads of step k have returned (xch_sync waits for lgkmcnt(0) in front of the barrier).
//   softmax, O^T += V^T P^T on the wave's 128 latent columns: the D = 128 wave's code (lds_read_tr_frag, tr_lane_off<128>).
// The paged lookup is the body's PAGED pipeline: a scalar table entry looked up a step ahead through the constant address
// space and a descriptor rebased on the page that covers the page's rows below L only; an entry outside the pool gives an
// empty descriptor.  No access leaves the pool whatever the table or cache_seqlens hold, and rows at or past L are never read.
// There is one key group, so the merge only lays the four waves' 128 columns side by side (fp32 rows of 512 + 4) and writes
// O / LSE (one split) or the fp32 partial (O, m, l) in the decode calls' workspace layout with D = 512.  Every order is fixed:
// the result is deterministic.
// LDS: 32 KiB of V tiles + 32 KiB of exchange slots in the loop, the 64.5 KiB merge stage over them: 64.75 KiB, two workgroups
// per CU.
#include <algorithm>

#include "fa_common.h"
#include "fa_decode_mla.h"

namespace fa {

#include "fa_decode_combine.inc"

namespace {

constexpr int kMlaTile = 32;    // keys per step
constexpr int kMlaRows = 32;    // MFMA rows per workgroup
constexpr int kMlaWaves = 4;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

struct MlaCfg {
  static constexpr int HD = kMlaDv / kMlaWaves;             // the latent columns of one wave: the D = 128 wave's tile
  static constexpr int RD = (kMlaD - kMlaDv) / kMlaWaves;   // its RoPE columns: one k-step
  static constexpr int KS = HD / 16;                        // latent k-steps of S^T = K Q^T
  static constexpr int DB = HD / 32;                        // 32-column blocks of the wave's O^T
  static constexpr int ROWB = HD * 2;                       // a row of the wave's V tile
  static constexpr int VT_BYTES = kMlaWaves * kMlaTile * ROWB;
  static constexpr int XCH_OFF = VT_BYTES;                  // behind the V tiles
  static constexpr int XCH_SLOT = 64 * 16 * 4;              // one wave's 32 x 32 fp32 partial scores
  static constexpr int LOOP_BYTES = XCH_OFF + 2 * kMlaWaves * XCH_SLOT;
  static constexpr int OST = kMlaDv + 4;                    // fp32 row stride of the merge stage (bank spread)
  static constexpr int MERGE_BYTES = kMlaRows * OST * 4;
  static constexpr int ML_OFF = MERGE_BYTES;
  static constexpr int LDS_BYTES = (LOOP_BYTES > MERGE_BYTES ? LOOP_BYTES : MERGE_BYTES) + 2 * kMlaRows * 4;
  static_assert(RD == 16, "the RoPE slice of a wave is one MFMA k-step");
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

}  // namespace

template <typename TAG, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_paged_kernel(MlaParams p) {
  static_assert(std::is_same<TAG, MLA>::value, "the MLA overload");
  constexpr bool RAGGED = false;
  const int *cu_q = nullptr, *plan = nullptr;   // the packed kernel's, unused here
  constexpr int total_q = 0;
#include "fa_decode_mla_body.inc"
}

// The append: kv_new [B, S_new, 576] -> cache rows seqlens[b] + j through the table, one 16-byte chunk per thread, as
// fa_kvcache_append_paged_kernel does.  A row outside [0, Scache), or whose table entry is outside the pool, is dropped.
// (T: the rows are copied, whatever 16-bit type they hold; the instances follow the attention kernel's.)
template <typename TAG, typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(MlaParams p) {
  static_assert(std::is_same<TAG, MLA>::value, "the MLA overload");
  constexpr int cpr = kMlaRowB / 16;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.B * p.Snew * cpr) return;
  const int c = (int)(item % cpr);
  const long long rowi = item / cpr;   // b * S_new + j
  const int j = (int)(rowi % p.Snew), b = (int)(rowi / p.Snew);
  const int dst = p.seqlens[b] + j;
  if (dst < 0 || dst >= p.Scache) return;
  const int pi = dst / p.page_size;
  const int page = p.table[(long long)b * p.bt_stride + pi];
  if ((unsigned)page >= (unsigned)p.num_pages) return;
  *(u32x4*)((char*)p.kv + page * p.kv_ps + (long long)(dst - pi * p.page_size) * p.kv_rs + c * 16) =
      *(const u32x4*)((const char*)p.kv_new + rowi * kMlaRowB + c * 16);
}

// ---- packed variable-length queries (include_mla_ragged/mi355fa_ragged_mla.h, fa_decode_mla.h LatentRaggedParams) ----------
//   fa_decode_ragged_plan_kernel               fa_decode.hip's, with group = H: cu_seqlens_q -> the step's 32-row blocks (b, rb)
//   fa_kvcache_append_ragged_kernel<Latent, T>  packed kv_new rows -> cache rows seqlens[b] + i through the table
//   fa_decode_ragged_kernel<Latent, T>          the body with RAGGED: one workgroup per (plan entry, split)
//   fa_decode_combine_ragged_kernel<Latent, T>  nsplit > 1: the combine by (head, packed row) at the latent width
// (overloads of the packed decode kernels' names by their template parameters, as the rectangular kernels above are of the
// paged ones': the Latent tag is a type, which no other overload takes first.  A tag and a parameter block of their own: the
// rectangular kernels' names -- <MLA, T>, <512, T>, MlaParams -- are a recorded set, tests/test_host_mla.py.)
template <typename TAG, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_ragged_kernel(LatentRaggedParams p) {
  static_assert(std::is_same<TAG, Latent>::value, "the latent overload");
  constexpr bool RAGGED = true;
  const int *cu_q = p.cu_q, *plan = p.plan;
  const int total_q = p.total_q;
#include "fa_decode_mla_body.inc"
}

// ragged_len, the owner bisection and the combine's arithmetic below are fa_decode.hip's (ragged_len, ragged_owner,
// fa_decode_combine_ragged_kernel), written again here: they are static to that translation unit, whose text is a recorded
// surface (tests/test_host_scaffold.py), and its combine kernel takes its width as a template argument, which would put a
// <512, T> instance among the rectangular kernels' names.
FA_DEVINL int latent_ragged_len(const int* cu_q, int b, int total_q, int* q0) {
  *q0 = min(max(cu_q[b], 0), total_q);
  return min(max(cu_q[b + 1], *q0), total_q) - *q0;
}

// The packed append: kv_new [total_q, 576], packed row t of sequence b (the last b with cu_q[b] <= t, found by bisection: cu_q
// ascends unless it is malformed) goes to cache row seqlens[b] + (t - cu_q[b]) through the table, one 16-byte chunk per thread.
// A row no sequence owns -- the padding at or past cu_q[B], or anything a malformed cu_q leaves -- is dropped before it is read,
// as is a row past the table or one whose table entry is outside the pool.
template <typename TAG, typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_ragged_kernel(LatentRaggedParams p) {
  static_assert(std::is_same<TAG, Latent>::value, "the latent overload");
  constexpr int cpr = kMlaRowB / 16;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.total_q * cpr) return;
  const int c = (int)(item % cpr), t = (int)(item / cpr);
  if (p.cu_q[0] > t) return;
  int lo = 0, hi = p.B;   // cu_q[lo] <= t, and lo is the last such index below hi
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.cu_q[mid] <= t) lo = mid; else hi = mid;
  }
  int q0;
  const int S = latent_ragged_len(p.cu_q, lo, p.total_q, &q0);
  const int j = t - q0;
  if (j < 0 || j >= S) return;
  const int dst = p.seqlens[lo] + j;
  if (dst < 0 || dst >= p.Scache) return;
  const int pi = dst / p.page_size;
  const int page = p.table[(long long)lo * p.bt_stride + pi];
  if ((unsigned)page >= (unsigned)p.num_pages) return;
  *(u32x4*)((char*)p.kv + page * p.kv_ps + (long long)(dst - pi * p.page_size) * p.kv_rs + c * 16) =
      *(const u32x4*)((const char*)p.kv_new + (long long)t * kMlaRowB + c * 16);
}

// The combine by packed row: row = head * total_q + packed row, fa_decode_combine_ragged_kernel's arithmetic at D = 512 (the
// width is a constant in here, not a template argument).  Rows at or past the end of the last sequence (plan[1], written by the
// plan kernel) are the padding of a captured step: they are skipped, whatever the workspace holds.
template <typename TAG, typename T>
__global__ __launch_bounds__(256) void fa_decode_combine_ragged_kernel(LatentRaggedParams p) {
  static_assert(std::is_same<TAG, Latent>::value, "the latent overload");
  constexpr int D = kMlaDv, TPR = D / 4, RPB = 256 / TPR;
  const int total_q = p.total_q;
  const long long R = (long long)p.H * total_q;
  const long long ridx = (long long)blockIdx.x * RPB + threadIdx.x / TPR;
  if (ridx >= R) return;
  const int head = (int)(ridx / total_q), row = (int)(ridx - (long long)head * total_q);
  if (row >= min(p.plan[1], total_q)) return;
  const int d4 = (threadIdx.x % TPR) * 4, n = p.nsplit;
  const float* ml = p.ws + (long long)n * R * D;
  float mx = -INFINITY;
#pragma unroll 8
  for (int s = 0; s < n; ++s) mx = __builtin_fmaxf(mx, ml[2 * (s * R + ridx)]);
  const float mo = mx == -INFINITY ? 0.f : mx;
  float ls = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int s = 0; s < n; ++s) {
    const long long pr = s * R + ridx;
    const float e = __builtin_amdgcn_exp2f(ml[2 * pr] - mo);
    ls += e * ml[2 * pr + 1];
    acc += e * *(const f32x4*)(p.ws + pr * D + d4);
  }
  const float inv = ls > 0.f ? 1.f / ls : 0.f;
  typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
  e4 ov;
#pragma unroll
  for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
  *(u32x2*)((char*)p.o + (long long)head * p.lo.sh + (long long)row * p.lo.rs + d4 * 2) = __builtin_bit_cast(u32x2, ov);
  if (d4 == 0 && p.lse) p.lse[ridx] = ls > 0.f ? (mx + __builtin_log2f(ls)) * kLn2 : -INFINITY;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// Split count: up to two workgroups per CU (512 over (sequence, row block, split)) and splits of at least sqrt(16 * S_cache)
// keys (n <= sqrt(S_cache / 16)), at most 64.  A rule of its own, not the D = 128 one: as at D = 256 every step ends at a
// workgroup barrier and a workgroup takes ONE tile per step here, so a split streams its keys at a quarter of the D = 128
// rate and the machine fills only once the budget is used.  DESIGN.md section 3 has the forced-split sweep behind it
// (profiles/mla_split_sweep.jsonl) and how far the rule lies from the best swept count at each point.
int mla_splits(long long wgs, int S_cache, int forced) {
  if (forced > 0) return forced;
  constexpr int kMaxSplits = 64, kTargetWgs = 512, kKeys = 16;
  wgs = std::max<long long>(1, wgs);
  long long n = (kTargetWgs + wgs - 1) / wgs;
  long long by_len = 1;
  while ((by_len + 1) * (by_len + 1) * kKeys <= S_cache) ++by_len;
  n = std::min(n, by_len);
  return (int)std::max<long long>(1, std::min<long long>(n, kMaxSplits));
}

template <typename T>
static hipError_t launch_decode_mla_t(const MlaParams& p, hipStream_t s) {
  if (p.Snew > 0) {
    const long long items = (long long)p.B * p.Snew * (kMlaRowB / 16);
    hipLaunchKernelGGL((fa_kvcache_append_paged_kernel<MLA, T>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p);
    if (hipError_t e = hipGetLastError()) return e;
  }
  const long long wgs = (long long)p.B * decode_row_blocks(p.H, p.Sq);
  if (hipError_t e = launch_kernel<fa_decode_paged_kernel<MLA, T>>((unsigned)(wgs * p.nsplit), 256, MlaCfg::LDS_BYTES, s, p)) return e;
  if (p.nsplit <= 1) return hipSuccess;
  // the shared combine kernel reads the workspace, the split count and O / LSE from the decode calls' parameter block
  DecodeParams d{};
  d.o = p.o;
  d.lse = p.lse;
  d.ws = p.ws;
  d.lo = p.lo;
  d.B = p.B;
  d.H = p.H;
  d.Sq = p.Sq;
  d.D = kMlaDv;
  d.nsplit = p.nsplit;
  const long long rows = (long long)p.B * p.H * p.Sq, rpb = 256 / (kMlaDv / 4);
  hipLaunchKernelGGL((fa_decode_combine_kernel<kMlaDv, T>), dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, s, d);
  return hipGetLastError();
}

hipError_t launch_decode_mla(const MlaParams& p, int dtype, hipStream_t s) {
  return dtype == 1 ? launch_decode_mla_t<BF16>(p, s) : launch_decode_mla_t<FP16>(p, s);
}

// The packed step: the grid is sized from total_q and B alone (p.nb_max = ragged_nb_max(H, total_q, B)), never from the longest
// sequence, and nothing here reads device memory.
template <typename T>
static hipError_t launch_decode_mla_ragged_t(const LatentRaggedParams& p, hipStream_t s) {
  const DecodeRagged rd{p.cu_q, p.total_q, p.plan, p.nb_max};
  if (hipError_t e = launch_ragged_plan(p.cu_q, p.B, /*group=*/p.H, rd, s)) return e;
  if (p.Snew) {
    const long long items = (long long)p.total_q * (kMlaRowB / 16);
    hipLaunchKernelGGL((fa_kvcache_append_ragged_kernel<Latent, T>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (hipError_t e = launch_kernel<fa_decode_ragged_kernel<Latent, T>>((unsigned)((long long)p.nb_max * p.nsplit), 256,
                                                                     MlaCfg::LDS_BYTES, s, p))
    return e;
  if (p.nsplit <= 1) return hipSuccess;
  const long long rows = (long long)p.H * p.total_q, rpb = 256 / (kMlaDv / 4);
  hipLaunchKernelGGL((fa_decode_combine_ragged_kernel<Latent, T>), dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_decode_mla_ragged(const LatentRaggedParams& p, int dtype, hipStream_t s) {
  return dtype == 1 ? launch_decode_mla_ragged_t<BF16>(p, s) : launch_decode_mla_ragged_t<FP16>(p, s);
}

}  // namespace fa
