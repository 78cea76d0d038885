// Top-k selection from indexer logits (include_mla_select/mi355fa_mla_select.h): per row (b, i) of fp32 logits [B, S_q, W] the
// min(topk, #candidates) best columns, written in ASCENDING column order, then -1 up to topk.  A column is a candidate when it is
// below the row's length and its value is neither -inf nor NaN; candidates are ordered by value descending (-0.0 == +0.0, +inf an
// ordinary largest value), ties by lower column first.  Exact, unique and the same bits on every launch.
//
// Who does what (fa_decode_paged_kernel<IdxSelect, RowHome>).  grid = (S_q, B): ONE workgroup of 256 lanes owns one row, and no
// workgroup ever waits for another -- no flag, no ticket.  The row is addressed in "shifted" columns u = t + off, off = the
// row's distance (0..3 elements) from the 16-byte boundary below it, so that vector v = columns u in [4v, 4v + 4) is one aligned
// 16-byte load; a vector that is not wholly inside [0, n) is read element by element under its guard (the peel), so nothing at
// or past the row's length n = clamp(lengths[b], 0, W) is ever read.  A lane's loads are requested without a branch between them
// and only then turned into keys (SelRowGlobal): one wave per SIMD has nothing else to hide their latency behind.
//
//   1 keys     fp32 -> uint32, order-preserving: -0.0 folded into +0.0 on the bits, all bits flipped where the sign is set, the
//              sign bit set otherwise.  Valid keys are [0x00800000 (-FLT_MAX), 0xff800000 (+inf)]; -inf, both NaN ranges and
//              columns outside [0, n) become key 0, which nothing selects.  The same pass counts the top 11 bits of every valid
//              key into a 2048-bin LDS histogram (ds_add_u32) and -- RowHome::kLds -- stores the keys to LDS, so that the row
//              crosses HBM / L2 exactly once.  Sixteen 16-byte loads are in flight per lane.
//   2 coarse   sel_find: a suffix sum from the top bin -- each lane adds its bins, a 6-step wave scan, the wave totals through
//              LDS -- gives the number of candidates (k_eff = min(topk, that)), the threshold bin d, the count strictly above it
//              and the number r still owed from inside it.  No more candidates than topk: every candidate is taken, T = 0.
//   3 refine   the keys of bin d are compacted into an LDS buffer (their order in it is whatever the slot counter gave, and
//              nothing depends on it: the buffer is only ever counted) and the remaining 21 bits fall in radix steps of 8, 8 and
//              5 bits over a 256-bin histogram, to the exact threshold key T and the number r_T of T-valued columns to take.  A
//              bin that does not fit the buffer (an all-equal row) runs the same three steps over the row itself under the
//              prefix found so far: one row pass per step, still exact.  Histogram counts do not depend on the order in which
//              the atomics land, so neither path does.
//   4 emit     the row once more in ascending columns, 4096 a step (four vectors a lane): ballots and mbcnt count the `key > T` and `key == T`
//              columns of the wave's lower lanes, the waves' totals (16 + 16 bit) go through LDS: the numbers of both kinds before each column;
//              a running base carries them across steps.  Column t goes to position gt_before + min(eq_before, r_T), an equal
//              one only while eq_before < r_T: ascending order and the lower-column-first tie rule are the scan's own, and no
//              position comes from an atomic.  The walk ends once k_eff columns are out; then -1 from k_eff to topk.
//
// LDS (static): keys 32772 * 4 (kLds only), histogram 8 KiB, candidate buffer 16 KiB (kLds) or 64 KiB (kGlobal), 144 bytes of
// scan state: 155 808 bytes resident, 73 872 streaming.  Plain C++, vector loads and stores, LDS atomics only.
#include <stdint.h>

#include "fa_common.h"
#include "fa_mla_select.h"

namespace fa {
namespace {

// the order-preserving key of the fp32 bits `b`; 0 = hidden
FA_DEVINL unsigned sel_key(unsigned b) {
  if (b == 0x80000000u) b = 0u;
  const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return k - 0x00800000u <= 0xff800000u - 0x00800000u ? k : 0u;
}

// The row in global memory: `base` = the row's address rounded down to 16 bytes, column t at base[t + off].  Vectors [v_lo, v_hi)
// lie wholly inside [0, n) and are read by one 16-byte load; the one before and the one after (the peel) element by element.
// A request is split in two so that a lane's loads all leave before the first is waited for: raw() has no branch -- a vector
// outside [v_lo, v_hi) re-reads the nearest one inside --, finish() turns the bits into keys, 0 where the column is outside
// [0, n), and alone reads the peel.  Nothing at or past n is ever read.
struct SelRowGlobal {
  const float* base;
  int off, n, v_lo, v_hi, nv;
  FA_DEVINL bool any() const { return v_hi > v_lo; }
  FA_DEVINL u32x4 raw(int v) const { return *(const u32x4*)(base + 4 * (size_t)min(max(v, v_lo), v_hi - 1)); }
  FA_DEVINL u32x4 finish(int v, u32x4 w) const {
    const bool in = v >= v_lo && v < v_hi;
    u32x4 k;
#pragma unroll
    for (int e = 0; e < 4; ++e) k[e] = in ? sel_key(w[e]) : 0u;
    if (!in && v < nv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = 4 * v - off + e;
        if (t >= 0 && t < n) k[e] = sel_key(__builtin_bit_cast(unsigned, base[4 * (size_t)v + e]));
      }
    }
    return k;
  }
};

// The row's keys in LDS, as pass 1 stored them: whole vectors, 0 where hidden
struct SelRowLds {
  const unsigned* keys;
  int nv;
  FA_DEVINL bool any() const { return true; }
  FA_DEVINL u32x4 raw(int v) const { return *(const u32x4*)(keys + 4 * min(v, max(nv - 1, 0))); }
  FA_DEVINL u32x4 finish(int v, u32x4 w) const { return v < nv ? w : u32x4{0u, 0u, 0u, 0u}; }
};

// the bits of vectors v0 + 256 j, j < N: N loads with no branch between them
template <int N, typename Row>
FA_DEVINL void sel_request(const Row& row, int v0, u32x4 (&w)[N]) {
  if (row.any()) {
#pragma unroll
    for (int j = 0; j < N; ++j) w[j] = row.raw(v0 + j * kSelThreads);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) w[j] = u32x4{0u, 0u, 0u, 0u};
  }
}

// f(key) for every valid key of the row, kSelFlight vectors in flight per lane, in no particular order
template <typename Row, typename F>
FA_DEVINL void sel_for_each(const Row& row, int nv, int tid, F&& f) {
  for (int v0 = tid; v0 < nv; v0 += kSelFlight * kSelThreads) {
    u32x4 w[kSelFlight];
    sel_request(row, v0, w);
#pragma unroll
    for (int j = 0; j < kSelFlight; ++j) {
      const u32x4 k = row.finish(v0 + j * kSelThreads, w[j]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k[e]) f(k[e]);
    }
  }
}

// inclusive sum over the lanes of a wave
FA_DEVINL unsigned sel_wave_scan(unsigned x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(x, d);
    if (lane >= d) x += o;
  }
  return x;
}

// the set bits of a ballot below this lane
FA_DEVINL unsigned sel_lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

struct SelFound {
  int digit;        // the bin that holds the k-th largest key, k = min(k_req, total)
  int above;        // keys in the bins above it
  int count;        // keys in it
  int total;        // keys in all bins
};

// The k_req-th key from the top of hist[0, NB): bins are summed from the top, lane `tid` owning NB / 256 of them (one, or none
// past NB).  wsum: kSelWaves words, res: 3 words.  Two barriers; the caller's next write to hist, wsum or res comes after
// another.  Exactly one lane finds prefix < k <= prefix + its own bins.
template <int NB>
FA_DEVINL SelFound sel_find(const unsigned* hist, unsigned* wsum, unsigned* res, int k_req, int tid) {
  constexpr int BPT = NB >= kSelThreads ? NB / kSelThreads : 1;
  const int lane = tid & 63, wave = tid >> 6, first = tid * BPT;
  unsigned mine = 0;
  if (first < NB)
#pragma unroll
    for (int j = 0; j < BPT; ++j) mine += hist[NB - 1 - (first + j)];
  const unsigned incl = sel_wave_scan(mine, lane);
  if (lane == 63) wsum[wave] = incl;
  if (tid == 0) res[0] = res[1] = res[2] = 0u;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kSelWaves; ++w) {
    const unsigned s = wsum[w];
    before += w < wave ? s : 0u;
    total += s;
  }
  const unsigned k = min((unsigned)k_req, total);
  unsigned a = before + incl - mine;
  if (a < k && k <= a + mine) {
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const unsigned c = hist[NB - 1 - (first + j)];
      if (a < k && k <= a + c) res[0] = NB - 1 - (first + j), res[1] = a, res[2] = c;
      a += c;
    }
  }
  __syncthreads();
  return SelFound{(int)res[0], (int)res[1], (int)res[2], (int)total};
}

}  // namespace

template <typename Tag, RowHome H>
__global__ __launch_bounds__(kSelThreads) void fa_decode_paged_kernel(const SelectParams p) {
  constexpr bool RES = H == RowHome::kLds;
  constexpr int CAP = RES ? kSelCandLds : kSelCandGlobal;
  __shared__ __attribute__((aligned(16))) unsigned keys[RES ? kSelResidentW + 4 : 4];
  __shared__ unsigned hist[kSelBins];
  __shared__ unsigned cand[CAP];
  __shared__ unsigned wsum[2][kSelEmitVecs * kSelWaves];   // the emit's two alternating sets; [0] is sel_find's before it
  __shared__ unsigned res[4];               // sel_find's answer; [3]: the slot counter of the compaction
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, i = blockIdx.x;
  const float* rowp = p.logits + (long long)b * p.l_sb + (long long)i * p.l_ss;
  int* out = p.out + (long long)b * p.o_sb + (long long)i * p.o_ss;
  const int n = p.lengths ? min(max(p.lengths[b], 0), p.W) : p.W;
  const int off = (int)(((uintptr_t)rowp >> 2) & 3);
  const int nv = n > 0 ? (n + off + 3) >> 2 : 0;
  const SelRowGlobal grow{rowp - off, off, n, off ? 1 : 0, (n + off) >> 2, nv};

  for (int e = tid; e < kSelBins; e += kSelThreads) hist[e] = 0u;
  if (tid == 0) res[3] = 0u;
  __syncthreads();

  // 1: keys, the coarse histogram, and (resident) the row into LDS
  for (int v0 = tid; v0 < nv; v0 += kSelFlight * kSelThreads) {
    u32x4 w[kSelFlight];
    sel_request(grow, v0, w);
#pragma unroll
    for (int j = 0; j < kSelFlight; ++j) {
      const int v = v0 + j * kSelThreads;
      const u32x4 k = grow.finish(v, w[j]);
      if constexpr (RES)
        if (v < nv) *(u32x4*)(keys + 4 * v) = k;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k[e]) atomicAdd(&hist[k[e] >> (32 - kSelCoarseBits)], 1u);
    }
  }
  __syncthreads();
  const auto row = [&] {
    if constexpr (RES)
      return SelRowLds{keys, nv};
    else
      return grow;
  }();

  // 2: the coarse digit
  const SelFound c = sel_find<kSelBins>(hist, wsum[0], res, p.topk, tid);
  const int k_eff = min(p.topk, c.total);
  unsigned T = 0u;   // every valid key is above 0: all candidates, no ties to split
  int rT = 0;
  if (c.total > p.topk) {
    // 3: the other 21 bits
    unsigned prefix = (unsigned)c.digit;
    int r = k_eff - c.above;
    const int nb = c.count;
    const bool fits = nb <= CAP;
    if (fits) {
      sel_for_each(row, nv, tid, [&](unsigned key) {
        if (key >> (32 - kSelCoarseBits) == prefix) {
          const unsigned slot = atomicAdd(&res[3], 1u);
          if (slot < (unsigned)CAP) cand[slot] = key;
        }
      });
    }
    int known = kSelCoarseBits;
#pragma unroll
    for (int level = 0; level < 3; ++level) {
      const int bits = level < 2 ? 8 : 32 - kSelCoarseBits - 16;
      const int shift = 32 - known - bits;
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();   // (and the compaction is complete)
      const auto tally = [&](unsigned key) {
        if (key >> (shift + bits) == prefix) atomicAdd(&hist[(key >> shift) & ((1u << bits) - 1u)], 1u);
      };
      if (fits) {
        for (int e = tid; e < nb; e += kSelThreads) tally(cand[e]);
      } else {
        sel_for_each(row, nv, tid, tally);
      }
      __syncthreads();
      const SelFound f = sel_find<256>(hist, wsum[0], res, r, tid);
      prefix = (prefix << bits) | (unsigned)f.digit;
      r -= f.above;
      known += bits;
    }
    T = prefix;
    rT = r;
  }

  // 4: emit in ascending columns: kSelEmitVecs vectors per lane and step, vector j of lane l at column block j * 256 + l of the
  // step -- 4 * kSelEmitVecs "virtual waves" in column order, their totals through LDS
  constexpr int EV = kSelEmitVecs, VW = EV * kSelWaves;
  int gt_base = 0, eq_base = 0;
  u32x4 cur[EV];
  sel_request(row, tid, cur);
#pragma unroll
  for (int j = 0; j < EV; ++j) cur[j] = row.finish(j * kSelThreads + tid, cur[j]);
  for (int s = 0; s * EV * kSelThreads < nv; ++s) {
    const int v0 = s * EV * kSelThreads + tid;
    u32x4 nxt[EV];   // the next step's bits, requested ahead of this step's barrier and turned into keys at its end
    unsigned below[EV], before[EV];   // packed (`> T` | `== T` << 16) counts: of the wave's lower lanes, of the earlier waves
    sel_request(row, v0 + EV * kSelThreads, nxt);
#pragma unroll
    for (int j = 0; j < EV; ++j) {
      unsigned tot = 0u;
      below[j] = before[j] = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {   // ballot and mbcnt: no LDS round trip inside the wave
        const unsigned long long bg = __ballot(cur[j][e] > T), bq = __ballot(cur[j][e] == T);
        below[j] += sel_lanes_below(bg) + (sel_lanes_below(bq) << 16);
        tot += (unsigned)__popcll(bg) + ((unsigned)__popcll(bq) << 16);
      }
      if (lane == 0) wsum[s & 1][j * kSelWaves + wave] = tot;
    }
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < VW; ++w) {
      const unsigned x = wsum[s & 1][w];
#pragma unroll
      for (int j = 0; j < EV; ++j) before[j] += w < j * kSelWaves + wave ? x : 0u;
      total += x;
    }
#pragma unroll
    for (int j = 0; j < EV; ++j) {
      const unsigned excl = before[j] + below[j];
      int g = gt_base + (int)(excl & 0xffffu), q = eq_base + (int)(excl >> 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = 4 * (v0 + j * kSelThreads) + e - off;
        if (cur[j][e] > T) {
          const int pos = g + min(q, rT);
          if ((unsigned)pos < (unsigned)k_eff) out[pos] = t;
          ++g;
        } else if (cur[j][e] == T) {
          if (q < rT && (unsigned)(g + q) < (unsigned)k_eff) out[g + q] = t;
          ++q;
        }
      }
    }
    gt_base += (int)(total & 0xffffu);
    eq_base += (int)(total >> 16);
    if (gt_base + min(eq_base, rT) >= k_eff) break;
#pragma unroll
    for (int j = 0; j < EV; ++j) cur[j] = row.finish(v0 + (EV + j) * kSelThreads, nxt[j]);
  }
  for (int j = k_eff + tid; j < p.topk; j += kSelThreads) out[j] = -1;
}

hipError_t launch_mla_select(const SelectParams& p, hipStream_t s) {
  const dim3 grid((unsigned)p.Sq, (unsigned)p.B);
  if (p.W <= kSelResidentW)
    hipLaunchKernelGGL((fa_decode_paged_kernel<IdxSelect, RowHome::kLds>), grid, dim3(kSelThreads), 0, s, p);
  else
    hipLaunchKernelGGL((fa_decode_paged_kernel<IdxSelect, RowHome::kGlobal>), grid, dim3(kSelThreads), 0, s, p);
  return hipGetLastError();
}

}  // namespace fa
