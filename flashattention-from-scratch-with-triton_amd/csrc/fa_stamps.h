// -DFA_STAMPS diagnostic builds (tools/stamps*.py): a per-phase cycle account of every wave, written to the `dbg` pointer of
// the parameter block.  A kernel opens with FA_STAMPS_BEGIN(number of segments), closes a phase with FA_STAMP(segment) and
// at its end writes its record -- stamp_record(): `words` 64-bit words per wave; which word holds what is the kernel's own
// layout, the tools read it -- with the elapsed clocks from FA_STAMPS_END.  Release builds compile all of it to nothing.
// -DFA_STAMPS_ITER (with FA_STAMPS) turns on the per-block-iteration stamps, FA_ISTAMP.
#pragma once
#include "fa_common.h"

#ifdef FA_STAMPS
namespace fa {
struct StampClocks {
  unsigned long long clk, rt;   // shader clock, constant-rate realtime counter
};
// (__device__ functions: an asm statement with a register constraint written in a __global__ body, see fa_common.h keep_live)
FA_DEVINL unsigned long long stamp_clock() {
  unsigned long long now;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
  return now;
}
FA_DEVINL unsigned long long stamp_clock_after_stores() {   // ... once the wave's global stores are out
  unsigned long long now;
  asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
  return now;
}
FA_DEVINL StampClocks stamp_clocks() {
  StampClocks c;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(c.clk), "=s"(c.rt)::"memory");
  return c;
}
FA_DEVINL unsigned long long* stamp_record(void* dbg, int wave, int words) {
  return (unsigned long long*)dbg + ((size_t)blockIdx.x * 4 + wave) * words;
}
}  // namespace fa
#define FA_STAMPS_BEGIN(NSEG)                       \
  const StampClocks stamps_t0_ = stamp_clocks();    \
  unsigned long long seg[NSEG] = {}, last_ = stamps_t0_.clk
#define FA_STAMP(slot)                                \
  do {                                                \
    __builtin_amdgcn_sched_barrier(0);                \
    const unsigned long long now_ = stamp_clock();    \
    __builtin_amdgcn_sched_barrier(0);                \
    seg[slot] += now_ - last_;                        \
    last_ = now_;                                     \
  } while (0)
// d[CLK] = shader clocks, d[CLK + 1] = realtime ticks since FA_STAMPS_BEGIN
#define FA_STAMPS_END(d, CLK)                         \
  do {                                                \
    const StampClocks stamps_t1_ = stamp_clocks();    \
    (d)[CLK] = stamps_t1_.clk - stamps_t0_.clk;       \
    (d)[(CLK) + 1] = stamps_t1_.rt - stamps_t0_.rt;   \
  } while (0)
#else
#define FA_STAMP(slot) do {} while (0)
#endif
#ifdef FA_STAMPS_ITER
#define FA_ISTAMP(slot) FA_STAMP(slot)
#else
#define FA_ISTAMP(slot) do {} while (0)
#endif
