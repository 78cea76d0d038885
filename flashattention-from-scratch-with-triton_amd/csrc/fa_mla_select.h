// Top-k selection from indexer logits to the `indices` of the sparse MLA calls (fa_mla_select.hip; C ABI in
// include_mla_select/mi355fa_mla_select.h, argument checks in fa_api_mla_select.hip): the parameter block of its two kernels and
// the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

namespace fa {

constexpr int kSelThreads = 256;                   // one workgroup per row, 4 waves: the library's workgroup size
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelFlight = 16;                     // 16-byte loads a lane has in flight in the counting passes
constexpr int kSelEmitVecs = 4;                    // vectors per lane and emit step: 4096 columns between two barriers
constexpr int kSelCoarseBits = 11;                 // the coarse digit: sign, exponent and two mantissa bits of the key
constexpr int kSelBins = 1 << kSelCoarseBits;
constexpr int kSelResidentW = 32768;               // widest row whose keys stay in LDS (128 KiB of the CU's 160)
constexpr int kSelCandLds = 4096;                  // keys of the threshold bin kept for the refinement: beside a resident row ...
constexpr int kSelCandGlobal = 16384;              // ... and where the row stays in global memory and LDS is free
constexpr int kSelMaxTopk = 65536;

// Where the row's keys live after the first pass: the row accessor of the one kernel body.
enum class RowHome { kLds, kGlobal };

// A tag and a block of their own for the overloads <IdxSelect, RowHome> of fa_decode_paged_kernel: the other decode kernels'
// names are recorded sets, and the race tables claim this stem.
struct IdxSelect {};
struct SelectParams {
  const float* logits;    // fp32 [B, S_q, W] through l_sb / l_ss (elements), rows 4-byte aligned
  const int* lengths;     // int32 [B] or nullptr (every row is W long)
  int* out;               // int32 [B, S_q, topk] through o_sb / o_ss (elements)
  long long l_sb, l_ss, o_sb, o_ss;
  int B, Sq, W, topk;
};

// Enqueue the selection on `s`: the resident kernel where W <= kSelResidentW, the streaming one above.
hipError_t launch_mla_select(const SelectParams& p, hipStream_t s);

}  // namespace fa
