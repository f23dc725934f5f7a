// Weight warming: a launch touches the read-only bytes the NEXT launch of the step reads first (its weight stream, then the small
// fp32 vectors on its dependent chain), so that launch does not open with misses on addresses known a whole launch earlier.
// A touch is one 4-byte load per 128-byte line whose value is discarded; nothing is written and no result depends on it.
//
// The slice rule (warm_slice) is plain C++: it compiles for the host and the device under hipcc and under g++
// (tests/test_weight_warm_host.py walks it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MDM_WARM_HD __host__ __device__
#else
#define MDM_WARM_HD
#endif

namespace mdm {

constexpr int WARM_RANGES = 6;
constexpr int WARM_LINE = 128;     // bytes per touched line
constexpr int WARM_MAX_STEPS = 4;  // touches per thread at most
// Coverage: every XCD that runs a workgroup of the launch touches every line once, into its own L2 (workgroup wg runs on XCD
// wg & 7: the round-robin dispatch xcd_remap relies on).  Chip-wide single coverage (1 here: the whole grid touches every line
// once, which warms the Infinity Cache only) measured nine tenths of the gain.
constexpr int WARM_XCDS = 8;

struct Warm {  // up to six read-only ranges, all zero = nothing
  const void* p[WARM_RANGES];
  int64_t bytes[WARM_RANGES];
};

struct WarmSlice {
  int range;       // -1: nothing to touch
  int64_t offset;  // byte offset into the range: a multiple of 128 with offset + 4 <= bytes[range]
};

// lines of a range: a line counts when a 4-byte load at its start stays inside the range
MDM_WARM_HD inline int64_t warm_lines(int64_t bytes) { return bytes < 4 ? 0 : (bytes + (WARM_LINE - 4)) / WARM_LINE; }

// The line thread `tid` of workgroup `wg` (of `nwg`, `nthreads` threads each) touches at step k.  The ranges are concatenated
// into one space of lines; the nx workgroups of an XCD walk it with stride nx * nthreads, at most WARM_MAX_STEPS steps: where
// the lines exceed WARM_MAX_STEPS * nx * nthreads only that prefix is touched (the head of a stream is what its reader needs first).
MDM_WARM_HD inline WarmSlice warm_slice(const Warm& w, int wg, int nwg, int tid, int nthreads, int k) {
  const WarmSlice none = {-1, 0};
  if (k < 0 || k >= WARM_MAX_STEPS || wg < 0 || wg >= nwg || tid < 0 || tid >= nthreads) return none;
  // everything down to `first` is the same for the whole workgroup: on the device it is scalar work, and a workgroup whose
  // step lies past the last line leaves here
  const int x = wg % WARM_XCDS, j = wg / WARM_XCDS;
  const int64_t nx = (nwg - x + WARM_XCDS - 1) / WARM_XCDS;  // workgroups of this XCD
  const int64_t first = ((int64_t)k * nx + j) * nthreads;
  int64_t n[WARM_RANGES], total = 0;
  for (int r = 0; r < WARM_RANGES; ++r) total += n[r] = w.p[r] ? warm_lines(w.bytes[r]) : 0;
  if (first >= total) return none;
  const int64_t line = first + tid;
  WarmSlice s = {-1, 0};
  int64_t start = 0;  // the last non-empty range that starts at or before the line holds it
  for (int r = 0; r < WARM_RANGES; ++r) {
    if (n[r] > 0 && line >= start) s.range = r, s.offset = start;
    start += n[r];
  }
  if (line >= total) return none;
  s.offset = (line - s.offset) * WARM_LINE;
  return s;
}

#if defined(__HIPCC__)
// One 4-byte vector load per line of this thread's slice.  The loads are plain C++ (the compiler's wait-count insertion tracks
// them) and nothing waits for them where they are issued: their values travel in the token to warm_done() at the end of the
// kernel, which is their only use.  (A volatile load would not do: it is compiled to a system-scope load with a wait for it right
// behind it, four round trips to memory in a row.)
struct WarmTok {
  uint32_t v[WARM_MAX_STEPS];
};
__device__ __forceinline__ WarmTok warm_touch(const Warm& w, int wg, int nwg, int tid, int nthreads) {
  WarmTok t = {};
  uintptr_t any = 0;
#pragma unroll
  for (int r = 0; r < WARM_RANGES; ++r) any |= (uintptr_t)w.p[r];
  if (!any) return t;
#pragma unroll
  for (int k = 0; k < WARM_MAX_STEPS; ++k) {
    const WarmSlice s = warm_slice(w, wg, nwg, tid, nthreads, k);
    if (s.range < 0) continue;
    const uint8_t* base = (const uint8_t*)w.p[0];  // (selected, not indexed: a kernel argument indexed at run time would move to scratch)
#pragma unroll
    for (int r = 1; r < WARM_RANGES; ++r) base = s.range == r ? (const uint8_t*)w.p[r] : base;
    t.v[k] = *(const __attribute__((address_space(1))) uint32_t*)(uintptr_t)(base + s.offset);
  }
  return t;
}
// the end of the touches' life: keeps the loads (their values are "used" here) without an instruction
__device__ __forceinline__ void warm_done(const WarmTok& t) {
#pragma unroll
  for (int k = 0; k < WARM_MAX_STEPS; ++k) asm volatile("" ::"v"(t.v[k]));
}
#endif

// host side: append a range (ignored when null, empty or when the six are taken)
inline void warm_add(Warm& w, const void* p, int64_t bytes) {
  if (!p || bytes < 4) return;
  for (int r = 0; r < WARM_RANGES; ++r)
    if (!w.p[r]) {
      w.p[r] = p, w.bytes[r] = bytes;
      return;
    }
}

}  // namespace mdm
