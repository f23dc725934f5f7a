"""CPU: the slice rule of the weight warming (csrc/warm.h, warm_slice) walked exhaustively by a small g++ program.

The rule: the ranges of a Warm are concatenated into one space of 128-byte lines (a line counts when a 4-byte load at its start
stays inside its range); workgroup wg belongs to XCD wg & 7 and is number wg >> 3 there; the nx workgroups of an XCD walk the
line space with stride nx * threads for at most 4 steps.  So, for every XCD that has a workgroup, every line is touched exactly
once when the lines fit in 4 * nx * threads, otherwise exactly the prefix of that length; an XCD without a workgroup, an
all-zero Warm and a workgroup or thread outside the launch touch nothing; every offset is 4-byte aligned with its 4 bytes inside
the range.  The program restates the line space on its own and compares."""
import os
import subprocess

from conftest import ROOT

SRC = r"""
#include "warm.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace mdm;

static const int64_t SIZES[] = {0, 4, 127, 128, 129, 524288, 1572864, 4194304 + 64};
static long checked = 0;

static int fail(const char* what, int nwg, int nth, int cfg, long a, long b) {
  std::printf("FAIL %s: nwg %d threads %d config %d: %ld %ld\n", what, nwg, nth, cfg, a, b);
  return 1;
}

static int check(const Warm& w, int nwg, int nth, int cfg) {
  // the line space, restated: range r holds the lines l with 128 l + 4 <= bytes[r]
  int64_t first[WARM_RANGES + 1];
  first[0] = 0;
  for (int r = 0; r < WARM_RANGES; ++r) {
    int64_t n = 0;
    if (w.p[r])
      while (128 * n + 4 <= w.bytes[r]) ++n;
    first[r + 1] = first[r] + n;
  }
  const int64_t total = first[WARM_RANGES];
  for (int x = 0; x < 8; ++x) {
    std::vector<int> hits(total, 0);
    int nx = 0;
    for (int wg = x; wg < nwg; wg += 8) {
      ++nx;
      for (int tid = 0; tid < nth; ++tid)
        for (int k = 0; k < WARM_MAX_STEPS; ++k) {
          const WarmSlice s = warm_slice(w, wg, nwg, tid, nth, k);
          if (s.range < 0) continue;
          if (s.range >= WARM_RANGES || !w.p[s.range]) return fail("range", nwg, nth, cfg, s.range, 0);
          if (s.offset < 0 || (s.offset & 3) || s.offset >= w.bytes[s.range] || s.offset + 4 > w.bytes[s.range])
            return fail("offset", nwg, nth, cfg, s.range, (long)s.offset);
          if (s.offset % 128) return fail("not a line start", nwg, nth, cfg, s.range, (long)s.offset);
          const int64_t line = first[s.range] + s.offset / 128;
          if (line >= first[s.range + 1]) return fail("line outside its range", nwg, nth, cfg, s.range, (long)line);
          ++hits[line];
          ++checked;
        }
    }
    const int64_t reach = (int64_t)WARM_MAX_STEPS * nx * nth;
    const int64_t want = total < reach ? total : reach;  // everything, or exactly the prefix
    for (int64_t l = 0; l < total; ++l)
      if (hits[l] != (l < want ? 1 : 0)) return fail("coverage", nwg, nth, cfg, (long)l, hits[l]);
    if (nx == 0)  // (no workgroup: the loop above made no call; the rule must also refuse a workgroup the launch does not have)
      for (int tid = 0; tid < nth; tid += 37)
        for (int k = 0; k < WARM_MAX_STEPS; ++k)
          if (warm_slice(w, nwg + x, nwg, tid, nth, k).range >= 0) return fail("workgroup outside the launch", nwg, nth, cfg, x, k);
  }
  // outside the launch, outside the steps
  if (warm_slice(w, 0, nwg, nth, nth, 0).range >= 0 || warm_slice(w, 0, nwg, -1, nth, 0).range >= 0 ||
      warm_slice(w, 0, nwg, 0, nth, WARM_MAX_STEPS).range >= 0 || warm_slice(w, -1, nwg, 0, nth, 0).range >= 0 ||
      warm_slice(w, nwg, nwg, 0, nth, 0).range >= 0)
    return fail("outside", nwg, nth, cfg, 0, 0);
  return 0;
}

int main() {
  static_assert(WARM_MAX_STEPS == 4 && WARM_RANGES == 6 && WARM_XCDS == 8, "the rule the test restates");
  const int NWG[] = {1, 7, 8, 9, 197, 253, 256, 784}, NTH[] = {256, 512};
  // byte counts per configuration (index into SIZES; -1 = no range in that slot): each count alone, then two to six ranges
  const int CFG[][WARM_RANGES] = {
      {0, -1, -1, -1, -1, -1}, {1, -1, -1, -1, -1, -1}, {2, -1, -1, -1, -1, -1}, {3, -1, -1, -1, -1, -1}, {4, -1, -1, -1, -1, -1},
      {5, -1, -1, -1, -1, -1}, {6, -1, -1, -1, -1, -1}, {7, -1, -1, -1, -1, -1}, {4, 1, -1, -1, -1, -1},  {6, 5, -1, -1, -1, -1},
      {1, 0, 4, -1, -1, -1},   {6, 5, 5, 3, -1, -1},    {5, 0, 2, 4, 1, -1},     {6, 5, 5, 3, 3, 3},      {7, 6, 5, 4, 2, 1},
      {0, 0, 0, 0, 0, 0},      {-1, -1, -1, -1, -1, -1}, {-1, 5, -1, 4, -1, 1}};
  int ncfg = 0;
  for (const auto& c : CFG) {
    Warm w = {};
    for (int r = 0; r < WARM_RANGES; ++r)
      if (c[r] >= 0) w.p[r] = (const void*)(uintptr_t)(0x100000 * (r + 1)), w.bytes[r] = SIZES[c[r]];  // never dereferenced
    for (int nwg : NWG)
      for (int nth : NTH)
        if (check(w, nwg, nth, ncfg)) return 1;
    ++ncfg;
  }
  // all zero touches nothing; warm_add fills from the front and drops what does not fit or is empty
  Warm z = {};
  for (int k = 0; k < WARM_MAX_STEPS; ++k)
    if (warm_slice(z, 0, 256, 0, 512, k).range >= 0) return fail("all-zero Warm", 256, 512, -1, k, 0);
  Warm a = {};
  int dummy[8];
  warm_add(a, nullptr, 64), warm_add(a, dummy, 0), warm_add(a, dummy, 3);
  if (a.p[0]) return fail("warm_add kept an empty range", 0, 0, -1, 0, 0);
  for (int i = 0; i < 8; ++i) warm_add(a, dummy + i, 4);
  for (int r = 0; r < WARM_RANGES; ++r)
    if (a.p[r] != dummy + r || a.bytes[r] != 4) return fail("warm_add order", 0, 0, -1, r, 0);
  std::printf("ok %d configurations, %ld touches checked\n", ncfg, checked);
  return 0;
}
"""


def test_slice_rule_covers_every_line_once_per_xcd(tmp_path):
    src = tmp_path / "warm_walk.cpp"
    src.write_text(SRC)
    exe = tmp_path / "warm_walk"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "motiondiffusion-moe_amd", "csrc"),
                           str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 18 configurations")
