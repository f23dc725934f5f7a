// Row-wise (HBM-bound) kernels of the denoiser: LayerNorm chains, stylization inputs, per-head
// normalisations of the Performer attention, softmaxes, MoE routing and the sampler update.
// One wave (64 lanes) owns one row of D elements; everything stays in fp32.
#include "kernels.h"
#include "moe_gate_row.h"
#include "row.h"

namespace mdm {
namespace {

// ---- LN chain: y1 = LN1(x), y2 = LN2(y1) --------------------------------------------------------
// FMT = the 16-bit format of whichever tensors are 16-bit (1 = bf16, 2 = fp16; one format per launch), a template argument so
// that the conversions are straight-line code and every load of an iteration is issued before the first wait (row.h)
template <int NE, bool VEC, int FMT>
__device__ __forceinline__ void ln_chain_rows(const float* __restrict__ x, bool x_h, int64_t M, int D, const float* w1,
                                              const float* b1, void* y1, int y1_h, const float* w2, const float* b2,
                                              void* y2, int y2_h) {  // y?_h: 0 fp32, 1 16-bit (FMT), 2 x2 rows
  const int lane = threadIdx.x & 63;
  Row<NE, VEC> ww1, bb1, ww2, bb2;
  ww1.load(w1, D, lane), bb1.load(b1, D, lane);
  if (w2) ww2.load(w2, D, lane), bb2.load(b2, D, lane);
  // two rows per wave per iteration: both rows' loads are in flight before either is reduced
  for (int64_t row = 2 * (blockIdx.x * (int64_t)WPB + (threadIdx.x >> 6)); row < M; row += 2 * (int64_t)gridDim.x * WPB) {
    const bool two = row + 1 < M;
    Row<NE, VEC> r, q;
    if (x_h) {
      r.template load_h16<FMT>((const uint16_t*)x + row * D, D, lane);
      q.template load_h16<FMT>((const uint16_t*)x + (two ? row + 1 : row) * D, D, lane);
    } else {
      r.load(x + row * D, D, lane);
      q.load(x + (two ? row + 1 : row) * D, D, lane);
    }
    r.layernorm(ww1, bb1, D, lane);
    q.layernorm(ww1, bb1, D, lane);
    if (y1) {
      r.template store_mode<FMT>(y1, row, D, lane, y1_h);
      if (two) q.template store_mode<FMT>(y1, row + 1, D, lane, y1_h);
    }
    if (w2) {
      r.layernorm(ww2, bb2, D, lane);
      q.layernorm(ww2, bb2, D, lane);
      r.template store_mode<FMT>(y2, row, D, lane, y2_h);
      if (two) q.template store_mode<FMT>(y2, row + 1, D, lane, y2_h);
    }
  }
}
template <int NE, bool VEC>
__global__ __launch_bounds__(256) void ln_chain_kernel(const float* __restrict__ x, int x_bf, int64_t M, int D,
                                                       const float* w1, const float* b1, void* y1, int y1_bf,
                                                       const float* w2, const float* b2, void* y2, int y2_bf) {
  const int m1 = y1_bf == 4 ? 2 : (y1_bf != 0), m2 = y2_bf == 4 ? 2 : (y2_bf != 0);  // 4 = x2 rows (MDM_OP_X2_ROW)
  if (((x_bf | y1_bf | y2_bf) & 3) == 2) {
    ln_chain_rows<NE, VEC, 2>(x, x_bf != 0, M, D, w1, b1, y1, m1, w2, b2, y2, m2);
  } else {
    ln_chain_rows<NE, VEC, 1>(x, x_bf != 0, M, D, w1, b1, y1, m1, w2, b2, y2, m2);
  }
}

// ---- stylization input: s = SiLU( LN_style(a) * (1 + scale[b]) + shift[b] ) ---------------------
// a = x                                               (cross / ffn blocks, stylization.py:29-30)
// a = normalize(LN_post(x)) * sqrt(D)                  (Performer tail, fast_attention.py:169-172)
// a = 0.5 * sum of the 4 routed expert rows            (MoE combine, switch_moe.py:109 + multi_branch.py:58-59)
template <int NE, bool VEC, int FMT>
__device__ __forceinline__ void style_in_rows(const float* __restrict__ x, int64_t M, int D, int S, const float* pw,
                                              const float* pb, const float* sw, const float* sb,
                                              const float* __restrict__ sc, const int* __restrict__ pos4, bool x_h,
                                              void* __restrict__ out, bool out_h) {
  const int lane = threadIdx.x & 63;
  Row<NE, VEC> pww, pbb, sww, sbb;  // requested before the data rows, not after the reductions that precede their use
  if (pw) pww.load(pw, D, lane), pbb.load(pb, D, lane);
  sww.load(sw, D, lane), sbb.load(sb, D, lane);
  for (int64_t row = blockIdx.x * (int64_t)WPB + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * WPB) {
    const float* scb = sc + (row / S) * 2 * (int64_t)D;
    Row<NE, VEC> r, scale, shift;
    scale.load(scb, D, lane);  // first: they depend on the row number only, and must not queue behind the gathered rows' wait
    shift.load(scb + D, D, lane);
    if (pos4) {
      // the token's four routed rows: one 16-byte read of their positions, then all four rows in flight together
      const int p0 = pos4[row * 4 + 0], p1 = pos4[row * 4 + 1], p2 = pos4[row * 4 + 2], p3 = pos4[row * 4 + 3];
      Row<NE, VEC> a, b, c, d;
      if (x_h) {
        const uint16_t* xh = (const uint16_t*)x;
        a.template load_h16<FMT>(xh + (int64_t)p0 * D, D, lane);
        b.template load_h16<FMT>(xh + (int64_t)p1 * D, D, lane);
        c.template load_h16<FMT>(xh + (int64_t)p2 * D, D, lane);
        d.template load_h16<FMT>(xh + (int64_t)p3 * D, D, lane);
      } else {
        a.load(x + (int64_t)p0 * D, D, lane);
        b.load(x + (int64_t)p1 * D, D, lane);
        c.load(x + (int64_t)p2 * D, D, lane);
        d.load(x + (int64_t)p3 * D, D, lane);
      }
#pragma unroll
      for (int j = 0; j < NE; ++j) r.e[j] = ((a.e[j] + b.e[j]) + (c.e[j] + d.e[j])) * 0.5f;
    } else {
      if (x_h) {
        r.template load_h16<FMT>((const uint16_t*)x + row * D, D, lane);
      } else {
        r.load(x + row * D, D, lane);
      }
    }
    if (pw) {
      r.layernorm(pww, pbb, D, lane);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NE; ++j) s += r.e[j] * r.e[j];
      const float inv = sqrtf((float)D) / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
#pragma unroll
      for (int j = 0; j < NE; ++j) r.e[j] *= inv;
    }
    r.layernorm(sww, sbb, D, lane);
#pragma unroll
    for (int j = 0; j < NE; ++j) r.e[j] = silu(r.e[j] * (1.f + scale.e[j]) + shift.e[j]);
    r.template store_to<FMT>(out, row, D, lane, out_h);
  }
}
template <int NE, bool VEC>
__global__ __launch_bounds__(256) void style_in_kernel(const float* __restrict__ x, int64_t M, int D, int S,
                                                       const float* pw, const float* pb,  // optional post_norm
                                                       const float* sw, const float* sb,  // style norm
                                                       const float* __restrict__ sc,      // (B, 2D) scale|shift
                                                       const int* __restrict__ pos4,      // optional (M,4) rows of y2
                                                       int x_bf,                           // 16-bit source rows (format code)
                                                       void* __restrict__ out, int out_bf) {
  if ((x_bf | out_bf) == 2) {
    style_in_rows<NE, VEC, 2>(x, M, D, S, pw, pb, sw, sb, sc, pos4, x_bf != 0, out, out_bf != 0);
  } else {
    style_in_rows<NE, VEC, 1>(x, M, D, S, pw, pb, sw, sb, sc, pos4, x_bf != 0, out, out_bf != 0);
  }
}

// ---- MoE router: both branches' LayerNorm + gate + softmax + top-2 (lowest index wins ties) -----
// F8: the hn rows are e4m3 bytes with per-row scales (p.hn_bf16 == 3); a template argument, so that the other formats' code is
// the code it was (the generic 16-element form already spills registers)
template <int NE, bool VEC, bool F8>
__global__ __launch_bounds__(256) void moe_gate_kernel(const float* __restrict__ x, int64_t M, int D, int E,
                                                       MoeGateParams p) {
  // per-block counters in LDS, flushed with ONE global atomic per (branch, expert) per block: thousands of
  // tokens adding straight into 2E global words serialise at the memory side
  __shared__ int s_hist[32];
  __shared__ float s_usage[32], s_imp[32];
  if (threadIdx.x < 32) s_hist[threadIdx.x] = 0, s_usage[threadIdx.x] = 0.f, s_imp[threadIdx.x] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int64_t row = blockIdx.x * (int64_t)WPB + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * WPB) {
    Row<NE, VEC> xr;
    xr.load(x + row * D, D, lane);
#pragma unroll
    for (int br = 0; br < 2; ++br) {
      Row<NE, VEC> r = xr;
      r.layernorm(p.ln_w[br], p.ln_b[br], D, lane);
      if constexpr (F8) {  // e4m3 rows and their scales, as the LDS-staged router writes them (csrc/moe_gate_row.h)
        r.store_e4m3((uint8_t*)p.hn + ((int64_t)br * M + row) * D, p.hn_scale + (int64_t)br * M + row, D, lane);
      } else {
        r.store_as(p.hn, (int64_t)br * M + row, D, lane, p.hn_bf16);
      }
      float logit[16];
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        logit[e] = -INFINITY;
        if (e < E) {
          Row<NE, VEC> g;
          g.load(p.gate_w[br] + (int64_t)e * D, D, lane);
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < NE; ++j) s += r.e[j] * g.e[j];
          logit[e] = wave_sum(s) + p.gate_b[br][e];
          mx = fmaxf(mx, logit[e]);
        }
      }
      float den = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        logit[e] = e < E ? expf(logit[e] - mx) : 0.f;
        den += logit[e];
      }
      // top-2 is TOTAL: a row of non-finite logits still yields two distinct in-range experts (its outputs are NaN, which
      // is the wanted signal); every `>` below is false for NaN, so the initial pair survives
      int i1 = 0, i2 = 1;
      float v1 = -1.f, v2 = -1.f;
      if (p.forced_idx) {  // test hook: routing injected, probabilities still computed here
        i1 = min(max(p.forced_idx[((int64_t)br * M + row) * 2 + 0], 0), E - 1);
        i2 = min(max(p.forced_idx[((int64_t)br * M + row) * 2 + 1], 0), E - 1);
        v1 = v2 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pe = logit[e] / den;
          v1 = e == i1 ? pe : v1;
          v2 = e == i2 ? pe : v2;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pe = logit[e] / den;
          if (e < E) {
            if (pe > v1) {
              v2 = v1, i2 = i1;
              v1 = pe, i1 = e;
            } else if (pe > v2) {
              v2 = pe, i2 = e;
            }
          }
        }
        if (!(v2 >= 0.f)) {  // non-finite probabilities: keep the pair distinct and report NaN weights
          i2 = i1 == 0 ? 1 : 0;
          v1 = v2 = __int_as_float(0x7fc00000);
        }
      }
      if (lane == 0) {
        const int64_t o = ((int64_t)br * M + row) * 2;
        p.top_idx[o] = i1, p.top_idx[o + 1] = i2;
        p.top_val[o] = v1, p.top_val[o + 1] = v2;
        atomicAdd(&s_hist[br * E + i1], 1);
        atomicAdd(&s_hist[br * E + i2], 1);
        atomicAdd(&s_usage[br * E + i1], 1.f);  // switch_moe.py:71-92 counters, device side, no host sync
        atomicAdd(&s_imp[br * E + i1], v1);
        atomicAdd(&s_imp[br * E + i2], v2);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * E) {  // per-block partials, summed by moe_offsets_kernel: no global atomics at all
    const int g = threadIdx.x;
    p.hist[blockIdx.x * 32 + g] = s_hist[g];
    p.uimp[blockIdx.x * 64 + g] = s_usage[g];
    p.uimp[blockIdx.x * 64 + 32 + g] = s_imp[g];
  }
}

// Router, 16 lanes per token (4 tokens per wave): one set of LayerNorm statistics serves both branches, the gate
// matrices of both branches sit in LDS, and the 2E logits are reduced with 4-step group shuffles (the one-token-per-
// wave version above spends its time in 2E full-wave reductions).  Requires D % 64 == 0.
// FAST (the 16-bit / fp8 modes, whose routing differences from the fp32-grade mode are budgeted anyway): gate logits as an
// explicit FMA chain; otherwise the sum-of-products form the fp32-grade mode has always used (its near-tie decisions are
// pinned by the parity tests, and a different association resolves some of them differently).
// EX > 0 / HNF >= 0: the expert count and the format of the hn rows as compile-time constants (HNF as p.hn_bf16).  With both, a
// chunk of the logit loop is straight-line code: no `e < E` tests (256 uniform branches per token group) and no branch around the
// hn store (rows past M are clamped to M - 1 and store that row's own values again).  It has to be BOTH: with E constant but a
// branch per chunk left, hipcc sinks all FMAs of a branch below the last chunk and keeps its 80 LDS rows alive (289 - 1358
// spilled registers).  A scheduling fence per chunk keeps the reads next to their FMAs.
template <int NV, bool FAST, int EX = 0, int HNF = -1>  // float4 per lane: D = 64 * NV
__global__ __launch_bounds__(256) void moe_gate16_kernel(const float* __restrict__ x, int64_t M, int D_rt, int E_rt,
                                                         MoeGateParams p) {
  const int E = EX > 0 ? EX : E_rt;
  const int hnf = HNF >= 0 ? HNF : p.hn_bf16;
  constexpr int D = 64 * NV;  // (== D_rt: the host dispatches on D / 64) -- a compile-time row length folds the gate-row and
                              // output addresses into immediates
  extern __shared__ __attribute__((aligned(16))) float gsm[];  // [2][E][D] gate weights, [2][D] LN weights, [2][D] LN biases, counters
  float* gw = gsm;
  float* lnw = gsm + 2 * E * D;  // from LDS, not from global memory: between the hn stores of two chunks a global load
  float* lnb = lnw + 2 * D;      // cannot be moved up (the stores may alias it), so every chunk paid a round trip
  int* s_hist = (int*)(lnb + 2 * D);
  float* s_usage = (float*)(s_hist + 32);
  float* s_imp = s_usage + 32;
  const int l16 = threadIdx.x & 15;
  const int64_t tpb = 16;  // tokens per block iteration
  const int64_t stride = (int64_t)gridDim.x * tpb;
  auto load_x = [&](int64_t base, f32x4(&r)[NV]) {
    const int64_t row = base + (threadIdx.x >> 4);
    const int64_t rc = row < M ? row : M - 1;
#pragma unroll
    for (int c = 0; c < NV; ++c) r[c] = *(const f32x4*)(x + rc * D + 4 * (l16 + 16 * c));
  };
  // the first token rows are requested before the gate matrices are staged, so that their latency runs under the staging
  f32x4 vn[NV];
  if constexpr (NV <= 8)
    if (blockIdx.x * tpb < M) load_x(blockIdx.x * tpb, vn);
  // gate matrices -> LDS, four 16-B loads in flight per lane (written as one loop over both branches the pointer of the
  // branch is itself fetched per iteration and every load waits for the one before: ~11 us of serial round trips per block)
#pragma unroll
  for (int br = 0; br < 2; ++br) {
    const float* src = p.gate_w[br];
    const int n4 = E * D / 4;
    for (int i0 = threadIdx.x; i0 < n4; i0 += 4 * 256) {
      f32x4 t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + 256 * j < n4) t[j] = *(const f32x4*)(src + 4 * (i0 + 256 * j));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + 256 * j < n4) *(f32x4*)(gw + br * E * D + 4 * (i0 + 256 * j)) = t[j];
    }
  }
  for (int i = threadIdx.x; i < D / 4; i += 256) {
    const f32x4 w0 = *(const f32x4*)(p.ln_w[0] + 4 * i), w1 = *(const f32x4*)(p.ln_w[1] + 4 * i);
    const f32x4 b0 = *(const f32x4*)(p.ln_b[0] + 4 * i), b1 = *(const f32x4*)(p.ln_b[1] + 4 * i);
    *(f32x4*)(lnw + 4 * i) = w0, *(f32x4*)(lnw + D + 4 * i) = w1;
    *(f32x4*)(lnb + 4 * i) = b0, *(f32x4*)(lnb + D + 4 * i) = b1;
  }
  if (threadIdx.x < 32) s_hist[threadIdx.x] = 0, s_usage[threadIdx.x] = 0.f, s_imp[threadIdx.x] = 0.f;
  __syncthreads();
  for (int64_t base = blockIdx.x * tpb; base < M; base += stride) {
    const int64_t row = base + (threadIdx.x >> 4);
    const bool ok = row < M;
    const int64_t rc = ok ? row : M - 1;
    if constexpr (NV > 8) load_x(base, vn);  // D = 1024: a second row set in flight costs the second wave per SIMD
    f32x4 v[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = vn[c];
    const float s = gate16_row_sum(v);
    // next iteration's rows, in flight during this one's arithmetic
    if constexpr (NV <= 8)
      if (base + stride < M) load_x(base + stride, vn);
    gate16_row<NV, FAST, EX, HNF>(v, s, row, ok, rc, M, E, hnf, l16, gw, lnw, lnb, s_hist, s_usage, s_imp, p);
  }
  __syncthreads();
  if (threadIdx.x < 2 * E) {  // per-block partials, summed by moe_offsets_kernel: no global atomics at all
    const int g = threadIdx.x;
    p.hist[blockIdx.x * 32 + g] = s_hist[g];
    p.uimp[blockIdx.x * 64 + g] = s_usage[g];
    p.uimp[blockIdx.x * 64 + 32 + g] = s_imp[g];
  }
}

// sums the per-block partial counters, builds the slab offsets, zeroes the cursors and folds the usage / importance
// increments into the module's persistent buffers (single writer, deterministic)
__global__ __launch_bounds__(1024) void moe_offsets_kernel(const int* __restrict__ hist_part,
                                                            const float* __restrict__ uimp_part, int nparts, int E,
                                                            int* __restrict__ goff, int* __restrict__ cursor,
                                                            MoeGateParams p) {
  __shared__ int sh[32][33];
  __shared__ float su[32][33], si[32][33];
  __shared__ int tot[32];
  const int g = threadIdx.x & 31, c = threadIdx.x >> 5, G = 2 * E;  // 32 counters x 32 part-chunks
  int h = 0;
  float u = 0.f, im = 0.f;
  if (g < G) {
#pragma unroll 4
    for (int b = c; b < nparts; b += 32) {  // independent loads: all in flight together
      h += hist_part[b * 32 + g];
      u += uimp_part[b * 64 + g];
      im += uimp_part[b * 64 + 32 + g];
    }
  }
  sh[c][g] = h, su[c][g] = u, si[c][g] = im;
  __syncthreads();
  if (threadIdx.x < G) {
    int ht = 0;
    float ut = 0.f, it = 0.f;
    for (int k = 0; k < 32; ++k) ht += sh[k][g], ut += su[k][g], it += si[k][g];  // fixed order: deterministic
    tot[g] = ht;
    cursor[g] = 0;
    const int br = g / E, e = g - br * E;
    if (p.usage[br]) {  // atomics: forwards of different batch chunks may run concurrently on separate streams
      atomicAdd(&p.usage[br][e], ut);
      atomicAdd(&p.importance[br][e], it);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < G; ++i) {
      goff[i] = s;
      s += tot[i];
    }
    goff[G] = s;
  }
}

// positions inside each expert's contiguous slab: rank within the block from an LDS counter, one global
// atomic per (block, expert) to reserve the block's range.  Order within a slab is irrelevant (rows are independent).
// OFFS (the folded route, moe_route_folded): there is no moe_offsets_kernel in front.  Every workgroup sums the nparts histogram
// partials of the producing launch itself (<= 1024 x 2E ints, L2-resident, independent loads; integer sums, so every workgroup
// gets the same offsets) and scans them in LDS.  The grid has ONE workgroup more than the assignment needs: that last one does the
// bookkeeping and nothing else -- goff for the expert MLP, usage / importance partials folded into the module buffers (single
// writer, fixed order) -- so its two extra passes over the partials run beside the others' assignment instead of in front of it.
// The cursors were zeroed by workgroup 0 of the producing launch.  No workgroup waits for another.
template <bool OFFS>
__global__ __launch_bounds__(256) void moe_assign_kernel(const int* __restrict__ top_idx, const float* __restrict__ top_val,
                                                         int64_t M, int E, int* __restrict__ goff,
                                                         int* __restrict__ cursor, int* __restrict__ perm,
                                                         float* __restrict__ rowscale, int* __restrict__ pos4, int nparts,
                                                         MoeGateParams p) {
  __shared__ int s_cnt[32], s_base[32], s_goff[33];
  if constexpr (OFFS) {
    // column sums of the partials in three steps, every load of a thread requested before the first is used (one memory round
    // trip): thread t sums rows t, t + 256, ... (a row = the 32 counters of one producing workgroup, 128 B), the 256 row sums go
    // through an LDS tile, eight 32-row chunks are summed per counter, then the eight chunk sums.  The order is fixed, so the float
    // sums of the bookkeeping workgroup are deterministic; the integer sums are the same in every workgroup.
    __shared__ int tile[256][33];
    __shared__ int chunk[8][33];
    const int g = threadIdx.x & 31, c = threadIdx.x >> 5, G = 2 * E;
    const bool book = blockIdx.x == gridDim.x - 1;
    auto col_sums = [&](auto zero, const decltype(zero)* __restrict__ part, int ld) {  // -> chunk[0][g], as raw bits
      typedef decltype(zero) T;
      T acc[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) acc[j] = zero;
      for (int b0 = threadIdx.x; b0 < nparts; b0 += 512) {
        const int b1 = b0 + 256;
        uint4 r0[8], r1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r0[j] = 4 * j < G ? *(const uint4*)(part + (int64_t)b0 * ld + 4 * j) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) r1[j] = 4 * j < G && b1 < nparts ? *(const uint4*)(part + (int64_t)b1 * ld + 4 * j) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t w0[4] = {r0[j].x, r0[j].y, r0[j].z, r0[j].w}, w1[4] = {r1[j].x, r1[j].y, r1[j].z, r1[j].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[4 * j + i] += __builtin_bit_cast(T, w0[i]);
            acc[4 * j + i] += __builtin_bit_cast(T, w1[i]);  // (+ 0 past the end: exact for both types)
          }
        }
      }
      __syncthreads();  // (the tile's previous use is over)
#pragma unroll
      for (int j = 0; j < 32; ++j) tile[threadIdx.x][j] = __builtin_bit_cast(int, acc[j]);
      __syncthreads();
      T s = zero;
      for (int i = 0; i < 32; ++i) s += __builtin_bit_cast(T, tile[32 * c + i][g]);
      chunk[c][g] = __builtin_bit_cast(int, s);
      __syncthreads();
      if (threadIdx.x < 32) {
        T t = zero;
        for (int k = 0; k < 8; ++k) t += __builtin_bit_cast(T, chunk[k][g]);
        chunk[0][g] = __builtin_bit_cast(int, t);
      }
      __syncthreads();
    };
    // (counters g >= 2 E of a row are never written by the producer: those in the last 16 bytes read are summed as they are, never used)
    col_sums(0, p.hist, 32);
    if (threadIdx.x < 32) s_cnt[g] = g < G ? chunk[0][g] : 0;  // (reset at the top of the loop below)
    if (book) {  // single writer of the module buffers
      float ut = 0.f, it = 0.f;
      col_sums(0.f, p.uimp, 64);
      if (threadIdx.x < G) ut = __int_as_float(chunk[0][g]);
      col_sums(0.f, p.uimp + 32, 64);
      if (threadIdx.x < G) {
        it = __int_as_float(chunk[0][g]);
        const int br = g / E, e = g - br * E;
        if (p.usage[br]) {  // atomics: forwards of different batch chunks may run concurrently on separate streams
          atomicAdd(&p.usage[br][e], ut);
          atomicAdd(&p.importance[br][e], it);
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
      for (int i = 0; i < G; ++i) {
        s_goff[i] = s;
        s += s_cnt[i];
      }
      s_goff[G] = s;
    }
    __syncthreads();
    if (book) {
      if (threadIdx.x <= G) goff[threadIdx.x] = s_goff[threadIdx.x];
      return;
    }
  } else {
    if (threadIdx.x <= 2 * E) s_goff[threadIdx.x] = goff[threadIdx.x];
    __syncthreads();
  }
  const int64_t total = 2 * M * 2;
  const int64_t nwork = OFFS ? gridDim.x - 1 : gridDim.x;  // workgroups that assign
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < total; base += nwork * blockDim.x) {
    if (threadIdx.x < 32) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = base + threadIdx.x;
    int g = -1, rank = 0;
    int64_t br = 0, tok = 0;
    int k = 0;
    if (i < total) {
      br = i / (2 * M);
      const int64_t rem = i - br * 2 * M;
      tok = rem >> 1, k = (int)(rem & 1);
      g = (int)br * E + min(max(top_idx[i], 0), E - 1);
      rank = atomicAdd(&s_cnt[g], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2 * E && s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
    if (g >= 0) {
      const int pos = s_goff[g] + s_base[g] + rank;
      perm[pos] = (int)(br * M + tok);
      rowscale[pos] = top_val[i];
      pos4[tok * 4 + br * 2 + k] = pos;
    }
    __syncthreads();
  }
}

// ---- per-head (dh) units: G lanes x 4 floats -----------------------------------------------------
template <int G>
__device__ __forceinline__ void head_ln(f32x4& v, const float* w, const float* b, int dh, int gl) {
  const float mean = group_sum<G>(v[0] + v[1] + v[2] + v[3]) / dh;
  const f32x4 d = {v[0] - mean, v[1] - mean, v[2] - mean, v[3] - mean};
  const float rstd = rsqrtf(group_sum<G>(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) / dh + 1e-5f);
  const f32x4 ww = *(const f32x4*)(w + 4 * gl), bb = *(const f32x4*)(b + 4 * gl);
  v = (f32x4){d[0] * rstd * ww[0] + bb[0], d[1] * rstd * ww[1] + bb[1], d[2] * rstd * ww[2] + bb[2],
              d[3] * rstd * ww[3] + bb[3]};
}

// qkv (M,3,H,dh) in place: LN_dh on q,k,v; L2-normalise q,k           (fast_attention.py:44-55)
template <int G>
__global__ __launch_bounds__(256) void head_norm_kernel(float* __restrict__ qkv, int64_t units, int H, int dh,
                                                        const float* w, const float* b) {
  const int gl = threadIdx.x % G;
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G;
  const int64_t ng = (int64_t)gridDim.x * blockDim.x / G;
  for (int64_t u = gid; u < units; u += ng) {
    float* p = qkv + u * dh + 4 * gl;
    f32x4 v = *(const f32x4*)p;
    head_ln<G>(v, w, b, dh, gl);
    const int which = (int)((u / H) % 3);
    if (which < 2) {
      const float n = sqrtf(group_sum<G>(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]));
      const float inv = 1.f / fmaxf(n, 1e-12f);
      v *= inv;
    }
    *(f32x4*)p = v;
  }
}

// out[tok,h,:] = LN_dh( num[tok,h,:] / max(<qphi,kphi>, 1e-6) )       (fast_attention.py:81-90); m == dh
template <int G>
__global__ __launch_bounds__(256) void den_ln_kernel(const float* __restrict__ num, const float* __restrict__ phi,
                                                     int64_t M, int H, int dh, const float* w, const float* b,
                                                     void* __restrict__ out, int out_bf) {
  const int gl = threadIdx.x % G;
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G;
  const int64_t ng = (int64_t)gridDim.x * blockDim.x / G;
  for (int64_t u = gid; u < M * H; u += ng) {
    const int64_t tok = u / H, h = u - tok * H;
    const f32x4 qf = *(const f32x4*)(phi + (tok * 2 * H + h) * dh + 4 * gl);
    const f32x4 kf = *(const f32x4*)(phi + (tok * 2 * H + H + h) * dh + 4 * gl);
    float den = group_sum<G>(qf[0] * kf[0] + qf[1] * kf[1] + qf[2] * kf[2] + qf[3] * kf[3]);
    den = fmaxf(den, 1e-6f);
    f32x4 v = *(const f32x4*)(num + u * dh + 4 * gl);
    v = (f32x4){v[0] / den, v[1] / den, v[2] / den, v[3] / den};
    head_ln<G>(v, w, b, dh, gl);
    if (out_bf) {
      *(uint2*)((uint16_t*)out + u * dh + 4 * gl) = make_uint2(pack_h16(out_bf, v[0], v[1]), pack_h16(out_bf, v[2], v[3]));
    } else {
      *(f32x4*)((float*)out + u * dh + 4 * gl) = v;
    }
  }
}

// softmax over dh per (token, head), in place                           (fast_attention.py:248)
template <int G>
__global__ __launch_bounds__(256) void head_softmax_kernel(float* __restrict__ q, int64_t units, int dh) {
  const int gl = threadIdx.x % G;
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G;
  const int64_t ng = (int64_t)gridDim.x * blockDim.x / G;
  for (int64_t u = gid; u < units; u += ng) {
    float* p = q + u * dh + 4 * gl;
    f32x4 v = *(const f32x4*)p;
    const float mx = group_max<G>(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    v = (f32x4){expf(v[0] - mx), expf(v[1] - mx), expf(v[2] - mx), expf(v[3] - mx)};
    const float s = group_sum<G>(v[0] + v[1] + v[2] + v[3]);
    *(f32x4*)p = (f32x4){v[0] / s, v[1] / s, v[2] / s, v[3] / s};
  }
}

#define MDM_HEAD_DISPATCH(dh, CALL)                 \
  do {                                              \
    switch (dh) {                                   \
      case 16: CALL(4); break;                      \
      case 32: CALL(8); break;                      \
      case 64: CALL(16); break;                     \
      case 128: CALL(32); break;                    \
      case 256: CALL(64); break;                    \
      default: return MDM_ERR_UNSUPPORTED;          \
    }                                               \
  } while (0)

// softmax over the last dim N <= 128 of a (rows, N) matrix, 32 lanes per row, in place (fast_attention.py:320)
__global__ __launch_bounds__(256) void row_softmax_kernel(float* __restrict__ s, int64_t rows, int N, const int32_t* __restrict__ ntok,
                                                          int64_t rows_per_b) {
  const int gl = threadIdx.x & 31;
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 5;
  const int64_t ng = ((int64_t)gridDim.x * blockDim.x) >> 5;
  for (int64_t r = gid; r < rows; r += ng) {
    float* p = s + r * N;
    const int nv = ntok ? min(max(ntok[r / rows_per_b], 1), N) : N;  // this row's sample attends to its first nv text tokens
    float v[4], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = gl + 32 * j;
      v[j] = i < nv ? p[i] : -INFINITY;
      mx = fmaxf(mx, v[j]);
    }
    mx = group_max<32>(mx);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (gl + 32 * j < nv) ? expf(v[j] - mx) : 0.f;
      sum += v[j];
    }
    sum = group_sum<32>(sum);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gl + 32 * j < N) p[gl + 32 * j] = v[j] / sum;
  }
}

// softmax over the token axis n of k (B,N,D), one thread per (b, column), in place (fast_attention.py:249)
__global__ void col_softmax_kernel(float* __restrict__ k, int B, int N, int D, const int32_t* __restrict__ ntok) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * D) return;
  const int64_t b = i / D, c = i - b * D;
  float* p = k + b * N * (int64_t)D + c;
  const int nv = ntok ? min(max(ntok[b], 1), N) : N;  // tokens past the sample's own count are padding: weight 0
  float mx = -INFINITY;
  for (int n = 0; n < nv; ++n) mx = fmaxf(mx, p[(int64_t)n * D]);
  float s = 0.f;
  for (int n = 0; n < nv; ++n) s += expf(p[(int64_t)n * D] - mx);
  for (int n = 0; n < nv; ++n) p[(int64_t)n * D] = expf(p[(int64_t)n * D] - mx) / s;
  for (int n = nv; n < N; ++n) p[(int64_t)n * D] = 0.f;
}

// folded text cross-attention: bias -1e30 on the columns of padded tokens, so that their probability is exactly 0
__global__ void sd_fold_mask_cb_kernel(float* __restrict__ cb, int B, int np, int hpp, int N, const int32_t* __restrict__ ntok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * np * 128) return;
  const int b = i / (np * 128), col = i & 127;
  if (col < hpp * N && col % N >= min(max(ntok[b], 1), N)) cb[i] = -1e30f;
}

// ---- stem pieces ---------------------------------------------------------------------------------
// time.py:15-27: emb[b, i] = cos(t_b * f_i), emb[b, half + i] = sin(t_b * f_i), f_i = exp(-ln(1e4) * i / half)
__global__ void sinusoid_kernel(const int64_t* __restrict__ t, int B, int D, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = D / 2;
  if (i >= B * D) return;
  const int b = i / D, c = i - b * D;
  float v = 0.f;
  if (c < 2 * half) {
    const int f = c < half ? c : c - half;
    const float freq = expf(-9.210340371976184f * (float)f / (float)half);
    const float arg = (float)t[b] * freq;
    v = c < half ? cosf(arg) : sinf(arg);
  }
  out[i] = v;
}

// gate.py:18-20: g = sigmoid(t + x); out = g * t + (1 - g) * x
__global__ void gated_mix_kernel(const float* __restrict__ t, const float* __restrict__ x, int64_t n,
                                 float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float tv = t[i], xv = x[i];
  const float g = 1.f / (1.f + expf(-(tv + xv)));
  out[i] = g * tv + (1.f - g) * xv;
}

// text_encoder.py:40-43: xf_out[b] = cat(proj(prompts), proj(hidden[b])) ; xf_proj[b] = mean over the P + N0 tokens
__global__ void text_assemble_kernel(const float* __restrict__ pp, const float* __restrict__ ph, int B, int N0, int P, int Dt,
                                     float* __restrict__ xf_out, float* __restrict__ xf_proj) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * Dt) return;
  const int b = i / Dt, d = i - b * Dt, N = P + N0;
  float* o = xf_out + (int64_t)b * N * Dt + d;
  float s = 0.f;
  for (int n = 0; n < P; ++n) {
    const float v = pp[n * Dt + d];
    o[(int64_t)n * Dt] = v;
    s += v;
  }
  for (int n = 0; n < N0; ++n) {
    const float v = ph[((int64_t)b * N0 + n) * Dt + d];
    o[(int64_t)(P + n) * Dt] = v;
    s += v;
  }
  xf_proj[i] = s / (float)N;
}

// same with t looked up in a per-timestep table (stem cache) and an optional bf16 copy of the result
__global__ void gated_mix_gather_kernel(const float* __restrict__ table, const int64_t* __restrict__ ts, int steps,
                                        const float* __restrict__ x, int B, int D, float* __restrict__ out,
                                        uint16_t* __restrict__ out16, int fmt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D) return;
  const int b = i / D, c = i - b * D;
  int64_t t = ts[b];
  t = t < 0 ? 0 : (t >= steps ? steps - 1 : t);
  const float tv = table[t * D + c], xv = x[i];
  const float g = 1.f / (1.f + expf(-(tv + xv)));
  const float v = g * tv + (1.f - g) * xv;
  if (out) out[i] = v;
  if (out16) out16[i] = (uint16_t)(pack_h16(fmt, v, 0.f) & 0xffff);
}

__global__ void iota_i64_kernel(int64_t* dst, int64_t n, int64_t start) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) dst[i] = start + i;
}

// gate vector of the gated cross attention: gvec[c] = sigmoid(gate[c]) * sigmoid(adaptive_gate)
// (fast_attention.py:256-257,271-272 folded: x + sg*(x + sa*style - x) = x + sg*sa*style)
__global__ void xattn_gate_kernel(const float* __restrict__ gate, const float* __restrict__ ag, int D,
                                  float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D) out[i] = (1.f / (1.f + expf(-gate[i]))) * (1.f / (1.f + expf(-ag[0])));
}

__global__ void halve_lengths_kernel(const int* __restrict__ len, int B, int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) out[i] = (int)(((float)len[i]) / 2.f);  // (length / 2).long(), transformer.py:341
}

// ---- sampler updates (gaussian_diffusion.py:554-558, 462-475, 1075-1096, 725-742) ---------------
__global__ void cfg_step_kernel(const float* __restrict__ x, const float* __restrict__ eps_c,
                                const float* __restrict__ eps_u, const float* __restrict__ noise, int64_t n,
                                const float* __restrict__ tab, int ts, const int* __restrict__ t_ptr, int t_imm, float cfg_scale, int clip,
                                float* __restrict__ x_out, float* __restrict__ x0_out) {
  int t = t_ptr ? *t_ptr : t_imm;
  t = min(max(t, 0), ts - 1);  // a stale device counter must not index outside the table
  const float a = tab[TAB_SQRT_RECIP * ts + t], b = tab[TAB_SQRT_RECIPM1 * ts + t];
  const float c1 = tab[TAB_COEF1 * ts + t], c2 = tab[TAB_COEF2 * ts + t];
  const float sd = t == 0 ? 0.f : expf(0.5f * tab[TAB_LOGVAR * ts + t]);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float xv = x[i];
    float x0c = a * xv - b * eps_c[i];
    if (clip) x0c = fminf(fmaxf(x0c, -1.f), 1.f);
    float x0 = x0c;
    if (eps_u) {
      float x0u = a * xv - b * eps_u[i];
      if (clip) x0u = fminf(fmaxf(x0u, -1.f), 1.f);
      x0 = x0u + cfg_scale * (x0c - x0u);
    }
    const float mean = c1 * x0 + c2 * xv;
    x_out[i] = mean + (noise ? sd * noise[i] : 0.f);
    if (x0_out) x0_out[i] = x0;
  }
}

__global__ void ddim_step_kernel(const float* __restrict__ x, const float* __restrict__ eps_in,
                                 const float* __restrict__ noise, int64_t n, const float* __restrict__ tab, int ts,
                                 const int* __restrict__ t_ptr, int t_imm, float eta, int clip,
                                 float* __restrict__ x_out, float* __restrict__ x0_out) {
  int t = t_ptr ? *t_ptr : t_imm;
  t = min(max(t, 0), ts - 1);
  const float a = tab[TAB_SQRT_RECIP * ts + t], b = tab[TAB_SQRT_RECIPM1 * ts + t];
  const float ab = tab[TAB_ACP * ts + t], abp = tab[TAB_ACP_PREV * ts + t];
  const float sigma = eta * sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
  const float sq_abp = sqrtf(abp), dir = sqrtf(1.f - abp - sigma * sigma);
  const float nz = t == 0 ? 0.f : 1.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float xv = x[i];
    float x0 = a * xv - b * eps_in[i];
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const float eps = (a * xv - x0) / b;
    const float mean = x0 * sq_abp + dir * eps;
    x_out[i] = mean + (noise ? nz * sigma * noise[i] : 0.f);
    if (x0_out) x0_out[i] = x0;
  }
}

__global__ void to_bf16_kernel(const float* __restrict__ src, int64_t n4, uint16_t* __restrict__ dst, int fmt) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 v = *(const f32x4*)(src + 4 * i);
    *(uint2*)(dst + 4 * i) = make_uint2(pack_h16(fmt, v[0], v[1]), pack_h16(fmt, v[2], v[3]));
  }
}

// exact: the 11 significand bits of an fp16 value fit bf16 hi (8) + lo = rn(x - hi)
__global__ void f16_to_bf16x2_kernel(const uint32_t* __restrict__ src, int64_t n2, uint32_t* __restrict__ hi, uint32_t* __restrict__ lo) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t u = src[i];
    uint32_t h, l;
    split_bf16(f16_lo_f32(u), f16_hi_f32(u), h, l);
    hi[i] = h, lo[i] = l;
  }
}

__global__ void fill_i64_kernel(int64_t* dst, int64_t n, const int* src) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (int64_t)*src;
}
__global__ void add_i32_kernel(int* dst, int delta) { *dst += delta; }

inline int unit_grid(int64_t units, int G) {
  int64_t per_block = 256 / G;
  int64_t g = (units + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

int ln_chain(const float* x, int64_t M, int D, const float* w1, const float* b1, void* y1, int y1_bf, const float* w2,
             const float* b2, void* y2, int y2_bf, hipStream_t s, int x_bf) {
  if (M <= 0) return MDM_OK;
  if (!x || !w1 || !b1 || (w2 && (!b2 || !y2)) || (!w2 && !y1)) return MDM_ERR_ARG;
  // formats: 0 fp32, 1 / 2 the launch's ONE 16-bit format, 4 (outputs only) x2 rows: D a multiple of 256 (the vector row widths)
  if ((unsigned)x_bf > 2 || (y1_bf != 4 && (unsigned)y1_bf > 2) || (y2_bf != 4 && (unsigned)y2_bf > 2) || ((x_bf | y1_bf | y2_bf) & 3) == 3)
    return MDM_ERR_ARG;
  if ((y1_bf == 4 || y2_bf == 4) && D != 256 && D != 512 && D != 1024) return MDM_ERR_UNSUPPORTED;
#define CALL(NE, VEC) \
  hipLaunchKernelGGL((ln_chain_kernel<NE, VEC>), dim3(row_grid((M + 1) / 2)), dim3(256), 0, s, x, x_bf, M, D, w1, b1, y1, y1_bf, w2, b2, y2, y2_bf)
  MDM_ROW_DISPATCH(D, CALL);
#undef CALL
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int style_in(const float* x, int64_t M, int D, int S, const float* pw, const float* pb, const float* sw,
             const float* sb, const float* sc, const int* pos4, int x_bf, void* out, int out_bf, hipStream_t s) {
  if (M <= 0) return MDM_OK;
  if (!x || !sw || !sb || !sc || !out || S <= 0) return MDM_ERR_ARG;
  if ((unsigned)x_bf > 2 || (unsigned)out_bf > 2 || (x_bf | out_bf) == 3 || (pw && !pb)) return MDM_ERR_ARG;  // one 16-bit format per launch
#define CALL(NE, VEC)                                                                                              \
  hipLaunchKernelGGL((style_in_kernel<NE, VEC>), dim3(row_grid(M)), dim3(256), 0, s, x, M, D, S, pw, pb, sw, sb, sc, \
                     pos4, x_bf, out, out_bf)
  MDM_ROW_DISPATCH(D, CALL);
#undef CALL
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

// The router with compile-time expert count and hn format (D = 512 / 1024, E = 8 / 16, 16-bit hn rows): bit-identical to the
// run-time version (tests/test_blocks_gpu.py) and 2 % of a step faster at both model sizes (5.85 -> 5.74 and 15.59 -> 15.27 ms,
// alternating runs on one box).  Default for E = 8 at D = 512 and D = 1024 (the combinations the bit-equality tests cover:
// tests/test_blocks_gpu.py, tests/test_bigsize_gpu.py); MDM_VAR_ROUTER_CONST_E takes it wherever it exists, MDM_VAR_ROUTER_RUNTIME_E
// never.
bool gate16_const_wanted(int nv, int E) {
  if (g_variant == MDM_VAR_ROUTER_RUNTIME_E) return false;
  // E = 16 (BASELINE configs[4]) as well: 6.65 -> 6.50 ms per step at its per-GPU shape (big, B = 8), same-box A/B of knobs 0 / 26
  return g_variant == MDM_VAR_ROUTER_CONST_E || ((nv == 8 || nv == 16) && (E == 8 || E == 16));
}
template <int NV, int EX, int HNF, bool FAST = true>
bool launch_gate16_const(int grid, int smem, hipStream_t s, const float* x, int64_t M, int D, int E, const MoeGateParams& p) {
  static DevInt attr_done;
  if (smem > 65536 && smem > attr_done) {
    if (hipFuncSetAttribute((const void*)moe_gate16_kernel<NV, FAST, EX, HNF>, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
      return false;
    attr_done = smem;
  }
  hipLaunchKernelGGL((moe_gate16_kernel<NV, FAST, EX, HNF>), dim3(grid), dim3(256), smem, s, x, M, D, E, p);
  return true;
}
template <int NV, int EX>
bool gate16_const_fmt(int grid, int smem, hipStream_t s, const float* x, int64_t M, int D, int E, const MoeGateParams& p) {
  switch (p.hn_bf16) {
    case 1: return launch_gate16_const<NV, EX, 1>(grid, smem, s, x, M, D, E, p);
    case 2: return launch_gate16_const<NV, EX, 2>(grid, smem, s, x, M, D, E, p);
    // fp32 rows (the fp32-grade modes): straight-line code as well, with the sum-of-products association of the logits that
    // those modes' routing is pinned to (FAST = false): bit-identical to the run-time-E kernel
    case 0:
      if constexpr (NV == 8 && EX == 8) return launch_gate16_const<NV, EX, 0, false>(grid, smem, s, x, M, D, E, p);
      return false;
    case 4:  // the same rows pre-split (x2): same logits, same routing
      if constexpr (NV == 8 && EX == 8) return launch_gate16_const<NV, EX, 4, false>(grid, smem, s, x, M, D, E, p);
      return false;
    default: return false;  // fp8 rows are written after the logit loop: nothing per chunk pins the FMAs, and they sink again
  }
}
bool gate16_const(int nv, int grid, int smem, hipStream_t s, const float* x, int64_t M, int D, int E, const MoeGateParams& p) {
  if (nv == 8 && E == 8) return gate16_const_fmt<8, 8>(grid, smem, s, x, M, D, E, p);
  if (nv == 8 && E == 16) return gate16_const_fmt<8, 16>(grid, smem, s, x, M, D, E, p);
  if (nv == 16 && E == 8) return gate16_const_fmt<16, 8>(grid, smem, s, x, M, D, E, p);
  if (nv == 16 && E == 16) return gate16_const_fmt<16, 16>(grid, smem, s, x, M, D, E, p);
  return false;
}

int moe_route(const float* x, int64_t M, int D, int E, const MoeGateParams& p, int* goff, int* cursor, int* perm,
              float* rowscale, int* pos4, hipStream_t s) {
  if (M <= 0) return MDM_OK;
  if (E < 2 || E > 16 || !x || !p.hn || !p.hist || !p.uimp || !p.top_idx || !p.top_val) return MDM_ERR_ARG;
  if (p.hn_bf16 == 3 && !p.hn_scale) return MDM_ERR_ARG;  // e4m3 rows go with their per-row scales
  int nparts = 0;
  // the LDS-staged router exists for D / 64 in {1, 2, 4, 8, 16}; every other width (768, 320, 1000, ...) takes the row kernel
  const int nv = D % 64 == 0 ? D / 64 : 0;
  if (nv == 1 || nv == 2 || nv == 4 || nv == 8 || nv == 16) {
    const int smem = 2 * E * D * 4 + 4 * D * 4 + 3 * 32 * 4;  // gate matrices, LayerNorm vectors, counters
    int64_t nb = (M + 15) / 16;
    const int grid = (int)(nb > 512 ? 512 : nb);  // measured end to end: 256 blocks -2 %, 1024 blocks -0.5 %
    nparts = grid;
    static DevInt attr_done;
    if (smem > 65536 && smem > attr_done) {
      const void* fns[4] = {(const void*)moe_gate16_kernel<16, true>, (const void*)moe_gate16_kernel<16, false>,
                            (const void*)moe_gate16_kernel<8, true>, (const void*)moe_gate16_kernel<8, false>};
      for (const void* fn : fns)
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) return MDM_ERR_LAUNCH;
      attr_done = smem;
    }
#define GATE16(NV)                                                                                            \
  do {                                                                                                        \
    if (gate16_const_wanted(NV, E) && gate16_const(NV, grid, smem, s, x, M, D, E, p)) {                      \
    } else if (p.hn_bf16 && p.hn_bf16 != 4) {                                                                 \
      hipLaunchKernelGGL((moe_gate16_kernel<NV, true>), dim3(grid), dim3(256), smem, s, x, M, D, E, p);       \
    } else {                                                                                                  \
      hipLaunchKernelGGL((moe_gate16_kernel<NV, false>), dim3(grid), dim3(256), smem, s, x, M, D, E, p);      \
    }                                                                                                         \
  } while (0)
    switch (D / 64) {
      case 1: GATE16(1); break;
      case 2: GATE16(2); break;
      case 4: GATE16(4); break;
      case 8: GATE16(8); break;
      case 16: GATE16(16); break;
      default: return MDM_ERR_UNSUPPORTED;
    }
#undef GATE16
  } else {
  const int gate_grid = row_grid(M) > 512 ? 512 : row_grid(M);
  nparts = gate_grid;
#define CALL(NE, VEC)                                                                                         \
  do {                                                                                                        \
    if (p.hn_bf16 == 3) {                                                                                     \
      hipLaunchKernelGGL((moe_gate_kernel<NE, VEC, true>), dim3(gate_grid), dim3(256), 0, s, x, M, D, E, p);  \
    } else {                                                                                                  \
      hipLaunchKernelGGL((moe_gate_kernel<NE, VEC, false>), dim3(gate_grid), dim3(256), 0, s, x, M, D, E, p); \
    }                                                                                                         \
  } while (0)
  MDM_ROW_DISPATCH(D, CALL);
#undef CALL
  }
  hipLaunchKernelGGL(moe_offsets_kernel, dim3(1), dim3(1024), 0, s, p.hist, p.uimp, nparts, E, goff, cursor, p);
  const int64_t total = 4 * M;
  int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(moe_assign_kernel<false>, dim3(blocks > 1024 ? 1024 : blocks), dim3(256), 0, s, p.top_idx, p.top_val, M, E,
                     goff, cursor, perm, rowscale, pos4, nparts, p);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

// The rest of the route behind a stylization launch that ran the gate in its epilogue (style_gemm with a StyleRoute): that launch
// left top_idx / top_val / hn, nparts per-workgroup partials in p.hist / p.uimp and zeroed cursors; ONE launch makes the offsets
// and assigns the slab positions.
int moe_route_folded(int64_t M, int E, const MoeGateParams& p, int nparts, int* goff, int* cursor, int* perm, float* rowscale,
                     int* pos4, hipStream_t s) {
  if (M <= 0) return MDM_OK;
  if (E < 2 || E > 16 || nparts < 1 || nparts > 1024 || !p.hist || !p.uimp || !p.top_idx || !p.top_val) return MDM_ERR_ARG;
  const int64_t total = 4 * M;
  int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(moe_assign_kernel<true>, dim3((blocks > 1024 ? 1024 : blocks) + 1), dim3(256), 0, s, p.top_idx, p.top_val, M, E,
                     goff, cursor, perm, rowscale, pos4, nparts, p);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int head_norm(float* qkv, int64_t M, int H, int dh, const float* w, const float* b, hipStream_t s) {
  if (M <= 0) return MDM_OK;
  const int64_t units = M * 3 * H;
#define CALL(G) hipLaunchKernelGGL((head_norm_kernel<G>), dim3(unit_grid(units, G)), dim3(256), 0, s, qkv, units, H, dh, w, b)
  MDM_HEAD_DISPATCH(dh, CALL);
#undef CALL
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int den_ln(const float* num, const float* phi, int64_t M, int H, int dh, const float* w, const float* b, void* out,
           int out_bf, hipStream_t s) {
  if (M <= 0) return MDM_OK;
#define CALL(G) \
  hipLaunchKernelGGL((den_ln_kernel<G>), dim3(unit_grid(M * H, G)), dim3(256), 0, s, num, phi, M, H, dh, w, b, out, out_bf)
  MDM_HEAD_DISPATCH(dh, CALL);
#undef CALL
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int head_softmax(float* q, int64_t units, int dh, hipStream_t s) {
  if (units <= 0) return MDM_OK;
#define CALL(G) hipLaunchKernelGGL((head_softmax_kernel<G>), dim3(unit_grid(units, G)), dim3(256), 0, s, q, units, dh)
  MDM_HEAD_DISPATCH(dh, CALL);
#undef CALL
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int row_softmax(float* sc, int64_t rows, int N, hipStream_t s, const int32_t* ntok, int64_t rows_per_b) {
  if (rows <= 0) return MDM_OK;
  if (N < 1 || N > 128 || rows_per_b < 1) return MDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(row_softmax_kernel, dim3(unit_grid(rows, 32)), dim3(256), 0, s, sc, rows, N, ntok, rows_per_b);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int col_softmax(float* k, int B, int N, int D, hipStream_t s, const int32_t* ntok) {
  const int64_t n = (int64_t)B * D;
  if (n <= 0) return MDM_OK;
  hipLaunchKernelGGL(col_softmax_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, k, B, N, D, ntok);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int sd_fold_mask_cb(float* cb, int B, int np, int hpp, int N, const int32_t* ntok, hipStream_t s) {
  const int n = B * np * 128;
  if (n <= 0 || !ntok) return MDM_OK;
  if (!cb || N < 1) return MDM_ERR_ARG;
  hipLaunchKernelGGL(sd_fold_mask_cb_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cb, B, np, hpp, N, ntok);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int sinusoid(const int64_t* t, int B, int D, float* out, hipStream_t s) {
  hipLaunchKernelGGL(sinusoid_kernel, dim3((B * D + 255) / 256), dim3(256), 0, s, t, B, D, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int gated_mix(const float* t, const float* x, int64_t n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(gated_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, x, n, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int text_assemble(const float* pp, const float* ph, int B, int N0, int P, int Dt, float* xf_out, float* xf_proj,
                  hipStream_t s) {
  hipLaunchKernelGGL(text_assemble_kernel, dim3((B * Dt + 255) / 256), dim3(256), 0, s, pp, ph, B, N0, P, Dt, xf_out, xf_proj);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int gated_mix_gather(const float* table, const int64_t* ts, int steps, const float* x, int B, int D, float* out,
                     uint16_t* out16, int h16, hipStream_t s) {
  hipLaunchKernelGGL(gated_mix_gather_kernel, dim3((B * D + 255) / 256), dim3(256), 0, s, table, ts, steps, x, B, D, out, out16, h16);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int iota_i64(int64_t* dst, int64_t n, int64_t start, hipStream_t s) {
  hipLaunchKernelGGL(iota_i64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, n, start);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int xattn_gate(const float* gate, const float* ag, int D, float* out, hipStream_t s) {
  hipLaunchKernelGGL(xattn_gate_kernel, dim3((D + 255) / 256), dim3(256), 0, s, gate, ag, D, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int halve_lengths(const int* len, int B, int* out, hipStream_t s) {
  hipLaunchKernelGGL(halve_lengths_kernel, dim3((B + 255) / 256), dim3(256), 0, s, len, B, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int to_bf16(const float* src, int64_t n, uint16_t* dst, int h16, hipStream_t s) {
  if (n <= 0) return MDM_OK;
  if (n & 3) return MDM_ERR_ARG;
  int64_t blocks = (n / 4 + 255) / 256;
  hipLaunchKernelGGL(to_bf16_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, src, n / 4, dst, h16);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int f16_to_bf16x2(const uint16_t* src, int64_t n, uint16_t* hi, uint16_t* lo, hipStream_t s) {
  if (n <= 0) return MDM_OK;
  if ((n & 1) || ((((uintptr_t)src) | ((uintptr_t)hi) | ((uintptr_t)lo)) & 3)) return MDM_ERR_ARG;
  int64_t blocks = (n / 2 + 255) / 256;
  hipLaunchKernelGGL(f16_to_bf16x2_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, (const uint32_t*)src, n / 2,
                     (uint32_t*)hi, (uint32_t*)lo);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int fill_i64(int64_t* dst, int64_t n, const int* src, hipStream_t s) {
  if (n <= 0) return MDM_OK;
  hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, n, src);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int add_i32(int* dst, int delta, hipStream_t s) {
  hipLaunchKernelGGL(add_i32_kernel, dim3(1), dim3(1), 0, s, dst, delta);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int cfg_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, int64_t n, const float* tab,
             int ts, const int* t_ptr, int t_imm, float cfg_scale, int clip, float* x_out, float* x0_out, hipStream_t s) {
  if (n <= 0) return MDM_OK;
  if (!x || !eps_c || !tab || !x_out) return MDM_ERR_ARG;
  int blocks = (int)((n + 255) / 256);
  hipLaunchKernelGGL(cfg_step_kernel, dim3(blocks > 2048 ? 2048 : blocks), dim3(256), 0, s, x, eps_c, eps_u, noise, n,
                     tab, ts, t_ptr, t_imm, cfg_scale, clip, x_out, x0_out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int ddim_step(const float* x, const float* eps, const float* noise, int64_t n, const float* tab, int ts, const int* t_ptr,
              int t_imm, float eta, int clip, float* x_out, float* x0_out, hipStream_t s) {
  if (n <= 0) return MDM_OK;
  if (!x || !eps || !tab || !x_out) return MDM_ERR_ARG;
  int blocks = (int)((n + 255) / 256);
  hipLaunchKernelGGL(ddim_step_kernel, dim3(blocks > 2048 ? 2048 : blocks), dim3(256), 0, s, x, eps, noise, n, tab, ts,
                     t_ptr, t_imm, eta, clip, x_out, x0_out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // namespace mdm
