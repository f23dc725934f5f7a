// The MoE router's work on ONE token row held by a 16-lane group (lane l16 holds columns k = 4 (l16 + 16 c), c < NV): one set of
// LayerNorm statistics, both branches' affine forms (the hn rows), 2 E gate logits, softmax denominator, top-2 and the workgroup's
// LDS counters.  Instantiated by moe_gate16_kernel (csrc/rowwise.hip: the row comes from global memory) and by the routing
// epilogue of the cross-attention stylization launch (csrc/style_gemm.hip: the row comes from the epilogue's LDS staging) -- one
// body, so the two route bit for bit alike.  The template arguments are those of moe_gate16_kernel (see the comment there).
#pragma once
#include "kernels.h"
#include "mdm_common.h"

namespace mdm {
namespace {

// LDS image the row body reads: [2][E][D] gate weights, [2][D] LayerNorm weights, [2][D] LayerNorm biases, then the counters
// (32 histogram ints, 32 usage floats, 32 importance floats)
__host__ __device__ constexpr int gate16_lds_bytes(int E, int D) { return 2 * E * D * 4 + 4 * D * 4 + 3 * 32 * 4; }

// v: the row (consumed), s = gate16_row_sum(v).  row / ok / rc: its index, whether it exists (row < M) and the index its stores go to (ok ? row : M - 1:
// with HNF >= 0 a past-the-end group holds row M - 1 and stores that row's own hn values again).
// EB: a scheduling fence after every EB experts of a chunk (only instruction order: each logit's FMA chain is its own), for a
// caller with fewer registers than moe_gate16_kernel.
// the lane's part of the row sum (the first LayerNorm statistic): the caller computes it as the row arrives and hands it to gate16_row
template <int NV>
__device__ __forceinline__ float gate16_row_sum(const f32x4 (&v)[NV]) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NV; ++c) s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
  return s;
}

template <int NV, bool FAST, int EX, int HNF, int EB = 16>
__device__ __forceinline__ void gate16_row(f32x4 (&v)[NV], float s, int64_t row, bool ok, int64_t rc, int64_t M, int E, int hnf, int l16,
                                           const float* gw, const float* lnw, const float* lnb, int* s_hist, float* s_usage,
                                           float* s_imp, const MoeGateParams& p) {
  constexpr int D = 64 * NV;
  const float mean = group_sum<16>(s) / D;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    v[c] = (f32x4){v[c][0] - mean, v[c][1] - mean, v[c][2] - mean, v[c][3] - mean};
    q += v[c][0] * v[c][0] + v[c][1] * v[c][1] + v[c][2] * v[c][2] + v[c][3] * v[c][3];
  }
  const float rstd = rsqrtf(group_sum<16>(q) / D + 1e-5f);
#pragma unroll
  for (int br = 0; br < 2; ++br) {
    float logit[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) logit[e] = 0.f;
    float amax = 0.f;  // fp8 rows: per-row scale from the largest |LN output|
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int k = 4 * (l16 + 16 * c);
      const f32x4 w = *(const f32x4*)(lnw + br * D + k), b = *(const f32x4*)(lnb + br * D + k);
      const f32x4 h = {v[c][0] * rstd * w[0] + b[0], v[c][1] * rstd * w[1] + b[1], v[c][2] * rstd * w[2] + b[2],
                       v[c][3] * rstd * w[3] + b[3]};
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(h[0]), fabsf(h[1])), fmaxf(fabsf(h[2]), fabsf(h[3]))));
      if constexpr (HNF >= 0) {
        if constexpr (HNF == 1 || HNF == 2) {
          *(uint2*)((uint16_t*)p.hn + ((int64_t)br * M + rc) * D + k) = make_uint2(pack_h16(HNF, h[0], h[1]), pack_h16(HNF, h[2], h[3]));
        } else if constexpr (HNF == 0) {
          *(f32x4*)((float*)p.hn + ((int64_t)br * M + rc) * D + k) = h;
        } else if constexpr (HNF == 4) {  // x2 rows (MDM_OP_X2_ROW): what the fp32-grade expert GEMM reads without re-splitting
          // (p.hn is a workspace buffer the library carves itself; all 16 lanes of a row store, past-the-end rows repeat row M - 1)
          static_assert(D % 32 == 0, "lane pairs of store_x2_4p hold k and k ^ 4 of one 32-column block");
          store_x2_4p((uint16_t*)p.hn + ((int64_t)br * M + rc) * 2 * D, k, h[0], h[1], h[2], h[3]);
        }
      } else if (ok && p.hn_bf16 != 3) {
        if (p.hn_bf16 == 4) {
          store_x2_4((uint16_t*)p.hn + ((int64_t)br * M + row) * 2 * D, k, h[0], h[1], h[2], h[3]);
        } else if (p.hn_bf16 == 2) {  // (one uniform branch per chunk, not one per converted pair)
          *(uint2*)((uint16_t*)p.hn + ((int64_t)br * M + row) * D + k) = make_uint2(pack_h16(2, h[0], h[1]), pack_h16(2, h[2], h[3]));
        } else if (p.hn_bf16) {
          *(uint2*)((uint16_t*)p.hn + ((int64_t)br * M + row) * D + k) = make_uint2(pack_h16(1, h[0], h[1]), pack_h16(1, h[2], h[3]));
        } else {
          *(f32x4*)((float*)p.hn + ((int64_t)br * M + row) * D + k) = h;
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < E) {
          const f32x4 g = *(const f32x4*)(gw + (br * E + e) * D + k);
          if constexpr (FAST) {
            // explicit FMA chain: written as a sum of products hipcc SLP-packs the four multiplies (v_pk_mul_f32) and adds
            // the results one by one -- 1626 VALU instructions per token group where 1024 FMAs do
            logit[e] = __builtin_fmaf(h[3], g[3], __builtin_fmaf(h[2], g[2], __builtin_fmaf(h[1], g[1], __builtin_fmaf(h[0], g[0], logit[e]))));
          } else {
            logit[e] += h[0] * g[0] + h[1] * g[1] + h[2] * g[2] + h[3] * g[3];
          }
          if constexpr (EX > 0 && HNF >= 0 && EB < 16)
            if ((e + 1) % EB == 0 && e + 1 < EX) __builtin_amdgcn_sched_barrier(0);
        }
      if constexpr (EX > 0 && HNF >= 0) __builtin_amdgcn_sched_barrier(0);
    }
    if (hnf == 3) {  // e4m3 rows, scale = amax / 448 (the LayerNorm output is recomputed: cheaper than keeping it)
      amax = group_max<16>(amax);
      const float scale = amax > 0.f ? amax * (1.f / 448.f) : 1.f, inv = 1.f / scale;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const int k = 4 * (l16 + 16 * c);
        const f32x4 w = *(const f32x4*)(lnw + br * D + k), b = *(const f32x4*)(lnb + br * D + k);
        uint32_t q8 = 0;
        q8 = __builtin_amdgcn_cvt_pk_fp8_f32((v[c][0] * rstd * w[0] + b[0]) * inv, (v[c][1] * rstd * w[1] + b[1]) * inv, q8, false);
        q8 = __builtin_amdgcn_cvt_pk_fp8_f32((v[c][2] * rstd * w[2] + b[2]) * inv, (v[c][3] * rstd * w[3] + b[3]) * inv, q8, true);
        if (HNF >= 0 || ok) *(uint32_t*)((uint8_t*)p.hn + ((int64_t)br * M + (HNF >= 0 ? rc : row)) * D + k) = q8;
      }
      if (ok && l16 == 0) p.hn_scale[(int64_t)br * M + row] = scale;
    }
    // top-2 is decided on the LOGITS (softmax is monotone; ties -> lowest index), the softmax denominator is built
    // with one exp per lane (lane e owns expert e) instead of E exps in every lane
    float mx = -INFINITY, mine = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (e < E) {
        logit[e] = group_sum<16>(logit[e]) + p.gate_b[br][e];
        mx = fmaxf(mx, logit[e]);
        mine = (l16 == e) ? logit[e] : mine;
      }
    }
    const float den = group_sum<16>(l16 < E ? expf(mine - mx) : 0.f);
    // top-2 is TOTAL (see moe_gate_kernel): NaN logits fail every `>`, the distinct in-range initial pair survives and the
    // probabilities (hence the token's outputs) come out NaN instead of an out-of-range index
    int i1 = 0, i2 = 1;
    float l1 = -INFINITY, l2 = -INFINITY;
    if (p.forced_idx) {
      i1 = min(max(p.forced_idx[((int64_t)br * M + rc) * 2 + 0], 0), E - 1);
      i2 = min(max(p.forced_idx[((int64_t)br * M + rc) * 2 + 1], 0), E - 1);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        l1 = e == i1 ? logit[e] : l1;
        l2 = e == i2 ? logit[e] : l2;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (e < E) {
          if (logit[e] > l1) {
            l2 = l1, i2 = i1;
            l1 = logit[e], i1 = e;
          } else if (logit[e] > l2) {
            l2 = logit[e], i2 = e;
          }
        }
      }
      if (i2 == i1) i2 = i1 == 0 ? 1 : 0;  // only reachable with non-finite logits
    }
    const float v1 = expf(l1 - mx) / den, v2 = expf(l2 - mx) / den;
    if (ok && l16 == 0) {
      const int64_t o = ((int64_t)br * M + row) * 2;
      p.top_idx[o] = i1, p.top_idx[o + 1] = i2;
      p.top_val[o] = v1, p.top_val[o + 1] = v2;
      atomicAdd(&s_hist[br * E + i1], 1);
      atomicAdd(&s_hist[br * E + i2], 1);
      atomicAdd(&s_usage[br * E + i1], 1.f);
      atomicAdd(&s_imp[br * E + i1], v1);
      atomicAdd(&s_imp[br * E + i2], v2);
    }
  }
}

}  // namespace
}  // namespace mdm
