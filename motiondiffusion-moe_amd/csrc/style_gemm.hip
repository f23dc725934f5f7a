// StylizationBlock in ONE launch (stylization.py:20-31 behind its callers' row-wise heads):
//     s   = SiLU( LN_style(a) * (1 + scale[b]) + shift[b] )                       a per row, as csrc/rowwise.hip style_in:
//           a = x | normalize(LN_post(x)) * sqrt(D) (Performer tail, fast_attention.py:169-172) | 0.5 * sum of the token's four
//           routed expert rows (MoE combine, switch_moe.py:109 + multi_branch.py:58-59)
//     out = resid + out_scale * colscale * ( s Wout^T + b )                        (out_layers.2 and the caller's residual)
// replaces the style_in launch + the D x D GEMM launch behind it (4 pairs per decoder layer, 32 per forward) and the 16-bit
// [M, D] tensor between them.  D = 512, 16-bit modes.
//
// One workgroup (8 waves, <= 128 registers: two resident per CU) owns 32 whole rows:
//   * row phase: wave w brings rows 4 w .. 4 w + 3 exactly as the row-wise kernel does (one wave per row, DPP reductions) and
//     leaves them as 16-bit MFMA rows in a 32-KiB LDS image (16-B chunk c of row r at slot c ^ (r & 15));
//   * GEMM phase: wave w owns output columns [64 w, 64 w + 64): the image is the shared operand, Wout is streamed global ->
//     registers from a packed fragment stream (mdm_gemm_stream_pack: per wave the 64 fragments of its columns in K order) through
//     an 8-fragment ring, as in csrc/mlp_stream.hip.  With 32 rows a weight fragment feeds only two MFMAs, so the launch is bound
//     by the 512 KiB of Wout every workgroup streams (98 / 196 MB per launch, L2-resident), not by the matrix pipe;
//   * epilogue: staged as fp32 rows through LDS, full-row stores, residual read coalesced;
//   * routing epilogue (RE > 0: the cross-attention position in front of the MoE block, when the caller passes a StyleRoute): the
//     finished rows go back into the staging, every 16-lane group takes one row into registers (32 rows x 16 lanes = the
//     workgroup), the staging -- dead from then on -- receives both branches' fp32 gate matrices and LayerNorm vectors, and the
//     group runs the router's row body (csrc/moe_gate_row.h, the one moe_gate16_kernel<8, true, RE, FMT> runs) on its row: hn rows,
//     top-2, and this workgroup's histogram / usage / importance partials at p.hist / p.uimp [blockIdx.x].  Workgroup 0 zeroes the
//     slab cursors for moe_assign_kernel<true>.  The gate data REPLACES the staging: 64 KiB of LDS at E = 8 (as without the
//     routing), 72.4 KiB at E = 16 -- two workgroups per CU either way;
//   * text epilogue (TX: the MoE block's stylization in front of the folded text cross-attention, when the caller passes a
//     StyleText): tiles follow the sample (ceil(S / 32) tiles of ceil(S / tiles) rows, as csrc/sdfold.hip tiles it), the finished
//     rows go back into LDS as the 16-bit rows the store phase writes to out16, and the workgroup runs what sd_fold_kernel runs
//     on them -- scores against K', softmax per (row, head), P V', + bout, LayerNorm -- with the same MFMAs in the same order,
//     K' and V' streamed global -> registers (wave-private: wave w owns score columns 16 w .. and output columns 16 w .. of every
//     128-column slab).  The staging is dead by then: row image 32 KiB | scores 16.5 KiB | P 8 KiB | reductions 2 KiB.
#include <type_traits>

#include "gemm.h"
#include "kernels.h"
#include "moe_gate_row.h"
#include "row.h"

namespace mdm {
namespace {

constexpr int SG_NT = 512, SG_D = 512, SG_NJ = 4;
// RT row tiles (16 rows each) per workgroup: 2 -> 32 rows, <= 128 registers, two workgroups per CU; 4 -> 64 rows, one per CU (half
// the weight bytes per row).  LDS: the fp32 staging of the epilogue (rows x 2 KiB) covers the 16-bit image (rows x 1 KiB).

__device__ __forceinline__ void sg_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// the lane's number in its wave, from the lane count and opaque to the compiler: what an epilogue derives from it is computed
// where it is used instead of living in a register through the phases before, which have none to spare
__device__ __forceinline__ int sg_lane_again() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

struct StyleGemmArgs {
  const void* src;      // fp32 [*, D] or 16-bit rows (format of the launch)
  int64_t M;
  int S;                // frames per sample: row m belongs to sample m / S
  const float *pw, *pb; // optional post_norm (+ L2 normalisation * sqrt(D))
  const float *sw, *sb; // style norm
  const float* sc;      // (B, 2 D) scale | shift
  const int* pos4;      // optional (M, 4): the row is 0.5 * the sum of these four source rows
  const uint16_t* ws;   // weight stream of out_layers.2
  const float* bias;
  const float* resid;   // optional [M, D]
  float out_scale;
  const float* colscale;  // optional [D]
  float* out;
  uint16_t* out16;      // optional 16-bit copy
  // fp32-grade form only (style_gemm3): what may follow the row while it is still on chip.  With r = resid + out_scale * colscale * (...)
  //   skip == NULL: out = r;  ln_out = LN(r; lw, lb) when lw is set                  (the pre-norm of the block that follows)
  //   skip != NULL: out = LN(skip + skip_scale * r; lw, lb)  (r itself is not written);  ln_out = LN(out; l2w, l2b) when l2w is set
  //                 (the tail of DualSelfAttentionBlock behind its second Performer, fast_attention.py:219-225)
  const float *lw, *lb;
  float* ln_out;
  const float* skip;
  float skip_scale;
  const float *l2w, *l2b;
  int ln_x2;  // ln_out as pre-split rows (MDM_OP_X2_ROW) for the GEMM that reads it, instead of fp32
};

struct StyleRouteArgs {  // the routing epilogue's operands (unused where RE == 0)
  MoeGateParams p;
  int* cursor;
};

struct StyleTextArgs {  // the text epilogue's operands (TX forms only): the folded text side as sd_fold_kernel reads it
  const uint16_t* kfold;  // [B][npass][128][D]
  const float* cb;        // [B][npass][128]
  const uint16_t* vfold;  // [B][npass][D][128]
  const float *bout, *ln_w, *ln_b;
  float* o32;      // [M, D] attention output + bout
  uint16_t* ln16;  // [M, D] LayerNorm of it, 16-bit
  int H, N, hpp, npass;
  int ntile, rpt;  // tiles per sample, rows per tile
};
constexpr int SGT_SC_LD = 132;  // fp32 score row stride (floats), as csrc/sdfold.hip
constexpr int sg_text_lds_bytes(int rows) { return rows * 1024 + rows * SGT_SC_LD * 4 + rows * 256 + 2 * rows * 8 * 4; }

// LDS of one workgroup: the fp32 staging, or the router's image where that is larger (RE = 16)
constexpr int sg_lds_bytes(int RT, int RE) {
  return RE > 0 && gate16_lds_bytes(RE, SG_D) > 16 * RT * SG_D * 4 ? gate16_lds_bytes(RE, SG_D) : 16 * RT * SG_D * 4;
}

template <typename HT, bool SRC16, int SG_RT, int RE = 0, bool TX = false>
__global__ __launch_bounds__(SG_NT, (SG_RT <= 2 ? 4 : 2)) void style_gemm_kernel(
    const StyleGemmArgs g, const typename std::conditional<TX, StyleTextArgs, StyleRouteArgs>::type rt) {
  static_assert(!TX || RE == 0, "the text epilogue and the routing epilogue both take the staging");
  constexpr int SG_ROWS = 16 * SG_RT, RPW = SG_ROWS / 8;  // rows per wave in the row phase
  typedef typename HT::frag_t frag_t;
  typedef Row<8, true> R8;
  constexpr int D = SG_D, FMT = HT::FMT;
  extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the tile's rows [row0, mend): flat 32-row tiles, or (TX) tile tl of sample bs -- a tile never crosses a sample
  int64_t row0 = (int64_t)blockIdx.x * SG_ROWS, mend = g.M;
  int bs = 0;
  if constexpr (TX) {
    // consecutive tiles -- the tiles of a sample, which share its K' and V' -- on one XCD, whose L2 then holds them
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    bs = wg / rt.ntile;
    const int t0 = (wg - bs * rt.ntile) * rt.rpt;
    const int nrows = g.S - t0 < rt.rpt ? g.S - t0 : rt.rpt;
    if (nrows <= 0) return;
    row0 = (int64_t)bs * g.S + t0, mend = row0 + nrows;
  }

  // the wave's weight stream: 64 fragments of 1 KiB; the ring's first 8 are requested before the row phase
  const uint8_t* wp = (const uint8_t*)g.ws + (int64_t)wn * 64 * 1024 + lane * 16;
  constexpr int NR = SG_RT <= 2 ? 16 : 8;  // ring depth: with 32 accumulator registers there is room for 16 fragments in flight
  frag_t R[NR];  // the first 8 are requested before the row phase, the rest behind it (the row phase needs the registers)
  constexpr int NPRE = TX ? 6 : 8;  // (the text form keeps more scalars, some of them in a vector register's lanes: 6)
#pragma unroll
  for (int f = 0; f < NPRE; ++f) R[f] = *(const frag_t*)(wp + f * 1024);

  // ---- row phase (csrc/rowwise.hip style_in_rows, one wave per row) ------------------------------------------------------
  {
    R8 pww, pbb, sww, sbb;
    if (g.pw) pww.load(g.pw, D, lane), pbb.load(g.pb, D, lane);
    sww.load(g.sw, D, lane), sbb.load(g.sb, D, lane);
#pragma unroll 2
    for (int q = 0; q < RPW; ++q) {
      const int rl = RPW * wn + q;
      int64_t row = row0 + rl;
      row = row < mend ? row : mend - 1;  // rows past the end: recomputed copies of the last row, never stored
      const float* scb = g.sc + (row / g.S) * 2 * (int64_t)D;
      R8 r, scale, shift;
      scale.load(scb, D, lane);
      shift.load(scb + D, D, lane);
      if (g.pos4) {
        const int p0 = g.pos4[row * 4 + 0], p1 = g.pos4[row * 4 + 1], p2 = g.pos4[row * 4 + 2], p3 = g.pos4[row * 4 + 3];
        R8 a, b, c, d;
        if constexpr (SRC16) {
          const uint16_t* xh = (const uint16_t*)g.src;
          a.template load_h16<FMT>(xh + (int64_t)p0 * D, D, lane);
          b.template load_h16<FMT>(xh + (int64_t)p1 * D, D, lane);
          c.template load_h16<FMT>(xh + (int64_t)p2 * D, D, lane);
          d.template load_h16<FMT>(xh + (int64_t)p3 * D, D, lane);
        } else {
          const float* x = (const float*)g.src;
          a.load(x + (int64_t)p0 * D, D, lane);
          b.load(x + (int64_t)p1 * D, D, lane);
          c.load(x + (int64_t)p2 * D, D, lane);
          d.load(x + (int64_t)p3 * D, D, lane);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) r.e[j] = ((a.e[j] + b.e[j]) + (c.e[j] + d.e[j])) * 0.5f;
      } else {
        if constexpr (SRC16) {
          r.template load_h16<FMT>((const uint16_t*)g.src + row * D, D, lane);
        } else {
          r.load((const float*)g.src + row * D, D, lane);
        }
      }
      if (g.pw) {
        r.layernorm(pww, pbb, D, lane);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += r.e[j] * r.e[j];
        const float inv = sqrtf((float)D) / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
#pragma unroll
        for (int j = 0; j < 8; ++j) r.e[j] *= inv;
      }
      r.layernorm(sww, sbb, D, lane);
#pragma unroll
      for (int j = 0; j < 8; ++j) r.e[j] = silu(r.e[j] * (1.f + scale.e[j]) + shift.e[j]);
      // lane holds columns 4 l .. 4 l + 3 and 256 + 4 l ..: 8 bytes each, 16-B chunks (l >> 1) and 32 + (l >> 1), half l & 1
      uint8_t* ir = smem + rl * 1024 + (lane & 1) * 8;
      *(uint2*)(ir + ((((lane >> 1)) ^ (rl & 15)) << 4)) = make_uint2(HT::pack(r.e[0], r.e[1]), HT::pack(r.e[2], r.e[3]));
      *(uint2*)(ir + (((32 + (lane >> 1)) ^ (rl & 15)) << 4)) = make_uint2(HT::pack(r.e[4], r.e[5]), HT::pack(r.e[6], r.e[7]));
    }
  }
#pragma unroll
  for (int f = NPRE; f < NR; ++f) R[f] = *(const frag_t*)(wp + f * 1024);
  wp += NR * 1024;
  sg_barrier();

  // ---- GEMM phase: y[32 rows x 64 columns of this wave] = image . Wout^T ---------------------------------------------------
  const int frow = lane & 15, fq = lane >> 4;
  f32x4 y[SG_RT][SG_NJ];
#pragma unroll
  for (int i = 0; i < SG_RT; ++i)
#pragma unroll
    for (int j = 0; j < SG_NJ; ++j) y[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const int xb = frow * 1024 + ((fq ^ frow) << 4);  // (row frow, K step 0); step s reads chunk (4 s) ^ (fq ^ frow)
    frag_t A[2][SG_RT];
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) A[0][i] = *(const frag_t*)(smem + xb + i * 16384);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s + 1 < 16) {
#pragma unroll
        for (int i = 0; i < SG_RT; ++i) A[(s + 1) & 1][i] = *(const frag_t*)(smem + (xb ^ (64 * ((s + 1) & 3))) + ((s + 1) >> 2) * 256 + i * 16384);
      }
#pragma unroll
      for (int j = 0; j < SG_NJ; ++j) {
        const int slot = (s * SG_NJ + j) & (NR - 1);
#pragma unroll
        for (int i = 0; i < SG_RT; ++i) y[i][j] = HT::mfma16(R[slot], A[s & 1][i], y[i][j]);
        R[slot] = *(const frag_t*)(wp + slot * 1024);  // the last NR refills read (and discard) the next wave's / the padding
        if (slot == NR - 1) wp += NR * 1024;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: (y + b) * out_scale * colscale staged as fp32 [rows][512], full rows out with the residual -----------------
  sg_barrier();
  float* stg = (float*)smem;
  int frow_e = frow, fq_e = fq;
  if constexpr (TX) {  // (the text form has no register to carry them through the GEMM phase)
    const int l = sg_lane_again();
    frow_e = l & 15, fq_e = l >> 4;
  }
  {
  const int frow = frow_e, fq = fq_e;
#pragma unroll
  for (int j = 0; j < SG_NJ; ++j) {
    const int n = wn * 64 + 16 * j + 4 * fq;
    f32x4 bb = *(const f32x4*)(g.bias + n);
    f32x4 cs = {g.out_scale, g.out_scale, g.out_scale, g.out_scale};
    if (g.colscale) {
      const f32x4 q = *(const f32x4*)(g.colscale + n);
      cs[0] *= q[0], cs[1] *= q[1], cs[2] *= q[2], cs[3] *= q[3];
    }
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) {
      const int ml = i * 16 + frow;
      f32x4 v = y[i][j];
      v[0] = (v[0] + bb[0]) * cs[0], v[1] = (v[1] + bb[1]) * cs[1], v[2] = (v[2] + bb[2]) * cs[2], v[3] = (v[3] + bb[3]) * cs[3];
      *(f32x4*)(stg + ml * D + (((n >> 2) ^ (ml & 31)) << 2)) = v;
    }
  }
  }
  // the thread's residual pieces are all requested before its first store: the residual is usually updated in place (out == resid), so
  // the compiler may not move a row's load above the previous row's store, and on gfx950 stores count in vmcnt -- left in the loop
  // every row waited for the row before it to be written (8 serial write round trips per tile)
  const int ts = TX ? wn * 64 + sg_lane_again() : tid;
  const int cl = ts & 127, n = 4 * cl;
  // (TX) the wave's 16 fragments of K' rows [16 w, 16 w + 16), then of its V' rows: the GEMM accumulators are dead, the first 8
  // fragments of K' are requested here
  [[maybe_unused]] frag_t F[TX ? 16 : 1];
  [[maybe_unused]] uint2 pk[TX ? SG_ROWS / 4 : 1];  // (TX) the thread's pieces of the finished rows, 16-bit
  if constexpr (TX) {
    const uint8_t* kb = (const uint8_t*)(rt.kfold + (int64_t)bs * rt.npass * 128 * D);  // (uniform base + 32-bit lane offset)
    const int ln = ts & 63;
    const uint32_t ko = ((16 * wn + (ln & 15)) * D + 8 * (ln >> 4)) * 2;
#pragma unroll
    for (int f = 0; f < 8; ++f) F[f] = *(const frag_t*)(kb + ko + 64 * f);
  }
  f32x4 q[SG_ROWS / 4];
#pragma unroll
  for (int k = 0; k < SG_ROWS / 4; ++k) {
    int64_t m = row0 + (ts >> 7) + 4 * k;
    m = m < mend ? m : mend - 1;
    q[k] = g.resid ? *(const f32x4*)(g.resid + m * D + n) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  sg_barrier();
#pragma unroll
  for (int k = 0; k < SG_ROWS / 4; ++k) {
    const int ml = (ts >> 7) + 4 * k;
    const int64_t m = row0 + ml;
    if constexpr (!TX) {
      if (m >= mend) continue;
    }
    f32x4 v = *(const f32x4*)(stg + ml * D + ((cl ^ (ml & 31)) << 2));
    if (g.resid) v[0] += q[k][0], v[1] += q[k][1], v[2] += q[k][2], v[3] += q[k][3];
    if constexpr (TX) {  // rows past the end stay copies of the last row for the epilogue; they are not stored
      pk[k] = make_uint2(HT::pack(v[0], v[1]), HT::pack(v[2], v[3]));
      if (m >= mend) continue;
    }
    *(f32x4*)(g.out + m * D + n) = v;
    if (g.out16) *(uint2*)(g.out16 + m * D + n) = make_uint2(HT::pack(v[0], v[1]), HT::pack(v[2], v[3]));
    if constexpr (RE > 0) *(f32x4*)(stg + ml * D + ((cl ^ (ml & 31)) << 2)) = v;  // the finished row, for the router below
  }

  // ---- routing epilogue: the MoE gate on the finished rows (csrc/moe_gate_row.h) --------------------------------------------
  if constexpr (RE > 0) {
    static_assert(SG_ROWS * 16 == SG_NT, "one 16-lane group per row of the tile");
    static_assert(2 * RE * D / 4 % (2 * SG_NT) == 0 && 4 * D / 4 == SG_NT, "staging loops below");
    static_assert(sg_lds_bytes(SG_RT, RE) <= 80 * 1024, "two workgroups per CU");
    constexpr int NV = D / 64, NG = 2 * RE * D / 4 / SG_NT;  // 16-B pieces of the gate matrices per thread
    const MoeGateParams& p = rt.p;
    // the thread index again, from the wave's number and the lane count: nothing of this epilogue is then live in the GEMM phase,
    // which has no register to spare
    const int tid = wn * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    // the gate matrices and LayerNorm vectors are requested now and parked in registers until the staging is free
    // (E = 16: one branch's matrix now, the other's once the rows have left the staging -- 8 pieces beside the 8 of the row spill)
    constexpr int NP = NG <= 4 ? NG : NG / 2;
    f32x4 tg[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) tg[j] = *(const f32x4*)(p.gate_w[j / (NG / 2)] + 4 * (tid + SG_NT * (j % (NG / 2))));
    const int lw = tid >> 7;  // ln_w[0] | ln_w[1] | ln_b[0] | ln_b[1], D / 4 pieces each
    const f32x4 tl = *(const f32x4*)((lw < 2 ? p.ln_w[lw] : p.ln_b[lw - 2]) + 4 * (tid & 127));
    sg_barrier();
    const int l16 = tid & 15;
    const int64_t row = row0 + (tid >> 4);
    const bool ok = row < g.M;
    const int64_t rc = ok ? row : g.M - 1;  // a past-the-end group takes row M - 1, as in moe_gate16_kernel
    const int rl = (int)(rc - row0);
    f32x4 v[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = *(const f32x4*)(stg + rl * D + (((l16 + 16 * c) ^ (rl & 31)) << 2));
    sg_barrier();  // every row is in registers: the staging becomes the router's image (layout of moe_gate16_kernel)
    float* gw = (float*)smem;
    float* lnw = gw + 2 * RE * D;
    float* lnb = lnw + 2 * D;
    int* s_hist = (int*)(lnb + 2 * D);
    float* s_usage = (float*)(s_hist + 32);
    float* s_imp = s_usage + 32;
#pragma unroll
    for (int j = 0; j < NP; ++j) *(f32x4*)(gw + (j / (NG / 2)) * RE * D + 4 * (tid + SG_NT * (j % (NG / 2)))) = tg[j];
    if constexpr (NP < NG) {
#pragma unroll
      for (int j = NP; j < NG; ++j) tg[j - NP] = *(const f32x4*)(p.gate_w[j / (NG / 2)] + 4 * (tid + SG_NT * (j % (NG / 2))));
#pragma unroll
      for (int j = NP; j < NG; ++j) *(f32x4*)(gw + (j / (NG / 2)) * RE * D + 4 * (tid + SG_NT * (j % (NG / 2)))) = tg[j - NP];
    }
    *(f32x4*)(lnw + 4 * tid) = tl;
    if (tid < 32) s_hist[tid] = 0, s_usage[tid] = 0.f, s_imp[tid] = 0.f;
    // the slab cursors of moe_assign_kernel<true>: the previous layer's assign launch has finished in stream order
    if (blockIdx.x == 0 && tid < 2 * RE) rt.cursor[tid] = 0;
    sg_barrier();
    gate16_row<NV, true, RE, FMT, (RE > 8 ? 4 : 16)>(v, gate16_row_sum(v), row, ok, rc, g.M, RE, FMT, l16, gw, lnw, lnb, s_hist, s_usage, s_imp, p);
    __syncthreads();
    if (tid < 2 * RE) {  // per-workgroup partials, summed by moe_assign_kernel<true>
      p.hist[blockIdx.x * 32 + tid] = s_hist[tid];
      p.uimp[blockIdx.x * 64 + tid] = s_usage[tid];
      p.uimp[blockIdx.x * 64 + 32 + tid] = s_imp[tid];
    }
  }

  // ---- text epilogue: the folded text cross-attention and its LayerNorm on the finished rows (csrc/sdfold.hip) --------------
  // sd_fold_kernel's arithmetic element for element -- the same MFMAs with the text fragment first, K ascending in steps of 32,
  // its softmax grouping and loops, its lane <-> column ownership and reduction order in the LayerNorm -- on 32 rows instead of 64
  if constexpr (TX) {
    static_assert(SG_RT == 2 && SG_ROWS * 16 == SG_NT, "32 rows: the softmax has a thread for every (row, head, lane of G)");
    static_assert(sg_text_lds_bytes(SG_ROWS) <= sg_lds_bytes(SG_RT, 0), "the epilogue's images replace the staging");
    uint8_t* const pim = smem + SG_ROWS * 1024 + SG_ROWS * SGT_SC_LD * 4;
    float* const sc = (float*)(smem + SG_ROWS * 1024);
    float* const red1 = (float*)(pim + SG_ROWS * 256);
    float* const red2 = red1 + SG_ROWS * 8;
    // the lane's fragment coordinates again, from the lane count: nothing of this epilogue is then live in the phases before it,
    // which have no register to spare; operands are addressed as a uniform base + a 32-bit lane offset
    const int ln = sg_lane_again();
    const int te0 = wn * 64 + ln, cl = te0 & 127;  // (the thread index, as the store phase has it)
    // K' fragments 8 .. 15 of the first pass take the registers the store phase has just left
    {
      const uint8_t* kb = (const uint8_t*)(rt.kfold + (int64_t)bs * rt.npass * 128 * D);
      const uint32_t ko = ((16 * wn + (ln & 15)) * D + 8 * (ln >> 4)) * 2;
#pragma unroll
      for (int f = 8; f < 16; ++f) F[f] = *(const frag_t*)(kb + ko + 64 * f);
    }
    sg_barrier();  // every thread has its pieces of the staging: the row image takes its place (layout of the row phase's image)
#pragma unroll
    for (int k = 0; k < SG_ROWS / 4; ++k) {
      const int ml = (te0 >> 7) + 4 * k;
      *(uint2*)(smem + ml * 1024 + (((cl >> 1) ^ (ml & 15)) << 4) + (cl & 1) * 8) = pk[k];
    }
    f32x4 o[4][SG_RT];

    // One pass of <= 128 folded columns.  The first pass has the registers for all 16 fragments of K' (requested around the store
    // phase) and then of V' (requested before the softmax): the output accumulators do not exist yet.  A further pass (N > 32 at
    // four heads) walks both through an 8-fragment ring beside them.
    auto text_pass = [&](auto first_c, const int pass) {
      constexpr bool FIRST = decltype(first_c)::value;
      // the thread index is taken again per pass: otherwise every lane-constant address of the softmax is hoisted out of the pass
      // loop and lives in (spilled) registers across it; recomputing is a few instructions
      const int te = wn * 64 + sg_lane_again();
      const int frow = te & 15, fq = (te >> 4) & 3;
      const uint32_t ko = ((16 * wn + frow) * D + 8 * fq) * 2;  // K'[16 w + frow][8 fq ..], + 64 bytes per K step
      const uint32_t vo = ((16 * wn + frow) * 128 + 8 * fq) * 2;  // V'[16 w + frow][8 fq ..], + 32 KiB per slab, + 64 bytes per K step
      const int xb = frow * 1024 + ((fq ^ frow) << 4);  // as in the GEMM phase: K step s reads chunk (4 s) ^ (fq ^ frow)
      const int hcnt = (rt.H - pass * rt.hpp) < rt.hpp ? (rt.H - pass * rt.hpp) : rt.hpp;  // heads of this pass
      const int64_t bp = (int64_t)bs * rt.npass + pass;
      const uint8_t* kb = (const uint8_t*)(rt.kfold + bp * 128 * D);
      const int n0 = 16 * wn + 4 * fq;
      f32x4 cbv;  // (requested ahead of the scores where there is a register for it)
      if constexpr (FIRST) cbv = *(const f32x4*)((const uint8_t*)(rt.cb + bp * 128) + (uint32_t)(4 * n0));
      if constexpr (!FIRST) {
#pragma unroll
        for (int f = 0; f < 8; ++f) F[f] = *(const frag_t*)(kb + ko + 64 * f);
      }
      // zero the probability image (its columns >= hcnt * N stay zero: they multiply the zero padding of V'); the previous
      // pass's readers are behind the barrier that ends it
      uint32_t z = 0;
      asm volatile("" : "+v"(z));  // (a zero made here: hoisted out of the pass loop it is four registers held across it)
      *(uint4*)(pim + te * 16) = make_uint4(z, z, z, z);
      sg_barrier();

      // scores[32 x 128] = rows . K'^T + cb; lane: rows 16 i + frow, columns 16 w + 4 fq ..
      f32x4 acc[SG_RT];
#pragma unroll
      for (int i = 0; i < SG_RT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
#pragma unroll
        for (int i = 0; i < SG_RT; ++i) {
          const frag_t xf = *(const frag_t*)(smem + (xb ^ (64 * (s & 3))) + (s >> 2) * 256 + i * 16384);
          acc[i] = HT::mfma16(F[FIRST ? s : (s & 7)], xf, acc[i]);
        }
        if constexpr (!FIRST) {
          if (s < 8) F[s] = *(const frag_t*)(kb + ko + 64 * (s + 8));
        }
      }
      if constexpr (!FIRST) cbv = *(const f32x4*)((const uint8_t*)(rt.cb + bp * 128) + (uint32_t)(4 * n0));
#pragma unroll
      for (int i = 0; i < SG_RT; ++i) {
        f32x4 v = acc[i];
        v[0] += cbv[0], v[1] += cbv[1], v[2] += cbv[2], v[3] += cbv[3];
        *(f32x4*)(sc + (16 * i + frow) * SGT_SC_LD + n0) = v;
      }
      // the wave's 16 fragments of V': rows 128 sidx + 16 w .. (its output columns) x K step ks, fragment 4 ks + sidx -- in flight
      // across the softmax
      const uint8_t* vb = (const uint8_t*)(rt.vfold + bp * D * 128);
#pragma unroll
      for (int f = 0; f < (FIRST ? 16 : 8); ++f) F[f] = *(const frag_t*)(vb + vo + (f & 3) * 32768 + 64 * (f >> 2));
      sg_barrier();  // scores complete

      // softmax over each head's N key columns, probabilities as 16-bit rows
      {
        // G lanes per (row, head) as sd_fold_kernel has them (8 with one head in the pass, 4 with two, 2 with three or four, 1
        // beyond): the order of a row's sum follows G, so it is not widened for the 32 rows of this tile.  A thread's scores
        // (i = sub, sub + G, ..: at most 128 / (hcnt G) of them) are read once, into registers; max, sum and the probabilities
        // are sd_fold_kernel's, in its order
        auto softmax = [&](auto g_c) {
          constexpr int G = decltype(g_c)::value, SMX = G == 1 ? 25 : (G == 2 ? 21 : 16);
          const int N = rt.N;
          const int unit = te / G, sub = te - unit * G;
          const bool on = unit < SG_ROWS * hcnt;
          const int row = on ? unit / hcnt : 0, h = on ? unit - row * hcnt : 0;
          const float* p = sc + row * SGT_SC_LD + h * N + sub;
          float pv[SMX];
#pragma unroll
          for (int k = 0; k < SMX; ++k) {  // (unconditional reads: past the row they stay inside the workgroup's LDS, and are dropped)
            const float t = p[k * G];
            pv[k] = sub + k * G < N ? t : -INFINITY;
          }
          float mx = -INFINITY;
#pragma unroll
          for (int k = 0; k < SMX; ++k) mx = fmaxf(mx, pv[k]);
#pragma unroll
          for (int o2 = 1; o2 < G; o2 <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
          float sum = 0.f;
#pragma unroll
          for (int k = 0; k < SMX; ++k) {
            pv[k] = exp_fast(pv[k] - mx);
            sum += pv[k];  // (past the head's tokens: exp(-inf) = +0, which leaves the sum as it is)
          }
#pragma unroll
          for (int o2 = 1; o2 < G; o2 <<= 1) sum += __shfl_xor(sum, o2, 64);
          const float inv = 1.f / sum;
          // (unconditional stores: what has no place in the image goes to the thread's own two bytes of the reduction buffers)
          // (the bound is taken on the column, in unsigned arithmetic: the 25 lane masks of the reads above would otherwise be kept
          // for these stores, in scalar registers the kernel does not have)
          uint8_t* const dump = (uint8_t*)red1 + te * 2;
          const uint32_t c0 = (uint32_t)(h * N + sub), cend = on ? (uint32_t)(h * N) + (uint32_t)N : 0u;
#pragma unroll
          for (int k = 0; k < SMX; ++k) {
            const uint32_t c = c0 + (uint32_t)(k * G);
            uint8_t* const dst = pim + row * 256 + ((((c >> 3) ^ (row & 15))) << 4) + (c & 7) * 2;
            *(uint16_t*)(c < cend ? dst : dump) = (uint16_t)(HT::pack(pv[k] * inv, 0.f) & 0xffff);
          }
        };
        const int gq = 8 / hcnt;
        if (gq >= 8) softmax(std::integral_constant<int, 8>{});
        else if (gq >= 4) softmax(std::integral_constant<int, 4>{});
        else if (gq >= 2) softmax(std::integral_constant<int, 2>{});
        else softmax(std::integral_constant<int, 1>{});
      }
      sg_barrier();

      // out[32 x 512] += P . V'^T; every accumulator takes its K steps in ascending order
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        frag_t pf[SG_RT];
#pragma unroll
        for (int i = 0; i < SG_RT; ++i) {
          const int ra = 16 * i + frow;
          pf[i] = *(const frag_t*)(pim + ra * 256 + (((ks * 4 + fq) ^ (ra & 15)) << 4));
        }
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx) {
          const int f = 4 * ks + sidx;
#pragma unroll
          for (int i = 0; i < SG_RT; ++i)
            o[sidx][i] = HT::mfma16(F[FIRST ? f : (f & 7)], pf[i], FIRST && ks == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : o[sidx][i]);
          if constexpr (!FIRST) {
            if (f < 8) F[f] = *(const frag_t*)(vb + vo + sidx * 32768 + 64 * (ks + 2));
          }
        }
      }
      if (pass + 1 < rt.npass) sg_barrier();  // every wave is done with this pass's scores and probability image
    };
    text_pass(std::true_type{}, 0);
#pragma unroll 1
    for (int pass = 1; pass < rt.npass; ++pass) text_pass(std::false_type{}, pass);

    // + bout, LayerNorm over the 512 columns (two passes through LDS across the 8 waves)
    // lane: rows m = 16 i + frow, columns j = 128 s + 16 w + 4 fq + r
    // (the LayerNorm's weights are requested with bout: they arrive behind the two barriers)
    const int te = sg_lane_again();
    const int frow = te & 15, fq = te >> 4;
    f32x4 bov[4], lwv[4], lbv[4];
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
      const uint32_t jo = 4 * (128 * sidx + 16 * wn + 4 * fq);
      bov[sidx] = *(const f32x4*)((const uint8_t*)rt.bout + jo);
      lwv[sidx] = *(const f32x4*)((const uint8_t*)rt.ln_w + jo);
      lbv[sidx] = *(const f32x4*)((const uint8_t*)rt.ln_b + jo);
    }
    float ps[SG_RT];
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) ps[i] = 0.f;
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
      const f32x4 bo = bov[sidx];
#pragma unroll
      for (int i = 0; i < SG_RT; ++i) {
        o[sidx][i][0] += bo[0], o[sidx][i][1] += bo[1], o[sidx][i][2] += bo[2], o[sidx][i][3] += bo[3];
        ps[i] += (o[sidx][i][0] + o[sidx][i][1]) + (o[sidx][i][2] + o[sidx][i][3]);
      }
    }
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) {
      ps[i] += __shfl_xor(ps[i], 16, 64);
      ps[i] += __shfl_xor(ps[i], 32, 64);
      if (fq == 0) red1[(16 * i + frow) * 8 + wn] = ps[i];
    }
    sg_barrier();
    float mean[SG_RT], rstd[SG_RT];
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) {
      const f32x4 a = *(const f32x4*)(red1 + (16 * i + frow) * 8), c = *(const f32x4*)(red1 + (16 * i + frow) * 8 + 4);
      mean[i] = (((a[0] + a[1]) + (a[2] + a[3])) + ((c[0] + c[1]) + (c[2] + c[3]))) * (1.f / D);
      float v = 0.f;
#pragma unroll
      for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = o[sidx][i][r] - mean[i];
          v += d * d;
        }
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (fq == 0) red2[(16 * i + frow) * 8 + wn] = v;
    }
    sg_barrier();
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) {
      const f32x4 a = *(const f32x4*)(red2 + (16 * i + frow) * 8), c = *(const f32x4*)(red2 + (16 * i + frow) * 8 + 4);
      rstd[i] = rsqrtf((((a[0] + a[1]) + (a[2] + a[3])) + ((c[0] + c[1]) + (c[2] + c[3]))) * (1.f / D) + 1e-5f);
    }
    const int nrows = (int)(mend - row0);
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
      const int j = 128 * sidx + 16 * wn + 4 * fq;
      const f32x4 w = lwv[sidx], bb = lbv[sidx];
#pragma unroll
      for (int i = 0; i < SG_RT; ++i) {
        const int m = 16 * i + frow;
        if (m >= nrows) continue;
        const f32x4 v = o[sidx][i];
        *(f32x4*)((uint8_t*)(rt.o32 + row0 * D) + (uint32_t)(4 * (m * D + j))) = v;
        const float y0 = (v[0] - mean[i]) * rstd[i] * w[0] + bb[0], y1 = (v[1] - mean[i]) * rstd[i] * w[1] + bb[1];
        const float y2 = (v[2] - mean[i]) * rstd[i] * w[2] + bb[2], y3 = (v[3] - mean[i]) * rstd[i] * w[3] + bb[3];
        *(uint2*)((uint8_t*)(rt.ln16 + row0 * D) + (uint32_t)(2 * (m * D + j))) = make_uint2(HT::pack(y0, y1), HT::pack(y2, y3));
      }
    }
  }
}

// ---- the same launch in the fp32-grade (bf16x3) arithmetic ---------------------------------------------------------------------
// Row phase in fp32 exactly as above (the source rows are fp32 in these modes); the rows are left as TWO 16-bit images (bf16 hi and
// lo = rn(x - hi)) and every product is three MFMAs (Wh Al + Wl Ah + Wh Ah, small terms first as csrc/gemm3.hip).  Wout streams as
// (hi, lo) fragment PAIRS (mdm_gemm_stream3_pack: per wave the 64 pairs of its 64 columns in K order, 2 KiB per pair).  A weight
// fragment pair feeds 3 RT MFMAs instead of RT: at the same stream rate three times the matrix work of the 16-bit launch, which is
// what this mode's arithmetic costs anyway -- the launch replaces style_in + a 128 x 128-tile bf16x3 GEMM (whose fp32 operand
// tiles cross L2 -> LDS four times) and the fp32 [M, D] tensor between them.
template <int SG_RT>
__global__ __launch_bounds__(SG_NT, (SG_RT <= 2 ? 4 : 2)) void style_gemm3_kernel(const StyleGemmArgs g) {
  constexpr int SG_ROWS = 16 * SG_RT, RPW = SG_ROWS / 8;
  typedef HB::frag_t frag_t;
  typedef Row<8, true> R8;
  constexpr int D = SG_D, IMG = SG_ROWS * 1024;
  extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];
  uint8_t* const imh = smem;
  uint8_t* const iml = smem + IMG;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * SG_ROWS;

  // the wave's stream: 64 (hi, lo) pairs = 128 fragments of 1 KiB; fragment f of the stream refills ring slot f % NR
  const uint8_t* wp = (const uint8_t*)g.ws + (int64_t)wn * 128 * 1024 + lane * 16;
  constexpr int NR = SG_RT <= 2 ? 8 : 16;
  frag_t R[NR];
#pragma unroll
  for (int f = 0; f < (NR < 8 ? NR : 8); ++f) R[f] = *(const frag_t*)(wp + f * 1024);

  {
    R8 pww, pbb, sww, sbb;
    if (g.pw) pww.load(g.pw, D, lane), pbb.load(g.pb, D, lane);
    sww.load(g.sw, D, lane), sbb.load(g.sb, D, lane);
#pragma unroll 2
    for (int q = 0; q < RPW; ++q) {
      const int rl = RPW * wn + q;
      int64_t row = row0 + rl;
      row = row < g.M ? row : g.M - 1;
      const float* scb = g.sc + (row / g.S) * 2 * (int64_t)D;
      R8 r, scale, shift;
      scale.load(scb, D, lane);
      shift.load(scb + D, D, lane);
      const float* x = (const float*)g.src;
      if (g.pos4) {
        const int p0 = g.pos4[row * 4 + 0], p1 = g.pos4[row * 4 + 1], p2 = g.pos4[row * 4 + 2], p3 = g.pos4[row * 4 + 3];
        R8 a, b, c, d;
        a.load(x + (int64_t)p0 * D, D, lane);
        b.load(x + (int64_t)p1 * D, D, lane);
        c.load(x + (int64_t)p2 * D, D, lane);
        d.load(x + (int64_t)p3 * D, D, lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) r.e[j] = ((a.e[j] + b.e[j]) + (c.e[j] + d.e[j])) * 0.5f;
      } else {
        r.load(x + row * D, D, lane);
      }
      if (g.pw) {
        r.layernorm(pww, pbb, D, lane);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += r.e[j] * r.e[j];
        const float inv = sqrtf((float)D) / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
#pragma unroll
        for (int j = 0; j < 8; ++j) r.e[j] *= inv;
      }
      r.layernorm(sww, sbb, D, lane);
#pragma unroll
      for (int j = 0; j < 8; ++j) r.e[j] = silu(r.e[j] * (1.f + scale.e[j]) + shift.e[j]);
      uint32_t h0, h1, h2, h3, l0, l1, l2, l3;
      split_bf16(r.e[0], r.e[1], h0, l0);
      split_bf16(r.e[2], r.e[3], h1, l1);
      split_bf16(r.e[4], r.e[5], h2, l2);
      split_bf16(r.e[6], r.e[7], h3, l3);
      const int o0 = rl * 1024 + ((((lane >> 1)) ^ (rl & 15)) << 4) + (lane & 1) * 8;
      const int o1 = rl * 1024 + (((32 + (lane >> 1)) ^ (rl & 15)) << 4) + (lane & 1) * 8;
      *(uint2*)(imh + o0) = make_uint2(h0, h1), *(uint2*)(imh + o1) = make_uint2(h2, h3);
      *(uint2*)(iml + o0) = make_uint2(l0, l1), *(uint2*)(iml + o1) = make_uint2(l2, l3);
    }
  }
#pragma unroll
  for (int f = 8; f < NR; ++f) R[f] = *(const frag_t*)(wp + f * 1024);
  wp += NR * 1024;
  sg_barrier();

  const int frow = lane & 15, fq = lane >> 4;
  f32x4 y[SG_RT][SG_NJ];
#pragma unroll
  for (int i = 0; i < SG_RT; ++i)
#pragma unroll
    for (int j = 0; j < SG_NJ; ++j) y[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const int xb = frow * 1024 + ((fq ^ frow) << 4);
    frag_t Ah[2][SG_RT], Al[2][SG_RT];
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) Ah[0][i] = *(const frag_t*)(imh + xb + i * 16384), Al[0][i] = *(const frag_t*)(iml + xb + i * 16384);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s + 1 < 16) {
#pragma unroll
        for (int i = 0; i < SG_RT; ++i) {
          const int off = (xb ^ (64 * ((s + 1) & 3))) + ((s + 1) >> 2) * 256 + i * 16384;
          Ah[(s + 1) & 1][i] = *(const frag_t*)(imh + off), Al[(s + 1) & 1][i] = *(const frag_t*)(iml + off);
        }
      }
#pragma unroll
      for (int j = 0; j < SG_NJ; ++j) {
        const int slot = (2 * (s * SG_NJ + j)) & (NR - 1);
#pragma unroll
        for (int i = 0; i < SG_RT; ++i) {
          y[i][j] = HB::mfma16(R[slot], Al[s & 1][i], y[i][j]);
          y[i][j] = HB::mfma16(R[slot + 1], Ah[s & 1][i], y[i][j]);
          y[i][j] = HB::mfma16(R[slot], Ah[s & 1][i], y[i][j]);
        }
        R[slot] = *(const frag_t*)(wp + slot * 1024);  // the last NR refills read (and discard) the next wave's / the padding
        R[slot + 1] = *(const frag_t*)(wp + (slot + 1) * 1024);
        if (slot + 2 == NR) wp += NR * 1024;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  sg_barrier();
  float* stg = (float*)smem;
#pragma unroll
  for (int j = 0; j < SG_NJ; ++j) {
    const int n = wn * 64 + 16 * j + 4 * fq;
    f32x4 bb = *(const f32x4*)(g.bias + n);
    f32x4 cs = {g.out_scale, g.out_scale, g.out_scale, g.out_scale};
    if (g.colscale) {
      const f32x4 q = *(const f32x4*)(g.colscale + n);
      cs[0] *= q[0], cs[1] *= q[1], cs[2] *= q[2], cs[3] *= q[3];
    }
#pragma unroll
    for (int i = 0; i < SG_RT; ++i) {
      const int ml = i * 16 + frow;
      f32x4 v = y[i][j];
      v[0] = (v[0] + bb[0]) * cs[0], v[1] = (v[1] + bb[1]) * cs[1], v[2] = (v[2] + bb[2]) * cs[2], v[3] = (v[3] + bb[3]) * cs[3];
      *(f32x4*)(stg + ml * D + (((n >> 2) ^ (ml & 31)) << 2)) = v;
    }
  }
  sg_barrier();
  {
    // one wave per row (lane: columns 4 l .. 4 l + 3 and 256 + 4 l ..): the residual / skip operands of the wave's rows are all
    // requested first (one memory round trip per wave), then row by row: residual, optional block tail and LayerNorms, stores
    R8 xr[RPW], sk[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      int64_t m = row0 + RPW * wn + q;
      m = m < g.M ? m : g.M - 1;
      if (g.resid) xr[q].load(g.resid + m * D, D, lane);
      if (g.skip) sk[q].load(g.skip + m * D, D, lane);
    }
    R8 lww, lbb, l2ww, l2bb;
    if (g.lw) lww.load(g.lw, D, lane), lbb.load(g.lb, D, lane);
    if (g.l2w) l2ww.load(g.l2w, D, lane), l2bb.load(g.l2b, D, lane);
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      const int rl = RPW * wn + q;
      const int64_t m = row0 + rl;
      if (m >= g.M) continue;  // (wave-uniform)
      const f32x4 v0 = *(const f32x4*)(stg + rl * D + ((lane ^ (rl & 31)) << 2));
      const f32x4 v1 = *(const f32x4*)(stg + rl * D + (((64 + lane) ^ (rl & 31)) << 2));
      R8 r;
      r.e[0] = v0[0], r.e[1] = v0[1], r.e[2] = v0[2], r.e[3] = v0[3], r.e[4] = v1[0], r.e[5] = v1[1], r.e[6] = v1[2], r.e[7] = v1[3];
      if (g.resid) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r.e[j] += xr[q].e[j];
      }
      if (g.skip) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r.e[j] = sk[q].e[j] + g.skip_scale * r.e[j];
        r.layernorm(lww, lbb, D, lane);
        r.store(g.out + m * D, D, lane);
        if (g.l2w) {
          r.layernorm(l2ww, l2bb, D, lane);
          if (g.ln_x2) r.store_x2((uint16_t*)g.ln_out + m * 2 * D, D, lane);
          else r.store(g.ln_out + m * D, D, lane);
        }
      } else {
        r.store(g.out + m * D, D, lane);
        if (g.lw) {
          r.layernorm(lww, lbb, D, lane);
          if (g.ln_x2) r.store_x2((uint16_t*)g.ln_out + m * 2 * D, D, lane);
          else r.store(g.ln_out + m * D, D, lane);
        }
      }
    }
  }
}

// stream3[wave w][pair p = 4 s + j][plane hi | lo][lane l][8]:  bf16 hi / lo of W[64 w + 16 j + (l & 15)][32 s + 8 (l >> 4) + e]
__global__ __launch_bounds__(256) void gemm_stream3_pack_kernel(const float* w, uint16_t* out) {
  for (int fi = blockIdx.x * 4 + (threadIdx.x >> 6); fi < 8 * 64; fi += gridDim.x * 4) {
    const int l = threadIdx.x & 63, wv = fi >> 6, f = fi & 63, s = f >> 2, j = f & 3;
    const float* src = w + (int64_t)(64 * wv + 16 * j + (l & 15)) * SG_D + 32 * s + 8 * (l >> 4);
    uint4 h, lo;
    split_bf16(src[0], src[1], h.x, lo.x);
    split_bf16(src[2], src[3], h.y, lo.y);
    split_bf16(src[4], src[5], h.z, lo.z);
    split_bf16(src[6], src[7], h.w, lo.w);
    *(uint4*)(out + (int64_t)fi * 1024 + l * 8) = h;
    *(uint4*)(out + (int64_t)fi * 1024 + 512 + l * 8) = lo;
  }
}

// stream[wave w][fragment f = 4 s + j][lane l][8]:  W[64 w + 16 j + (l & 15)][32 s + 8 (l >> 4) + e]   (N = 512, K = 512)
template <typename HT>
__global__ __launch_bounds__(256) void gemm_stream_pack_kernel(const float* w, uint16_t* out) {
  for (int fi = blockIdx.x * 4 + (threadIdx.x >> 6); fi < 8 * 64; fi += gridDim.x * 4) {
    const int l = threadIdx.x & 63, wv = fi >> 6, f = fi & 63, s = f >> 2, j = f & 3;
    const float* src = w + (int64_t)(64 * wv + 16 * j + (l & 15)) * SG_D + 32 * s + 8 * (l >> 4);
    uint4 o;
    o.x = HT::pack(src[0], src[1]), o.y = HT::pack(src[2], src[3]), o.z = HT::pack(src[4], src[5]), o.w = HT::pack(src[6], src[7]);
    *(uint4*)(out + (int64_t)fi * 512 + l * 8) = o;
  }
}

}  // namespace

int64_t gemm_stream_elems(int N, int K) { return (N == SG_D && K == SG_D) ? (int64_t)N * K + 16 * 512 : 0; }  // + the ring's overrun

int gemm_stream_pack(const float* w, int N, int K, int h16, uint16_t* out, hipStream_t stream) {
  if (!w || !out || N != SG_D || K != SG_D) return MDM_ERR_UNSUPPORTED;
  if (hipMemsetAsync(out + (int64_t)N * K, 0, 16 * 512 * sizeof(uint16_t), stream) != hipSuccess) return MDM_ERR_LAUNCH;
  if (h16 == MDM_H16_F16) {
    hipLaunchKernelGGL(gemm_stream_pack_kernel<HF>, dim3(128), dim3(256), 0, stream, w, out);
  } else {
    hipLaunchKernelGGL(gemm_stream_pack_kernel<HB>, dim3(128), dim3(256), 0, stream, w, out);
  }
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

bool style_gemm_supported(int D, int64_t M) { return D == SG_D && M > 0 && M / 32 < (1ll << 30); }


template <int RT, int RE = 0>
static int launch_style_gemm(const StyleGemmArgs& g, const StyleRouteArgs& rt, bool src16, int h16, hipStream_t s) {
  constexpr int smem = sg_lds_bytes(RT, RE);
  static DevOnce attr;
  if (!attr) {
    const void* fns[4] = {(const void*)style_gemm_kernel<HB, true, RT, RE>, (const void*)style_gemm_kernel<HB, false, RT, RE>,
                          (const void*)style_gemm_kernel<HF, true, RT, RE>, (const void*)style_gemm_kernel<HF, false, RT, RE>};
    for (const void* fn : fns)
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) return MDM_ERR_LAUNCH;
    attr = true;
  }
  const dim3 grid((unsigned)((g.M + 16 * RT - 1) / (16 * RT)));
  if (h16 == MDM_H16_F16) {
    if (src16) hipLaunchKernelGGL((style_gemm_kernel<HF, true, RT, RE>), grid, dim3(SG_NT), smem, s, g, rt);
    else hipLaunchKernelGGL((style_gemm_kernel<HF, false, RT, RE>), grid, dim3(SG_NT), smem, s, g, rt);
  } else {
    if (src16) hipLaunchKernelGGL((style_gemm_kernel<HB, true, RT, RE>), grid, dim3(SG_NT), smem, s, g, rt);
    else hipLaunchKernelGGL((style_gemm_kernel<HB, false, RT, RE>), grid, dim3(SG_NT), smem, s, g, rt);
  }
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

// The text epilogue: 16-bit source rows, 32-row tiles that follow the sample
static int launch_style_gemm_text(const StyleGemmArgs& g, const StyleTextArgs& tx, int64_t B, int h16, hipStream_t s) {
  constexpr int smem = sg_lds_bytes(2, 0);
  static DevOnce attr;
  if (!attr) {
    const void* fns[2] = {(const void*)style_gemm_kernel<HB, true, 2, 0, true>, (const void*)style_gemm_kernel<HF, true, 2, 0, true>};
    for (const void* fn : fns)
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) return MDM_ERR_LAUNCH;
    attr = true;
  }
  const dim3 grid((unsigned)(B * tx.ntile));
  if (h16 == MDM_H16_F16) hipLaunchKernelGGL((style_gemm_kernel<HF, true, 2, 0, true>), grid, dim3(SG_NT), smem, s, g, tx);
  else hipLaunchKernelGGL((style_gemm_kernel<HB, true, 2, 0, true>), grid, dim3(SG_NT), smem, s, g, tx);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

// whole samples of S rows, a text side sd_fold itself would take, a grid that fits
bool style_gemm_text_supported(int D, int64_t M, int S, int H, int N) {
  return style_gemm_supported(D, M) && S > 0 && M % S == 0 && sd_fold_supported(D, H, N) && (M / S) * ((S + 31) / 32) < (1ll << 30);
}

// The routing epilogue exists for E = 8 / 16 with hn rows in the launch's own 16-bit format; its partials are indexed by workgroup,
// so the grid has to fit the partial buffers ([1024][32] / [1024][64])
bool style_gemm_route_supported(int D, int64_t M, int E, int hn_fmt, int h16) {
  return style_gemm_supported(D, M) && (E == 8 || E == 16) && hn_fmt == h16 && (h16 == MDM_H16_BF16 || h16 == MDM_H16_F16) &&
         style_gemm_route_parts(M) <= 1024;
}
int64_t style_gemm_route_parts(int64_t M) { return (M + 31) / 32; }

// src_fmt: 0 = fp32 source rows, else the launch's 16-bit format (must equal h16)
int style_gemm(const void* src, int src_fmt, int64_t M, int D, int S, const float* pw, const float* pb, const float* sw, const float* sb,
               const float* sc, const int* pos4, const uint16_t* ws, const float* bias, const float* resid, float out_scale,
               const float* colscale, float* out, uint16_t* out16, int h16, hipStream_t s, const StyleRoute* route, const StyleText* text) {
  if (M <= 0) return MDM_OK;
  if (!style_gemm_supported(D, M)) return MDM_ERR_UNSUPPORTED;
  if (!src || !sw || !sb || !sc || !ws || !bias || !out || S <= 0 || (pw && !pb)) return MDM_ERR_ARG;
  if ((h16 != MDM_H16_BF16 && h16 != MDM_H16_F16) || (src_fmt != 0 && src_fmt != h16) || ((uintptr_t)ws & 15)) return MDM_ERR_ARG;
  StyleGemmArgs g = {};
  g.src = src, g.M = M, g.S = S, g.pw = pw, g.pb = pb, g.sw = sw, g.sb = sb, g.sc = sc, g.pos4 = pos4, g.ws = ws, g.bias = bias;
  g.resid = resid, g.out_scale = out_scale, g.colscale = colscale, g.out = out, g.out16 = out16;
  // 64-row tiles (one workgroup per CU, half the weight bytes per row) measured 1 % of a step SLOWER than two co-resident 32-row
  // workgroups per CU at 12544 rows; a row's arithmetic does not depend on the tile height
  if (text) {
    const StyleText& t = *text;
    if (route || src_fmt == 0) return MDM_ERR_UNSUPPORTED;
    if (!style_gemm_text_supported(D, M, S, t.H, t.N)) return MDM_ERR_UNSUPPORTED;
    if (!t.kfold || !t.cb || !t.vfold || !t.bout || !t.ln_w || !t.ln_b || !t.o32 || !t.ln16 || ((uintptr_t)t.kfold & 15) ||
        ((uintptr_t)t.vfold & 15) || ((uintptr_t)t.cb & 15) || ((uintptr_t)t.bout & 15) || ((uintptr_t)t.ln_w & 15) || ((uintptr_t)t.ln_b & 15))
      return MDM_ERR_ARG;
    if (t.hpp != sd_fold_heads_per_pass(t.H, t.N) || t.npass != sd_fold_passes(t.H, t.N)) return MDM_ERR_ARG;
    StyleTextArgs tx = {};
    tx.kfold = t.kfold, tx.cb = t.cb, tx.vfold = t.vfold, tx.bout = t.bout, tx.ln_w = t.ln_w, tx.ln_b = t.ln_b, tx.o32 = t.o32, tx.ln16 = t.ln16;
    tx.H = t.H, tx.N = t.N, tx.hpp = t.hpp, tx.npass = t.npass;
    tx.ntile = (S + 31) / 32, tx.rpt = (S + tx.ntile - 1) / tx.ntile;
    return launch_style_gemm_text(g, tx, M / S, h16, s);
  }
  StyleRouteArgs rt = {};
  if (route) {
    if (!route->gate || !route->cursor) return MDM_ERR_ARG;
    const MoeGateParams& p = *route->gate;
    if (!style_gemm_route_supported(D, M, route->E, p.hn_bf16, h16)) return MDM_ERR_UNSUPPORTED;
    if (!p.hn || !p.hist || !p.uimp || !p.top_idx || !p.top_val) return MDM_ERR_ARG;
    for (int b = 0; b < 2; ++b)
      if (!p.ln_w[b] || !p.ln_b[b] || !p.gate_w[b] || !p.gate_b[b] || ((uintptr_t)p.gate_w[b] & 15) || ((uintptr_t)p.ln_w[b] & 15) ||
          ((uintptr_t)p.ln_b[b] & 15))
        return MDM_ERR_ARG;
    rt.p = p, rt.cursor = route->cursor;
    return route->E == 8 ? launch_style_gemm<2, 8>(g, rt, src_fmt != 0, h16, s) : launch_style_gemm<2, 16>(g, rt, src_fmt != 0, h16, s);
  }
  return launch_style_gemm<2>(g, rt, src_fmt != 0, h16, s);
}

// ---- fp32-grade form ---------------------------------------------------------------------------------------------------------
int64_t gemm_stream3_elems(int N, int K) { return (N == SG_D && K == SG_D) ? 2 * (int64_t)N * K + 16 * 512 : 0; }

int gemm_stream3_pack(const float* w, int N, int K, uint16_t* out, hipStream_t stream) {
  if (!w || !out || N != SG_D || K != SG_D) return MDM_ERR_UNSUPPORTED;
  if (hipMemsetAsync(out + 2 * (int64_t)N * K, 0, 16 * 512 * sizeof(uint16_t), stream) != hipSuccess) return MDM_ERR_LAUNCH;
  hipLaunchKernelGGL(gemm_stream3_pack_kernel, dim3(128), dim3(256), 0, stream, w, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

template <int RT>
static int launch_style_gemm3(const StyleGemmArgs& g, hipStream_t s) {
  constexpr int smem = 16 * RT * SG_D * 4;  // hi | lo images = the fp32 staging of the epilogue
  static DevOnce attr;
  if (!attr) {
    if (hipFuncSetAttribute((const void*)style_gemm3_kernel<RT>, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) return MDM_ERR_LAUNCH;
    attr = true;
  }
  const dim3 grid((unsigned)((g.M + 16 * RT - 1) / (16 * RT)));
  hipLaunchKernelGGL((style_gemm3_kernel<RT>), grid, dim3(SG_NT), smem, s, g);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

// fp32 source rows, fp32 output; ws3 = the (hi, lo) pair stream of mdm_gemm_stream3_pack.  32-row tiles (two workgroups per CU) at
// every size: 64-row tiles (one per CU, half the weight bytes per row) measured 1 % of a step slower at the full time scale
// (10.18 vs 10.06 ms) -- as in the 16-bit form, a second resident workgroup hides more than the halved stream saves.  A row's
// arithmetic does not depend on the tile height.
int style_gemm3(const float* src, int64_t M, int D, int S, const float* pw, const float* pb, const float* sw, const float* sb,
                const float* sc, const int* pos4, const uint16_t* ws3, const float* bias, const float* resid, float out_scale,
                const float* colscale, float* out, const StyleTail3& t, hipStream_t s) {
  if (M <= 0) return MDM_OK;
  if (!style_gemm_supported(D, M)) return MDM_ERR_UNSUPPORTED;
  if (!src || !sw || !sb || !sc || !ws3 || !bias || !out || S <= 0 || (pw && !pb) || ((uintptr_t)ws3 & 15)) return MDM_ERR_ARG;
  if ((t.lw && !t.lb) || (t.skip && (!t.lw || !t.lb)) || (t.l2w && (!t.l2b || !t.skip)) || ((t.skip ? t.l2w != nullptr : t.lw != nullptr) != (t.ln_out != nullptr)))
    return MDM_ERR_ARG;
  StyleGemmArgs g = {};
  g.src = src, g.M = M, g.S = S, g.pw = pw, g.pb = pb, g.sw = sw, g.sb = sb, g.sc = sc, g.pos4 = pos4, g.ws = ws3, g.bias = bias;
  g.resid = resid, g.out_scale = out_scale, g.colscale = colscale, g.out = out;
  g.lw = t.lw, g.lb = t.lb, g.ln_out = t.ln_out, g.skip = t.skip, g.skip_scale = t.skip_scale, g.l2w = t.l2w, g.l2b = t.l2b, g.ln_x2 = t.ln_x2;
  return launch_style_gemm3<2>(g, s);
}

}  // namespace mdm
