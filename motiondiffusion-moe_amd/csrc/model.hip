// Host-side orchestration of one denoiser forward: a straight-line sequence of stream-ordered kernel
// launches (no allocation, no host sync) so that a whole sampling step can be captured into a hipGraph.
// Reference arithmetic: text2motion/models/transformer.py:291-361 and the blocks it calls (cited inline).
#include <type_traits>

#include "gemm.h"
#include "kernels.h"

namespace mdm {
namespace {

#define MDM_TRY(expr)            \
  do {                           \
    int st__ = (expr);           \
    if (st__ != MDM_OK) return st__; \
  } while (0)

// ---- measurement probe (mdm_probe_enable / mdm_probe_read): HIP events around the dominant kernel's launches -------
constexpr int PROBE_MAX = 64;
struct Probe {
  bool on = false;
  int n = 0;
  hipEvent_t a[PROBE_MAX], b[PROBE_MAX];
  int rows[PROBE_MAX];
  bool made = false;
};
Probe g_probe;
// the probe's bracket around the launches it times (nothing while it is off or full)
bool probe_armed() { return g_probe.on && g_probe.n < PROBE_MAX; }
int probe_begin(hipStream_t s) { return probe_armed() && hipEventRecord(g_probe.a[g_probe.n], s) != hipSuccess ? MDM_ERR_LAUNCH : MDM_OK; }
int probe_end(hipStream_t s, int rows) {
  if (!probe_armed()) return MDM_OK;
  if (hipEventRecord(g_probe.b[g_probe.n], s) != hipSuccess) return MDM_ERR_LAUNCH;
  g_probe.rows[g_probe.n++] = rows;
  return MDM_OK;
}
int32_t* g_route_dump = nullptr;  // mdm_route_dump: where the router's top-2 indices of every layer are copied (tests)
int64_t g_route_cap = 0;           // its capacity in int32 elements: a forward that would write past it is refused

struct Bump {  // carve the caller's workspace; with base == nullptr it only measures
  uint8_t* base;
  int64_t off = 0;
  explicit Bump(void* b) : base((uint8_t*)b) {}
  template <typename T>
  T* take(int64_t n) {
    off = (off + 255) & ~(int64_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += n * (int64_t)sizeof(T);
    return p;
  }
};

// The sub-buffers of the workspace, in carve order: X(element type, field, element count).  The counts are expressions over the
// locals of carve() (M = B * T rows, D, F, Te = 4 D, nblk = 8 L, dh = D / H, NN = max(N, 1), BN = B * NN, smax = max(Te, 2 D)).
// This one table declares Work, carves it, and describes it to the tests (mdm_workspace_layout / mdm_workspace_field_name).
//   token-major activations (M rows); x?16 / h016: bf16 shadows of the fp32 residual stream, written by the producing GEMM's
//   epilogue in the throughput mode so that the next GEMM streams bf16 straight into LDS;  top_idx .. len_low: the router;
//   s_a .. gvtmp: the stem (B rows);  tn, kb, vb: text cache scratch
#define MDM_WORK_FIELDS(X)                                                                                              \
  X(float, xa, M * D) X(float, xb, M * D) X(float, h0, M * D)                                                           \
  X(uint16_t, xa16, M * D) X(uint16_t, xb16, M * D) X(uint16_t, h016, M * D)                                            \
  X(float, t1, M * D) X(float, t2, M * D) X(float, t3, M * D) X(float, t4, M * D) X(float, t5, M * D)                   \
  X(float, qkv, M * 3 * D) X(float, phi, M * 2 * D) X(float, kvt, (int64_t)B * m.H * dh * dh) X(float, scr, M * m.H * NN) \
  X(float, f1, M * 4 * D) X(float, hn, 2 * M * D) X(float, hid, 4 * M * F) X(float, y2, 4 * M * D)                      \
  X(int, top_idx, 4 * M) X(float, top_val, 4 * M) X(int, perm, 4 * M) X(float, rowscale, 4 * M) X(int, pos4, 4 * M)    \
  X(float, hn_scale, 2 * M)                                                                                             \
  X(int, hist, 1024 * 32) X(float, uimp, 1024 * 64) X(int, goff, 2 * m.E + 1) X(int, cursor, 2 * m.E) X(int, len_low, B) \
  X(float, s_a, B * smax) X(float, s_b, B * smax) X(float, s_c, B * smax) X(float, emb, B * D)                          \
  X(float, e1, B * nblk * Te) X(float, sc, nblk * B * 2 * D) X(float, gvtmp, D)                                         \
  X(float, tn, BN * m.Dt) X(float, kb, BN * D) X(float, vb, BN * D)

struct Work {
#define X(T, f, n) T* f;
  MDM_WORK_FIELDS(X)
#undef X
  int64_t bytes;
};

#define X(T, f, n) #f,
const char* const kWorkFieldNames[] = {MDM_WORK_FIELDS(X)};
#undef X
constexpr int kWorkFields = sizeof(kWorkFieldNames) / sizeof(kWorkFieldNames[0]);

struct WorkLayout {  // what carve() tells mdm_workspace_layout: the first `cap` of the fields it took
  int64_t* off;
  int64_t* bytes;
  int32_t* kind;  // 0 = data (fp32 or a narrower float format, by mode), 1 = int32 indices / counters
  int cap;
  int count = 0;
  void add(int64_t o, int64_t b, bool is_int) {
    if (count < cap) off[count] = o, bytes[count] = b, kind[count] = is_int ? 1 : 0;
    ++count;
  }
};

Work carve(const MdmModel& m, int B, int T, int N, void* ws, WorkLayout* lay = nullptr) {
  Work w;
  Bump b(ws);
  const int64_t M = (int64_t)B * T, D = m.D, F = m.F, Te = 4 * D, nblk = 8 * m.L;
  const int64_t dh = m.D / m.H, NN = N > 0 ? N : 1, BN = B * NN, smax = Te > 2 * D ? Te : 2 * D;
#define X(Ty, f, cnt)       \
  w.f = b.take<Ty>(cnt);    \
  if (lay) lay->add(b.off - (int64_t)(cnt) * (int64_t)sizeof(Ty), (int64_t)(cnt) * (int64_t)sizeof(Ty), std::is_same<Ty, int>::value);
  MDM_WORK_FIELDS(X)
#undef X
  w.bytes = (b.off + 255) & ~(int64_t)255;
  return w;
}

struct Ctx {
  const MdmModel* m;
  hipStream_t s;
  int prec;         // GEMMs with fp32 activations: 1 = single bf16 pass, 3 = bf16x3
  bool bf;          // throughput modes (precision 1 / 2): GEMM-only tensors are kept in 16 bits
  int h16;          // the 16-bit format of this run: MDM_H16_BF16 (precision 1, 3) or MDM_H16_F16 (precision 2, 4)
  bool mix;         // precision 4: fp32-grade flow, but expert MLPs + the 4x FFN run as ONE fp16 pass on 16-bit operands
  bool fp8;         // precision 5: as 2, expert GEMMs on e4m3 operands (csrc/gemm8.hip)
  bool x2;          // fp32-grade GEMM chains: a tensor whose only consumer is a bf16x3 GEMM is written PRE-SPLIT by its producer
                    // (MDM_OP_X2_ROW rows: same bytes as fp32) -- the GEMM then does not re-split every fragment in its K loop
                    // (MDM_VAR_X3_F32_ROWS: off)
  int B, S, N;      // batch, frames at this scale, text tokens
  const int32_t* ntok = nullptr;  // per-sample text token counts [B] (MdmTextCache.ntok), or null: all N
  int64_t M;        // B*S
  const int* len;   // lengths at this scale
  Work w;
};

inline Operand packed(const MdmPacked& p) { return op_bf16(p.hi, p.lo, p.ld); }

// bf16 activation plumbing needs every GEMM K (D, 2D, 4D, F) to be a multiple of the 64-wide LDS-DMA k-tile
bool use_bf16_acts(const MdmModel* m, int precision) {
  return (precision == MDM_PREC_BF16 || precision == MDM_PREC_F16) && m->D % 64 == 0 && m->F % 64 == 0;
}
// precision (include/mdm_hip.h: MDM_PREC_*) -> how this run computes; false = unsupported combination
bool set_precision(Ctx& c, const MdmModel* m, int precision) {
  c.mix = false, c.bf = false, c.fp8 = false, c.h16 = MDM_H16_BF16;
  // (MDM_VAR_X3_REG puts the fp32-grade Linears on the register-staged kernel, which reads fp32 rows only)
  c.x2 = (precision == MDM_PREC_X3 || precision == MDM_PREC_MIXED) && g_variant != MDM_VAR_X3_F32_ROWS && g_variant != MDM_VAR_X3_REG &&
         (m->D == 256 || m->D == 512 || m->D == 1024) && m->F % 32 == 0;
  switch (precision) {
    case MDM_PREC_FP8:  // the fp16 throughput mode with fp8 expert GEMMs (K = D and K = F must be multiples of 128)
      c.prec = 1, c.bf = use_bf16_acts(m, MDM_PREC_F16), c.h16 = MDM_H16_F16, c.fp8 = true;
      return c.bf && m->D % 128 == 0 && m->F % 128 == 0;
    case MDM_PREC_BF16: c.prec = 1, c.bf = use_bf16_acts(m, precision); return true;
    case MDM_PREC_F16:  // fp16 weight planes are only readable by the 16-bit-activation kernels
      c.prec = 1, c.bf = use_bf16_acts(m, precision), c.h16 = MDM_H16_F16;
      return c.bf;
    case MDM_PREC_X3: c.prec = 3; return true;
    case MDM_PREC_MIXED:
      c.prec = 3, c.h16 = MDM_H16_F16, c.mix = m->D % 64 == 0 && m->F % 64 == 0;
      return c.mix;
    default: return false;
  }
}
inline GemmArgs gd(const Ctx& c) {  // GEMM descriptor defaults of this run
  GemmArgs g = gemm_defaults(c.prec);
  g.h16 = c.h16;
  return g;
}
// the mode combinations the choosers and block bodies below ask about
inline bool x3_flow(const Ctx& c) { return !c.bf && c.prec == 3; }  // fp32-grade flow: fp32 activations, bf16x3 GEMMs
inline bool x2_rows(const Ctx& c) { return !c.bf && c.x2; }         // ... its GEMM-only tensors written as pre-split rows
inline bool mlp16(const Ctx& c) { return c.bf || c.mix; }           // expert-MLP / 4x FFN operands in 16 bits
inline bool mlp_x2(const Ctx& c) { return x2_rows(c) && !c.mix; }   // ... else pre-split (x2 implies D % 64 == 0)
inline int fmt16(const Ctx& c) { return c.bf ? c.h16 : 0; }            // format code of a mode-typed tensor (0 = fp32)
inline int fmt_xn(const Ctx& c) { return x2_rows(c) ? 4 : fmt16(c); }  // ... of the pre-normed rows a projection reads (4 = pre-split)
inline int fmt_mlp(const Ctx& c) { return mlp_x2(c) ? 4 : mlp16(c) ? c.h16 : 0; }  // ... of the expert-MLP / FFN input rows

// a tensor that is fp32 in the fp32-grade mode and bf16 in the throughput mode, living in a float-sized buffer
struct Act {
  void* p;
  bool bf;
  bool x2 = false;  // pre-split rows (MDM_OP_X2_ROW) in an fp32-sized buffer
};
inline Act act_of(const Ctx& c, float* buf) { return Act{buf, c.bf}; }
inline Act act_x2(const Ctx& c, float* buf) { return Act{buf, c.bf, x2_rows(c)}; }  // a tensor its producer wrote in the mode's GEMM-input form
inline Act act_f32(const float* buf) { return Act{(void*)buf, false}; }
inline Act act_bf16(const uint16_t* buf) { return Act{(void*)buf, true}; }

struct LinOpts {
  int act = ACT_NONE;
  float alpha = 1.f, out_scale = 1.f, r1_scale = 1.f;
  const float* R1 = nullptr;
  const float* R2 = nullptr;
  const float* colscale = nullptr;
  int r1_mod = 0;
  uint16_t* outx2 = nullptr;  // fp32-grade kernel: the result as pre-split rows (MdmGemmDesc.Cx2)
};

// out32 / out16 = epilogue(A @ W^T) for a plain [M,K]x[N,K] Linear; either output may be null
int linear(const Ctx& c, Act A, int64_t M, int K, const MdmPacked& W, const float* bias, int N, float* out32,
           uint16_t* out16, const LinOpts& o = LinOpts()) {
  GemmArgs g = gd(c);
  if (A.bf) {
    g.A.p = A.p, g.A.ld = K, g.A.kind = OP_BF16_ROW;
    g.precision = 1;  // 16-bit activations: one pass of the format c.h16 (the weight was packed in it)
  } else {
    g.A = op_f32((const float*)A.p, K);
    if (A.x2) g.A.kind = OP_X2_ROW;
  }
  g.W = packed(W);
  g.w_stream = A.bf ? W.ws : nullptr;  // 16-bit rows and a fragment stream of W: the streamed-weight kernel where it is eligible (csrc/gemm_stream.hip)
  g.M = (int)M, g.N = N, g.K = K;
  g.C = out32, g.C16 = out16, g.ldc = N;
  g.Cx2 = o.outx2;
  g.bias = bias;
  g.act = o.act, g.alpha = o.alpha, g.out_scale = o.out_scale;
  g.R1 = o.R1, g.ldr1 = N, g.r1_scale = o.r1_scale, g.r1_mod = o.r1_mod;
  g.R2 = o.R2, g.ldr2 = N;
  g.colscale = o.colscale;
  if (A.bf && !gemm_bf16_eligible(g)) return MDM_ERR_UNSUPPORTED;
  return gemm(g, c.s);
}
// result typed like the mode: fp32 buffer in the fp32-grade mode, bf16 in the throughput mode
int linear_to_act(const Ctx& c, Act A, int64_t M, int K, const MdmPacked& W, const float* bias, int N, float* buf,
                  const LinOpts& o = LinOpts()) {
  return linear(c, A, M, K, W, bias, N, c.bf ? nullptr : buf, c.bf ? (uint16_t*)buf : nullptr, o);
}

// one contraction per (sample b, head h) of the generic attention chains: A and W are read at b * bs1 + h * bs2 (heads()),
// C is written at b * c_bs1 + h * c_bs2
inline Operand heads(Operand o, int64_t bs1, int64_t bs2) { o.bs1 = bs1, o.bs2 = bs2; return o; }
GemmArgs per_head(const Ctx& c, Operand A, Operand W, int M, int N, int K, int64_t ldc, int64_t c_bs1, int64_t c_bs2) {
  GemmArgs g = gd(c);
  g.A = A, g.W = W;
  g.M = M, g.N = N, g.K = K;
  g.batch = c.B * c.m->H, g.nb2 = c.m->H;
  g.ldc = ldc, g.c_bs1 = c_bs1, g.c_bs2 = c_bs2;
  return g;
}

// the input of an fp32-grade attention core: A W^T + bias (K = D) as bf16 hi | lo planes of [M, N] each; the caller adds the
// epilogue (ACT_HEADNORM, ACT_HEADSOFTMAX, alpha)
GemmArgs planes_gemm(const Ctx& c, Act A, const MdmPacked& W, const float* bias, int N, uint16_t* hi, uint16_t* lo) {
  const int K = c.m->D;
  GemmArgs g = gd(c);
  g.A = op_f32((const float*)A.p, K);
  if (A.x2) g.A.kind = OP_X2_ROW;
  g.W = packed(W);
  g.M = (int)c.M, g.N = N, g.K = K;
  g.bias = bias;
  g.C16 = hi, g.C16_lo = lo, g.ldc = N;
  return g;
}

// Stylization: one launch (csrc/style_gemm.hip) / the same on bf16x3 products, with the caller's tail when it asks for one
// (MDM_VAR_X3_TAILS_SPLIT: without) / style_in and the Linear as two launches (MDM_VAR_X3_STYLE_SPLIT in the fp32-grade modes)
enum class StylePath { FUSED16, FUSED3, FUSED3_TAIL, SPLIT };
StylePath style_path(const Ctx& c, const MdmStyle& st, bool src16, bool out16, bool tail) {
  const int D = c.m->D;
  if (c.bf && st.out_ws && style_gemm_supported(D, c.M)) return StylePath::FUSED16;
  if (x3_flow(c) && !src16 && !out16 && st.out_ws3 && g_variant != MDM_VAR_X3_STYLE_SPLIT && style_gemm_supported(D, c.M))
    return tail && g_variant != MDM_VAR_X3_TAILS_SPLIT ? StylePath::FUSED3_TAIL : StylePath::FUSED3;
  return StylePath::SPLIT;
}

// out = resid + out_scale * colscale * Lin(SiLU(LN(a)(1+scale)+shift)) with a = [post-processed] src
// t3: fp32-grade modes only -- what the fused launch does with the finished rows (csrc/gemm.h StyleTail3) where style_path()
// says FUSED3_TAIL (elsewhere the caller runs those LayerNorms itself)
int style_apply(const Ctx& c, const MdmStyle& st, const float* src, const float* pw, const float* pb, const int* pos4,
                const float* sc, float* tmp, const float* resid, float out_scale, const float* colscale, float* out,
                uint16_t* out16 = nullptr, bool src_bf16 = false, const StyleTail3* t3 = nullptr, const StyleRoute* route = nullptr,
                const StyleText* text = nullptr) {
  const int D = c.m->D;
  const StylePath path = style_path(c, st, src_bf16, out16 != nullptr, t3 != nullptr);
  if ((route || text) && path != StylePath::FUSED16) return MDM_ERR_UNSUPPORTED;  // (route_path() / text_path() ask for them on the one-launch form only)
  switch (path) {
    case StylePath::FUSED16:
      return style_gemm(src, src_bf16 ? c.h16 : 0, c.M, D, c.S, pw, pb, st.norm_w, st.norm_b, sc, pos4, st.out_ws, st.out_b, resid,
                        out_scale, colscale, out, out16, c.h16, c.s, route, text);
    case StylePath::FUSED3:
    case StylePath::FUSED3_TAIL:
      return style_gemm3(src, c.M, D, c.S, pw, pb, st.norm_w, st.norm_b, sc, pos4, st.out_ws3, st.out_b, resid, out_scale, colscale, out,
                         path == StylePath::FUSED3_TAIL ? *t3 : StyleTail3(), c.s);
    case StylePath::SPLIT: {
      MDM_TRY(style_in(src, c.M, D, c.S, pw, pb, st.norm_w, st.norm_b, sc, pos4, src_bf16 ? c.h16 : 0, tmp, fmt16(c), c.s));
      LinOpts o;
      o.out_scale = out_scale, o.R1 = resid, o.colscale = colscale;
      return linear(c, act_of(c, tmp), c.M, D, st.out, st.out_b, D, out, out16, o);
    }
  }
}

// the proj_out pair (fast_attention.py:121-126) as one launch of the streamed-weight kernel, in place on t4
MdmMlpDesc proj_pair_desc(const Ctx& c, const MdmPerformer& p) {
  const int D = c.m->D;
  MdmMlpDesc f = {};
  f.X = (const uint16_t*)c.w.t4, f.ldx = D, f.M = (int)c.M, f.Din = D, f.F = D, f.Dout = D;
  f.b1 = p.proj0_b, f.b2 = p.proj3_b, f.wstream = p.proj_ws, f.wstream_gs = 2 * (int64_t)D * D;
  f.r1_scale = 1.f, f.C16 = (uint16_t*)c.w.t4, f.ldc = D, f.h16 = c.h16;  // in place: a tile's rows are in LDS before its stores
  return f;
}
// Performer proj_out: pair + the Performer's tail in one launch, the pair's rows never leave the CU (MDM_VAR_TAIL_SPLIT: not) /
// the pair in one launch, hidden layer on chip (csrc/mlp_stream.hip) / the two Linears on pre-split rows / the two Linears
enum class ProjPath { PAIR_TAIL, PAIR, LINEARS_X2, LINEARS };
ProjPath proj_path(const Ctx& c, const MdmPerformer& p) {
  if (c.bf && p.proj_ws) {
    const MdmMlpDesc f = proj_pair_desc(c, p);
    if (p.style.out_ws && g_variant != MDM_VAR_TAIL_SPLIT && fused_pair_style_supported(f)) return ProjPath::PAIR_TAIL;
    if (fused_mlp_stream_supported(f)) return ProjPath::PAIR;
  }
  return x2_rows(c) ? ProjPath::LINEARS_X2 : ProjPath::LINEARS;
}

// Performer attention core with its q | k | v projection.  CORE3 (fp32-grade, head_dim 128): the projection's epilogue applies
// LN(dh) / L2 into bf16 hi | lo planes, ONE launch (csrc/perf_attn3.hip) does the rest on bf16x3 products (MDM_VAR_X3_ATTN_CHAIN:
// CHAIN).  CORE256 (16-bit, head_dim 256): the core in two launches.  CORE16_QKV (16-bit, head_dim 128): the projection inside
// the core's launch, k and v never leave the CU (MDM_VAR_QKV_SPLIT: CORE16).  CORE16: LN/L2 -> feature maps -> KV state ->
// num/den -> LN in ONE kernel per (batch, head).  CHAIN: five launches (MDM_VAR_GENERIC_DH256 at head_dim 256).
enum class PerfCore { CORE3, CORE256, CORE16_QKV, CORE16, CHAIN };
// weight warming (csrc/warm.h) is on unless the knob says otherwise: MDM_VAR_NO_WARM leaves every Warm empty
inline bool warm_on() { return g_variant != MDM_VAR_NO_WARM; }
PerfCore perf_core_path(const Ctx& c, const MdmPerformer& p, bool xn16) {
  const int D = c.m->D, H = c.m->H, dh = D / H;
  if (c.bf && g_variant != MDM_VAR_GENERIC_DH256 && perf_attn256_supported(dh, c.S) &&
      perf_attn256_scratch_bytes(c.B, H, c.S) <= c.M * 2 * D * (int64_t)sizeof(float))
    return PerfCore::CORE256;
  if (c.bf && perf_attn_supported(dh, c.S))
    return xn16 && g_variant != MDM_VAR_QKV_SPLIT && perf_attn_qkv_supported(dh, c.S, H) ? PerfCore::CORE16_QKV : PerfCore::CORE16;
  if (x3_flow(c) && !xn16 && g_variant != MDM_VAR_X3_ATTN_CHAIN && perf_attn3_supported(dh, c.S) && D % 32 == 0 && p.qkv.lo &&
      p.feat.lo && (c.M * 3 * D) % 8 == 0)
    return PerfCore::CORE3;
  return PerfCore::CHAIN;
}

// PerformerSelfAttention (fast_attention.py:137-179): xn = pre_norm(x) already computed; out = x + 0.1*style(...)
// pt: the caller's LayerNorms / block tail behind it (csrc/gemm.h StyleTail3) where proj_path() / style_path() say they run; the
// 16-bit modes' pair_tail (csrc/mlp_stream.hip) writes ln_out as 16-bit rows
// rider / rode: independent work offered to the idle CUs of the pair + tail launch, and whether it was taken (csrc/gemm.h)
int performer(const Ctx& c, const MdmPerformer& p, const float* x, Act xn, const float* sc, float* out,
              const StyleTail3& pt = StyleTail3(), const SkipRider* rider = nullptr, bool* rode = nullptr) {
  if (rode) *rode = false;
  const MdmModel& m = *c.m;
  const int D = m.D, H = m.H, dh = D / H, mf = dh;  // m = min(dh, 256) = dh for dh <= 256
  const Work& w = c.w;
  LinOpts qo;  // q|k|v = 0.1 * (xn W^T + b)                     (:145-157); 16-bit when a fused attention core reads it
  qo.alpha = 0.1f;
  Act att = act_of(c, w.t4);  // the attention rows as the core leaves them in t4
  switch (perf_core_path(c, p, xn.bf)) {
    case PerfCore::CORE3: {
      uint16_t* const xh = (uint16_t*)w.qkv;
      uint16_t* const xl = xh + c.M * 3 * D;  // the two 16-bit planes fill the fp32 [M, 3 D] buffer exactly
      GemmArgs g = planes_gemm(c, xn, p.qkv, p.qkv_b, 3 * D, xh, xl);
      g.alpha = 0.1f, g.act = ACT_HEADNORM, g.hn_w = p.hn_w, g.hn_b = p.hn_b, g.hn_l2_tiles = 2 * H;
      MDM_TRY(gemm(g, c.s));
      MDM_TRY(perf_attn3(xh, xl, p.feat.hi, p.feat.lo, (int)p.feat.ld, p.hn_w, p.hn_b, c.len, c.B, c.S, H, dh, w.t4, c.x2 ? 1 : 0, c.s));
      att.x2 = c.x2;  // the attention rows (t4) and the projection's hidden rows (t2) travel pre-split
      break;
    }
    case PerfCore::CORE256:  // feature maps (P^T resident), then KV state + num + LN per (batch, head); qphi / kphi^T / den
                             // pass through w.phi (L2 / MALL resident)
      MDM_TRY(linear(c, xn, c.M, D, p.qkv, p.qkv_b, 3 * D, nullptr, (uint16_t*)w.qkv, qo));
      MDM_TRY(perf_attn256(w.qkv, c.h16, p.feat.hi, (int)p.feat.ld, p.hn_w, p.hn_b, c.len, c.B, c.S, H, (uint16_t*)w.t4, w.phi, c.s));
      break;
    case PerfCore::CORE16_QKV: {
      // the core warms what the pair + tail launch behind it reads first (csrc/warm.h): the pair's stream, the stream of
      // out_layers.2, the plane its riders read, then the biases on its dependent chain
      Warm wm = {};
      if (warm_on() && proj_path(c, p) == ProjPath::PAIR_TAIL) {
        warm_add(wm, p.proj_ws, 2 * (int64_t)D * D * 2);
        warm_add(wm, p.style.out_ws, (int64_t)D * D * 2);
        if (rider) warm_add(wm, rider->W, (int64_t)D * rider->ldw * 2);
        warm_add(wm, p.proj0_b, D * 4), warm_add(wm, p.proj3_b, D * 4), warm_add(wm, p.style.out_b, D * 4);
      }
      MDM_TRY(perf_attn_qkv((const uint16_t*)xn.p, p.qkv.hi, (int)p.qkv.ld, p.qkv_b, 0.1f, (uint16_t*)w.qkv, c.h16, p.feat.hi,
                            (int)p.feat.ld, p.hn_w, p.hn_b, c.len, c.B, c.S, H, dh, (uint16_t*)w.t4, c.s, &wm));
      break;
    }
    case PerfCore::CORE16:  // (:44-90)
      MDM_TRY(linear(c, xn, c.M, D, p.qkv, p.qkv_b, 3 * D, nullptr, (uint16_t*)w.qkv, qo));
      MDM_TRY(perf_attn(w.qkv, c.h16, p.feat.hi, (int)p.feat.ld, p.hn_w, p.hn_b, c.len, c.B, c.S, H, dh, (uint16_t*)w.t4, c.s));
      break;
    case PerfCore::CHAIN: {
      MDM_TRY(linear(c, xn, c.M, D, p.qkv, p.qkv_b, 3 * D, w.qkv, nullptr, qo));
      // shared LN over head_dim, L2 normalise q,k                     (:44-55)
      MDM_TRY(head_norm(w.qkv, c.M, H, dh, p.hn_w, p.hn_b, c.s));
      // feature maps 0.1*exp(clamp(z P)), keys masked past length     (:58-74): rows = (token, slot<2H)
      // a model packed for the fp16 modes holds P as ONE fp16 plane, which only the 16-bit-activation kernels read: the chain
      // works on fp32 rows, so it re-splits that plane into bf16 hi | lo (exact; kvt is free until the KV GEMM) and runs its
      // GEMMs as bf16x3 -- a single bf16 pass on these rows would be coarser than the fp16 mode it serves
      const bool f16p = c.bf && c.h16 == MDM_H16_F16 && !p.feat.lo;
      Operand P = packed(p.feat);
      if (f16p) {
        const int64_t pn = (int64_t)mf * p.feat.ld;
        // cannot bind for a model the packer makes: an fp16 P exists at head_dim 128 / 256 only, where ld = dh (a multiple of 32)
        // and mf = dh, so pn = dh * dh <= B * H * dh * dh
        if (pn > (int64_t)c.B * H * dh * dh) return MDM_ERR_UNSUPPORTED;
        uint16_t* const ph = (uint16_t*)w.kvt;
        MDM_TRY(f16_to_bf16x2(p.feat.hi, pn, ph, ph + pn, c.s));
        P = op_bf16(ph, ph + pn, p.feat.ld);
      }
      const int cprec = f16p ? 3 : c.prec;
      GemmArgs g = gd(c);
      g.precision = cprec;
      g.A = op_f32(w.qkv, dh);
      g.A.rpg = 2 * H, g.A.gstride = 3 * D;
      g.W = P;
      g.M = (int)(c.M * 2 * H), g.N = mf, g.K = dh;
      g.C = w.phi, g.ldc = mf;
      g.act = ACT_FEAT;
      g.feat_len = c.len, g.feat_S = c.S, g.feat_rpt = 2 * H, g.feat_kslot = H;
      MDM_TRY(gemm(g, c.s));
      // KV^T[b,h] (dh x m) = 0.1 * sum_t v[t] (x) kphi[t]              (:77)
      GemmArgs kv = per_head(c, heads(op_f32_kstride(w.qkv + 2 * D, 3 * D), (int64_t)c.S * 3 * D, dh),
                             heads(op_f32_kstride(w.phi + H * mf, 2 * H * mf), (int64_t)c.S * 2 * H * mf, mf), dh, mf, c.S, mf,
                             (int64_t)H * dh * mf, (int64_t)dh * mf);
      kv.C = w.kvt, kv.out_scale = 0.1f, kv.precision = cprec;
      MDM_TRY(gemm(kv, c.s));
      // num = 0.1 * qphi KV                                            (:78) -> t2 (M, D) merged heads
      GemmArgs num = per_head(c, heads(op_f32(w.phi, 2 * H * mf), (int64_t)c.S * 2 * H * mf, mf),
                              heads(op_f32(w.kvt, mf), (int64_t)H * dh * mf, (int64_t)dh * mf), c.S, dh, mf, D, (int64_t)c.S * D, dh);
      num.C = w.t2, num.out_scale = 0.1f, num.precision = cprec;
      MDM_TRY(gemm(num, c.s));
      // same-t denominator, divide, LN over head_dim                   (:81-90) -> t4
      MDM_TRY(den_ln(w.t2, w.phi, c.M, H, dh, p.hn_w, p.hn_b, w.t4, fmt16(c), c.s));
      break;
    }
  }
  // proj_out: Linear -> GELU -> Linear                             (:121-126,165); its output feeds a LayerNorm only: 16 bits in
  // the 16-bit modes
  switch (proj_path(c, p)) {
    case ProjPath::PAIR_TAIL: {
      PairTail t = {};
      t.pw = p.post_w, t.pb = p.post_b, t.sw = p.style.norm_w, t.sb = p.style.norm_b, t.sc = sc, t.S = c.S;
      t.ws = p.style.out_ws, t.bias = p.style.out_b, t.resid = x, t.out_scale = 0.1f, t.out = out;
      t.lw = pt.lw, t.lb = pt.lb, t.ln16 = (uint16_t*)pt.ln_out, t.skip = pt.skip, t.skip_scale = pt.skip_scale, t.l2w = pt.l2w, t.l2b = pt.l2b;
      t.rider = rider;
      return fused_pair_style(proj_pair_desc(c, p), t, c.s, rode);
    }
    case ProjPath::PAIR:
      MDM_TRY(fused_mlp_stream(proj_pair_desc(c, p), c.s));
      break;
    case ProjPath::LINEARS_X2: {
      LinOpts o;
      o.act = ACT_GELU, o.outx2 = (uint16_t*)w.t2;
      MDM_TRY(linear(c, att, c.M, D, p.proj0, p.proj0_b, D, nullptr, nullptr, o));
      MDM_TRY(linear(c, Act{w.t2, false, true}, c.M, D, p.proj3, p.proj3_b, D, w.t4, nullptr));
      break;
    }
    case ProjPath::LINEARS: {
      LinOpts o;
      o.act = ACT_GELU;
      MDM_TRY(linear_to_act(c, att, c.M, D, p.proj0, p.proj0_b, D, w.t2, o));
      MDM_TRY(linear_to_act(c, act_of(c, w.t2), c.M, D, p.proj3, p.proj3_b, D, w.t4));
      break;
    }
  }
  // post_norm, normalize * sqrt(D), stylization, y = x + 0.1 * style (:169-178); fp32-grade modes: the caller's LayerNorms / block
  // tail behind it in the same launch when it asks for them (pt.ln_out / pt.skip)
  const bool tail3 = !c.bf && (pt.ln_out || pt.skip);
  return style_apply(c, p.style, w.t4, p.post_w, p.post_b, nullptr, sc, w.t2, x, 0.1f, nullptr, out, nullptr, c.bf,
                     tail3 ? &pt : nullptr);
}

// DualSelfAttentionBlock's tail inside its Performers' launches: T16 where both Performers end in the pair + tail launch
// (16-bit modes, D = 512), T3 where both stylizations take a tail (fp32-grade modes: style_gemm3); NONE: its own launches
enum class DualTail { NONE, T16, T3 };
DualTail dual_tail_path(const Ctx& c, const MdmLayer& l) {
  if (proj_path(c, l.local) == ProjPath::PAIR_TAIL && proj_path(c, l.global) == ProjPath::PAIR_TAIL) return DualTail::T16;
  if (style_path(c, l.local.style, false, false, true) == StylePath::FUSED3_TAIL &&
      style_path(c, l.global.style, false, false, true) == StylePath::FUSED3_TAIL)
    return DualTail::T3;
  return DualTail::NONE;
}

// DualSelfAttentionBlock (fast_attention.py:208-226): x -> out.  Uses t1..t5.  x16: bf16 shadow of x (throughput mode)
// next_w / next_b: optional LayerNorm of the FOLLOWING block (cross_attn.base_ca.norm) chained onto post_norm; its output
// goes to t2 typed like the mode, and cross_block(pre_normed = true) picks it up (one launch less per layer)
int dual_block(const Ctx& c, const MdmLayer& l, const float* x, const uint16_t* x16, const float* sc4, float* out,
               const float* next_w = nullptr, const float* next_b = nullptr) {
  const int D = c.m->D;
  const Work& w = c.w;
  const int64_t scs = (int64_t)c.B * 2 * D;
  const int xnf = fmt_xn(c);  // format of the pre-normed rows the q | k | v projections read
  const Act xa = c.bf ? act_bf16(x16) : act_f32(x);
  LinOpts so;  // skip = GELU(Lin(x))                                (:219-225)
  so.act = ACT_GELU;
  const DualTail path = dual_tail_path(c, l);
  switch (path) {
    case DualTail::T16:
    case DualTail::T3: {
      // skip is computed into the FFN's hidden buffer (free during this block), and the second Performer's launch ends
      // with out = post_norm(skip + 0.1 * global_out) and the next block's pre-norm -- no D x D GEMM waiting behind the
      // attention chain, no LayerNorm launch behind that.  T16: nothing but that tail reads skip and nothing in the block
      // writes x16, so the first Performer's pair + tail launch is offered the projection for its idle CUs (riders,
      // csrc/mlp_stream.hip; MDM_VAR_SKIP_LAUNCH: not); where it declines, or on T3, skip is a launch of its own
      const bool offer = path == DualTail::T16 && g_variant != MDM_VAR_SKIP_LAUNCH;
      const SkipRider sr = {x16, D, l.skip.hi, l.skip.ld, l.skip_b, w.f1, D, (int)c.M};
      bool rode = false;
      if (!offer) MDM_TRY(linear(c, xa, c.M, D, l.skip, l.skip_b, D, w.f1, nullptr, so));
      // h = pre_norm(x) -> t1 ; local.pre_norm(h) -> t3
      MDM_TRY(ln_chain(x, c.M, D, l.dual_pre_w, l.dual_pre_b, w.t1, 0, l.local.pre_w, l.local.pre_b, w.t3, xnf, c.s));
      StyleTail3 pt;  // local_out -> t5, global.pre_norm(local_out) -> t3 (t3 is dead by then)
      pt.lw = l.global.pre_w, pt.lb = l.global.pre_b, pt.ln_out = w.t3, pt.ln_x2 = c.x2;
      MDM_TRY(performer(c, l.local, w.t1, act_x2(c, w.t3), sc4 + 0 * scs, w.t5, pt, offer ? &sr : nullptr, &rode));
      if (offer && !rode) MDM_TRY(linear(c, xa, c.M, D, l.skip, l.skip_b, D, w.f1, nullptr, so));
      StyleTail3 bt;
      bt.skip = w.f1, bt.skip_scale = 0.1f, bt.lw = l.dual_post_w, bt.lb = l.dual_post_b;
      if (next_w) bt.l2w = next_w, bt.l2b = next_b, bt.ln_out = w.t2, bt.ln_x2 = c.x2;
      return performer(c, l.global, w.t5, act_x2(c, w.t3), sc4 + 1 * scs, out, bt);
    }
    case DualTail::NONE: {
      MDM_TRY(ln_chain(x, c.M, D, l.dual_pre_w, l.dual_pre_b, w.t1, 0, l.local.pre_w, l.local.pre_b, w.t3, xnf, c.s));
      // local_out -> t5; a local Performer that ends in the pair + tail launch also leaves global.pre_norm(local_out) in t3
      const bool normed = proj_path(c, l.local) == ProjPath::PAIR_TAIL;
      StyleTail3 pt;
      if (normed) pt.lw = l.global.pre_w, pt.lb = l.global.pre_b, pt.ln_out = w.t3;
      MDM_TRY(performer(c, l.local, w.t1, act_x2(c, w.t3), sc4 + 0 * scs, w.t5, pt));
      if (!normed) MDM_TRY(ln_chain(w.t5, c.M, D, l.global.pre_w, l.global.pre_b, w.t3, xnf, nullptr, nullptr, nullptr, 0, c.s));
      MDM_TRY(performer(c, l.global, w.t5, act_x2(c, w.t3), sc4 + 1 * scs, w.t1));  // global_out -> t1
      // out = post_norm(skip + 0.1 * global); fp32 on purpose: this sum is the block's output before its final LayerNorm
      // (storing it as bf16 measured +60 % block error for 0.01 ms per step)
      so.R1 = w.t1, so.r1_scale = 0.1f;
      MDM_TRY(linear(c, xa, c.M, D, l.skip, l.skip_b, D, w.t3, nullptr, so));
      return ln_chain(w.t3, c.M, D, l.dual_post_w, l.dual_post_b, out, 0, next_w, next_b, next_w ? w.t2 : nullptr, xnf, c.s);
    }
  }
}

// Linear cross-attention.  CORE3 (fp32-grade, head_dim 128): the head_dim softmax is the query projection's epilogue (bf16 hi |
// lo planes), the product with A[b, h] one launch on bf16x3 MFMAs (MDM_VAR_X3_XATTN_CHAIN: CHAIN).  CORE_Q (16-bit, head_dim
// 128): the query projection inside the core's launch (MDM_VAR_XQ_SPLIT: CORE).  CORE: projection, 16-bit core
// (MDM_VAR_GENERIC_DH256 at head_dim 256: CHAIN).  CHAIN: GEMM, head_softmax, batched contraction.
enum class XattnPath { CORE3, CORE_Q, CORE, CHAIN };
XattnPath lin_xattn_path(const Ctx& c, const MdmLayer& l) {
  const int D = c.m->D, H = c.m->H, dh = D / H;
  if (c.bf && lin_xattn_supported(dh) && !(dh == 256 && g_variant == MDM_VAR_GENERIC_DH256))
    return g_variant != MDM_VAR_XQ_SPLIT && D == 512 && lin_xattn_q_supported(dh, c.S, H) ? XattnPath::CORE_Q : XattnPath::CORE;
  if (x3_flow(c) && g_variant != MDM_VAR_X3_XATTN_CHAIN && xattn3_supported(dh, 1) && l.ca_q.lo && D % 32 == 0 && (c.M * D) % 8 == 0)
    return XattnPath::CORE3;
  return XattnPath::CHAIN;
}

// MoE router.  FOLDED (16-bit modes at D = 512, E = 8 / 16, hn rows in the mode's 16-bit format, inside decoder_layer): the gate
// runs in the epilogue of the cross-attention stylization launch in front of the MoE block, on the rows that launch has just
// finished, and the assign launch makes the slab offsets itself -- one router launch per layer instead of three, bit-identical
// routing (MDM_VAR_ROUTE_LAUNCH: LAUNCH).  LAUNCH: gate, offsets and assign as three launches (moe_route); also whenever the
// stylization grid would not fit the partial-counter buffers, and for a MoE block that runs alone.  The variants that pick the
// gate KERNEL (MDM_VAR_ROUTER_CONST_E / _RUNTIME_E) keep the launch they are about.
enum class RoutePath { FOLDED, LAUNCH };
RoutePath route_path(const Ctx& c, const MdmLayer& l) {
  if (g_variant == MDM_VAR_ROUTE_LAUNCH || g_variant == MDM_VAR_ROUTER_CONST_E || g_variant == MDM_VAR_ROUTER_RUNTIME_E) return RoutePath::LAUNCH;
  if (c.bf && !c.fp8 && style_path(c, l.ca_style, true, false, false) == StylePath::FUSED16 &&
      style_gemm_route_supported(c.m->D, c.M, c.m->E, fmt_mlp(c), c.h16))
    return RoutePath::FOLDED;
  return RoutePath::LAUNCH;
}
// the router's operands of one layer (forced: optional injected routing)
MoeGateParams gate_params(const Ctx& c, const MdmLayer& l, const int* forced) {
  const Work& w = c.w;
  MoeGateParams p = {};
  for (int b = 0; b < 2; ++b) {
    p.ln_w[b] = l.moe_ln_w[b], p.ln_b[b] = l.moe_ln_b[b];
    p.gate_w[b] = l.gate_w[b], p.gate_b[b] = l.gate_b[b];
    p.usage[b] = l.usage[b], p.importance[b] = l.importance[b];
  }
  p.hn = w.hn, p.hn_bf16 = c.fp8 ? 3 : fmt_mlp(c), p.hn_scale = w.hn_scale, p.top_idx = w.top_idx, p.top_val = w.top_val, p.hist = w.hist, p.uimp = w.uimp, p.forced_idx = forced;
  return p;
}

// GatedCrossAttention (fast_attention.py:242-272): out = x + sigmoid(gate)*sigmoid(adaptive)*style(softmax(q) A)
// route: the stylization launch also routes `out` for the MoE block that follows (RoutePath::FOLDED)
int cross_block(const Ctx& c, const MdmLayer& l, const float* at, const float* x, const float* sc, float* out,
                bool pre_normed = false, const StyleRoute* route = nullptr) {
  const MdmModel& m = *c.m;
  const int D = m.D, H = m.H, dh = D / H;
  const Work& w = c.w;
  if (!pre_normed) MDM_TRY(ln_chain(x, c.M, D, l.ca_norm_w, l.ca_norm_b, w.t2, fmt_xn(c), nullptr, nullptr, nullptr, 0, c.s));
  bool y16 = false;  // the core's output (t4) is 16-bit: it is consumed by the stylization LayerNorm only
  switch (lin_xattn_path(c, l)) {
    case XattnPath::CORE3: {
      uint16_t* const qh = (uint16_t*)w.t3;
      uint16_t* const ql = qh + c.M * D;  // the two planes fill the fp32 [M, D] buffer exactly
      GemmArgs g = planes_gemm(c, act_x2(c, w.t2), l.ca_q, l.ca_q_b, D, qh, ql);
      g.act = ACT_HEADSOFTMAX;
      MDM_TRY(gemm(g, c.s));
      MDM_TRY(lin_xattn3(qh, ql, at, c.B, c.S, H, dh, w.t4, c.s));
      break;
    }
    case XattnPath::CORE_Q:
      MDM_TRY(lin_xattn_q((const uint16_t*)w.t2, l.ca_q.hi, (int)l.ca_q.ld, l.ca_q_b, at, c.B, c.S, H, dh, nullptr, (uint16_t*)w.t4,
                          c.h16, c.s));
      y16 = true;
      break;
    case XattnPath::CORE:
      MDM_TRY(linear(c, act_x2(c, w.t2), c.M, D, l.ca_q, l.ca_q_b, D, nullptr, (uint16_t*)w.t3));
      MDM_TRY(lin_xattn(w.t3, c.h16, at, c.B, c.S, H, dh, nullptr, (uint16_t*)w.t4, c.h16, c.s));  // (:248,253)
      y16 = true;
      break;
    case XattnPath::CHAIN: {
      MDM_TRY(linear(c, act_x2(c, w.t2), c.M, D, l.ca_q, l.ca_q_b, D, w.t3, nullptr));
      MDM_TRY(head_softmax(w.t3, c.M * H, dh, c.s));  // softmax over head_dim (:248)
      // y[b,s,h,:] = q[b,s,h,:] A[b,h]  (:253), W = A^T rows
      GemmArgs g = per_head(c, heads(op_f32(w.t3, D), (int64_t)c.S * D, dh), heads(op_f32(at, dh), (int64_t)H * dh * dh, (int64_t)dh * dh),
                            c.S, dh, dh, D, (int64_t)c.S * D, dh);
      g.C = w.t4;
      MDM_TRY(gemm(g, c.s));
      break;
    }
  }
  return style_apply(c, l.ca_style, w.t4, nullptr, nullptr, nullptr, sc, w.t2, x, 1.f, l.ca_gvec, out, nullptr, y16, nullptr, route);
}

// one grouped expert GEMM: rows of A [., K] in the mode's expert-operand form (e4m3, 16-bit, pre-split or fp32 rows) times
// W_e^T + b_e, per expert's rows (w.goff); the caller adds the rest of the epilogue and the output
GemmArgs expert_gemm(const Ctx& c, const void* A, int K, const MdmPacked& W, const float* bias, int N) {
  GemmArgs g = gd(c);
  if (c.fp8) {  // W's channel scales live in its lo plane (packing)
    g.A.p = A, g.A.ld = K, g.A.kind = MDM_OP_FP8_ROW;
    g.W.p = W.hi, g.W.ld = W.ld, g.W.kind = MDM_OP_FP8_ROW, g.w_scale = (const float*)W.lo;
  } else if (mlp16(c)) {
    g.A.p = A, g.A.ld = K, g.A.kind = OP_BF16_ROW, g.precision = 1;
    g.W = packed(W);
  } else {
    g.A = op_f32((const float*)A, K);
    if (mlp_x2(c)) g.A.kind = OP_X2_ROW;
    g.W = packed(W);
  }
  g.W.bs1 = (int64_t)N * W.ld;
  g.goff = c.w.goff, g.ngroups = 2 * c.m->E;
  g.M = (int)(4 * c.M), g.N = N, g.K = K;
  g.bias = bias, g.bias_bs = N;
  g.ldc = N;
  // pre-split rows and a fragment pair stream of W: the streamed-weight bf16x3 kernel (csrc/gemm_stream3.hip)
  if (mlp_x2(c) && W.ws) g.w_stream = W.ws, g.w_stream_gs = gemm_stream3x_group_elems(N, K);
  return g;
}
// MoE experts: e4m3 operands (precision 5) / both expert GEMMs in one launch (f) on 16-bit operands / two grouped GEMMs
enum class MoePath { FP8, FUSED, GROUPED };
MoePath moe_path(const Ctx& c, const MdmMlpDesc& f) {
  if (c.fp8) return MoePath::FP8;
  return mlp16(c) && fused_mlp_supported(f) ? MoePath::FUSED : MoePath::GROUPED;
}

// the expert MLP of one layer as one launch of the fused kernel: routed hn rows -> W1_e, GELU, W2_e -> y2
MdmMlpDesc moe_mlp_desc(const Ctx& c, const MdmLayer& l) {
  const int D = c.m->D, F = c.m->F, E = c.m->E;
  const Work& w = c.w;
  MdmMlpDesc f = {};
  f.X = (const uint16_t*)w.hn, f.ldx = D, f.gather = w.perm;
  f.M = (int)(4 * c.M), f.Din = D, f.F = F, f.Dout = D;
  f.goff = w.goff, f.ngroups = 2 * E;
  f.w1 = l.w1.hi, f.ldw1 = l.w1.ld, f.w1_gs = (int64_t)F * l.w1.ld, f.b1 = l.b1, f.b1_gs = F;
  f.w2 = l.w2.hi, f.ldw2 = l.w2.ld, f.w2_gs = (int64_t)D * l.w2.ld, f.b2 = l.b2, f.b2_gs = D;
  f.rowscale = w.rowscale, f.r1_scale = 1.f;
  f.C = w.y2, f.ldc = D;
  f.h16 = c.h16;
  f.wstream = l.wstream, f.wstream_gs = l.wstream_gs;
  return f;
}

// MoEMultiBranchFFN (multi_branch.py:52-61) with SwitchMoELayer top-2 routing (switch_moe.py:44-111)
// rp == FOLDED: the launch that produced x has run the gate already (cross_block with a StyleRoute)
// text: the stylization launch also runs the folded text cross-attention behind the block (TextPath::EPILOGUE); out16 is then
// not written
int moe_block(const Ctx& c, const MdmLayer& l, const float* x, const float* sc, const int* forced, float* out,
              uint16_t* out16, int32_t* route_out = nullptr, RoutePath rp = RoutePath::LAUNCH, const StyleText* text = nullptr) {
  const MdmModel& m = *c.m;
  const int D = m.D, F = m.F, E = m.E;
  const Work& w = c.w;
  const MoeGateParams p = gate_params(c, l, forced);
  switch (rp) {
    case RoutePath::FOLDED:
      MDM_TRY(moe_route_folded(c.M, E, p, (int)style_gemm_route_parts(c.M), w.goff, w.cursor, w.perm, w.rowscale, w.pos4, c.s));
      break;
    case RoutePath::LAUNCH: MDM_TRY(moe_route(x, c.M, D, E, p, w.goff, w.cursor, w.perm, w.rowscale, w.pos4, c.s)); break;
  }
  if (route_out && hipMemcpyAsync(route_out, w.top_idx, 4 * c.M * sizeof(int32_t), hipMemcpyDeviceToDevice, c.s) != hipSuccess)
    return MDM_ERR_LAUNCH;
  MdmMlpDesc f = moe_mlp_desc(c, l);
  const MoePath mp = moe_path(c, f);
  if (text && !(mp == MoePath::FUSED && c.bf)) return MDM_ERR_UNSUPPORTED;  // (text_path() asks for it on 16-bit y2 rows only)
  switch (mp) {
    case MoePath::FP8: {
      // fp8 experts (switch_moe.py:19-25,104-109 on e4m3 operands): hidden = e4m3(8 * GELU(dequant(X8 W1_8^T) + b1)), then
      // y2 = prob * (dequant(hidden8 W2_8^T) / 8 + b2).  Row scales come from the router kernel, channel scales from packing.
      const float HS = 8.f;  // static hidden scale: GELU outputs of O(1) land in e4m3's normal range [2^-6, 448]
      GemmArgs g1 = expert_gemm(c, w.hn, D, l.w1, l.b1, F);
      g1.A.gather = w.perm, g1.a_scale = w.hn_scale, g1.act = ACT_GELU, g1.C8 = (uint8_t*)w.hid, g1.c8_scale = HS;
      MDM_TRY(gemm(g1, c.s));
      GemmArgs g2 = expert_gemm(c, w.hid, F, l.w2, l.b2, D);
      g2.a_scale_u = 1.f / HS, g2.rowscale = w.rowscale, g2.C16 = (uint16_t*)w.y2;
      MDM_TRY(gemm(g2, c.s));
      return style_apply(c, l.ffn_style, w.y2, nullptr, nullptr, w.pos4, sc, w.t2, x, 1.f, nullptr, out, out16, true);
    }
    case MoePath::FUSED: {  // hidden activations stay in LDS (switch_moe.py:19-25,104-109)
      if (c.bf) f.C = nullptr, f.C16 = (uint16_t*)w.y2;  // expert outputs stored in 16 bits (what autocast does to a Linear); mixed mode: fp32
      MDM_TRY(probe_begin(c.s));
      MDM_TRY(fused_mlp(f, c.s));
      MDM_TRY(probe_end(c.s, f.M));
      return style_apply(c, l.ffn_style, w.y2, nullptr, nullptr, w.pos4, sc, w.t2, x, 1.f, nullptr, out, text ? nullptr : out16, c.bf,
                         nullptr, nullptr, text);
    }
    case MoePath::GROUPED: {  // bracketed for the measurement probe like the fused kernel
      MDM_TRY(probe_begin(c.s));
      GemmArgs g1 = expert_gemm(c, w.hn, D, l.w1, l.b1, F);  // hidden = GELU(LN_b(x)[routed rows] W1_e^T + b1_e)
      g1.A.gather = w.perm, g1.act = ACT_GELU;
      if (mlp16(c)) g1.C16 = (uint16_t*)w.hid;
      else if (mlp_x2(c)) g1.Cx2 = (uint16_t*)w.hid;
      else g1.C = w.hid;
      MDM_TRY(gemm(g1, c.s));
      GemmArgs g2 = expert_gemm(c, w.hid, F, l.w2, l.b2, D);  // y2[pos] = prob[pos] * (hidden W2_e^T + b2_e)      (switch_moe.py:108-109)
      g2.rowscale = w.rowscale, g2.C = w.y2;  // fp32: the four routed rows of a token are summed in the stylization kernel
      MDM_TRY(gemm(g2, c.s));
      MDM_TRY(probe_end(c.s, (int)(4 * c.M)));
      // mean of the two branches (each the sum of its two routed rows), stylization, residual
      return style_apply(c, l.ffn_style, w.y2, nullptr, nullptr, w.pos4, sc, w.t2, x, 1.f, nullptr, out, out16, false);
    }
  }
}

// Passes the folded text cross-attention (csrc/sdfold.hip) takes, 0 = use the GEMM chain.  Measured end to end (configs[1],
// ms per step, folded / chain): N = 28: 6.09 / 6.28, N = 40: 6.16 / 6.27, N = 64: 6.21 / 6.29 (two passes), N = 85: 6.40 / 6.31
// (four passes: each pass re-streams the x tile and restarts the K' pipeline) -- so the fold is taken up to two passes;
// MDM_VAR_SD_FOLD_ANY forces it at any supported N (tests).
int sd_fold_policy(int D, int H, int N) {
  if (!sd_fold_supported(D, H, N)) return 0;
  const int np = sd_fold_passes(H, N);
  return (np <= 2 || g_variant == MDM_VAR_SD_FOLD_ANY) ? np : 0;
}

// MemoryEfficientCrossAttentionBlock (fast_attention.py:301-330); out must not alias x
struct SdFold {  // folded text side of one layer (MdmTextCache.sd_kfold / sd_cb / sd_vfold), or nulls
  const uint16_t* kfold = nullptr;
  const float* cb = nullptr;
  const uint16_t* vfold = nullptr;
};

// Text cross-attention.  FOLD_PAIR / FOLD (16-bit): query GEMM + attention core + output GEMM + LayerNorm in one launch
// (csrc/sdfold.hip), then the 4x FFN pair in one launch (f) / as two GEMMs.  The pair at the full time scale only: at the half
// scale of the bench batch (6272 rows -> 32-row tiles, every workgroup streams the pair's 4 MB for 32 rows) it measures slower
// than the two GEMMs (78 vs 66 us; 100 vs 120 us at 12544 rows).  The choice is made on the FRAME count of the scale, never on
// the batch: a sample's result must not depend on the batch it travels in (shard invariance, cond | uncond batching).
// CORE3 (fp32-grade, head_dim 128): query as bf16 hi | lo planes, scores / softmax / PV one launch on bf16x3 MFMAs
// (MDM_VAR_X3_XATTN_CHAIN: CHAIN).  CORE (16-bit): scores, softmax, PV in one launch (MDM_VAR_GENERIC_DH256 at head_dim 256:
// CHAIN).  CHAIN: two batched contractions around a row softmax.
enum class SdPath { FOLD_PAIR, FOLD, CORE3, CORE, CHAIN };
bool sd_folded(const Ctx& c, const SdFold& fold) {
  return c.bf && fold.kfold && g_variant != MDM_VAR_SD_UNFOLDED && sd_fold_policy(c.m->D, c.m->H, c.N) > 0;
}
SdPath sd_path(const Ctx& c, const MdmLayer& l, const SdFold& fold, const MdmMlpDesc& f) {
  const int D = c.m->D, H = c.m->H, dh = D / H, N = c.N;
  if (sd_folded(c, fold))
    return l.sd_ffn_ws && c.S >= 128 && fused_mlp_stream_supported(f) ? SdPath::FOLD_PAIR : SdPath::FOLD;
  if (x3_flow(c) && g_variant != MDM_VAR_X3_XATTN_CHAIN && xattn3_supported(dh, N) && l.sd_q.lo && D % 32 == 0 && (c.M * D) % 8 == 0)
    return SdPath::CORE3;
  if (c.bf && xattn_supported(dh, N) && !(dh == 256 && g_variant == MDM_VAR_GENERIC_DH256)) return SdPath::CORE;
  return SdPath::CHAIN;
}

// the 4x FFN (LayerNorm rows in t4 -> Linear -> GELU -> Linear) as two GEMMs: out = x + (o + ffn(o)), o in t3.  16-bit operands
// in the throughput AND the mixed mode; in the fp32-grade mode the hidden rows are written pre-split for the GEMM that reads them
int sd_ffn(const Ctx& c, const MdmLayer& l, const float* x, float* out, uint16_t* out16) {
  const int D = c.m->D;
  const Work& w = c.w;
  const bool h = mlp16(c), x2 = mlp_x2(c);
  LinOpts o1;
  o1.act = ACT_GELU;
  if (x2) o1.outx2 = (uint16_t*)w.f1;
  MDM_TRY(linear(c, Act{w.t4, h, x2}, c.M, D, l.sd_f1, l.sd_f1_b, 4 * D, (h || x2) ? nullptr : w.f1, h ? (uint16_t*)w.f1 : nullptr, o1));
  LinOpts o;
  o.R1 = x, o.R2 = w.t3;
  return linear(c, Act{w.f1, h, x2}, c.M, 4 * D, l.sd_f2, l.sd_f2_b, D, out, out16, o);
}

// Where the folded text cross-attention runs.  EPILOGUE (inside decoder_layer, 16-bit modes, D = 512, the MoE block on the fused
// 16-bit path, sd_path() FOLD_PAIR / FOLD with at most two passes): in the epilogue of the MoE block's stylization launch, on the
// rows that launch has just finished (csrc/style_gemm.hip TX form) -- the sd_fold launch and the 16-bit [M, D] tensor in front of
// it are gone, t3 / t4 come out bit-identical.  LAUNCH: sd_fold as a launch of its own (MDM_VAR_TEXT_LAUNCH); also for a block
// that runs alone.  The choice depends on the mode and the shapes of a SAMPLE (S, N), never on the batch.
enum class TextPath { EPILOGUE, LAUNCH };
TextPath text_path(const Ctx& c, const MdmLayer& l, const SdFold& fold) {
  const int D = c.m->D, H = c.m->H;
  if (g_variant == MDM_VAR_TEXT_LAUNCH || !sd_folded(c, fold) || c.fp8 || sd_fold_passes(H, c.N) > 2) return TextPath::LAUNCH;
  if (moe_path(c, moe_mlp_desc(c, l)) != MoePath::FUSED || style_path(c, l.ffn_style, true, false, false) != StylePath::FUSED16 ||
      c.M != (int64_t)c.B * c.S || !style_gemm_text_supported(D, c.M, c.S, H, c.N))
    return TextPath::LAUNCH;
  return TextPath::EPILOGUE;
}
// the operands of the text epilogue: what sd_fold takes in sdcross_block
StyleText text_operands(const Ctx& c, const MdmLayer& l, const SdFold& fold) {
  StyleText t;
  t.kfold = fold.kfold, t.cb = fold.cb, t.vfold = fold.vfold, t.bout = l.sd_out_b, t.ln_w = l.sd_ln_w, t.ln_b = l.sd_ln_b;
  t.o32 = c.w.t3, t.ln16 = (uint16_t*)c.w.t4;
  t.H = c.m->H, t.N = c.N, t.hpp = sd_fold_heads_per_pass(c.m->H, c.N), t.npass = sd_fold_passes(c.m->H, c.N);
  return t;
}

// tp == EPILOGUE: the launch that produced x has left o (t3) and LN(o) (t4) already (moe_block with a StyleText)
int sdcross_block(const Ctx& c, const MdmLayer& l, const float* kc, const float* vc, const float* x, const uint16_t* x16,
                  float* out, uint16_t* out16, const SdFold& fold = SdFold(), TextPath tp = TextPath::LAUNCH) {
  const MdmModel& m = *c.m;
  const int D = m.D, H = m.H, dh = D / H, N = c.N;
  const Work& w = c.w;
  MdmMlpDesc f = {};  // the FFN pair in one launch of the streamed-weight kernel: out = x + (o + ffn(o)), o in t3, LN(o) in t4
  f.X = (const uint16_t*)w.t4, f.ldx = D, f.M = (int)c.M, f.Din = D, f.F = 4 * D, f.Dout = D;
  f.b1 = l.sd_f1_b, f.b2 = l.sd_f2_b, f.wstream = l.sd_ffn_ws, f.wstream_gs = 8 * (int64_t)D * D;
  f.R1 = x, f.ldr1 = D, f.r1_scale = 1.f, f.R2 = w.t3, f.ldr2 = D;
  f.C = out, f.C16 = out16, f.ldc = D, f.h16 = c.h16;
  const SdPath path = sd_path(c, l, fold, f);
  const Act xa = c.bf ? act_bf16(x16) : act_f32(x);
  LinOpts qo;  // q = (x Wq^T + b) / sqrt(dh)
  qo.alpha = 1.f / sqrtf((float)dh);
  Act att = act_of(c, w.t2);  // the attention rows as the core leaves them in t2
  switch (path) {
    case SdPath::FOLD_PAIR:
    case SdPath::FOLD:
      if (tp == TextPath::LAUNCH)
        MDM_TRY(sd_fold(x16, fold.kfold, fold.cb, fold.vfold, l.sd_out_b, l.sd_ln_w, l.sd_ln_b, c.B, c.S, D, H, N, w.t3,
                        (uint16_t*)w.t4, c.h16, c.s));
      return path == SdPath::FOLD_PAIR ? fused_mlp_stream(f, c.s) : sd_ffn(c, l, x, out, out16);
    case SdPath::CORE3: {
      uint16_t* const qh = (uint16_t*)w.t1;
      uint16_t* const ql = qh + c.M * D;
      GemmArgs g = planes_gemm(c, act_f32(x), l.sd_q, l.sd_q_b, D, qh, ql);
      g.alpha = qo.alpha;
      MDM_TRY(gemm(g, c.s));
      MDM_TRY(sd_attn3(qh, ql, kc, vc, c.ntok, c.B, c.S, H, dh, N, w.t2, c.x2 ? 1 : 0, c.s));
      att.x2 = c.x2;
      break;
    }
    case SdPath::CORE:
      MDM_TRY(linear(c, xa, c.M, D, l.sd_q, l.sd_q_b, D, nullptr, (uint16_t*)w.t1, qo));
      MDM_TRY(sd_attn(w.t1, c.h16, kc, vc, c.B, c.S, H, dh, N, (uint16_t*)w.t2, nullptr, c.h16, c.s, c.ntok));
      break;
    case SdPath::CHAIN: {
      MDM_TRY(linear(c, xa, c.M, D, l.sd_q, l.sd_q_b, D, w.t1, nullptr, qo));
      // scores[b,h,s,n] = q . k
      GemmArgs g = per_head(c, heads(op_f32(w.t1, D), (int64_t)c.S * D, dh), heads(op_f32(kc, D), (int64_t)N * D, dh), c.S, N, dh,
                            N, (int64_t)H * c.S * N, (int64_t)c.S * N);
      g.C = w.scr;
      MDM_TRY(gemm(g, c.s));
      MDM_TRY(row_softmax(w.scr, c.M * H, N, c.s, c.ntok, (int64_t)H * c.S));
      // o[b,s,h,:] = p v
      GemmArgs pv = per_head(c, heads(op_f32(w.scr, N), (int64_t)H * c.S * N, (int64_t)c.S * N),
                             heads(op_f32_kstride(vc, D), (int64_t)N * D, dh), c.S, dh, N, D, (int64_t)c.S * D, dh);
      pv.C = c.bf ? nullptr : w.t2, pv.C16 = c.bf ? (uint16_t*)w.t2 : nullptr;
      MDM_TRY(gemm(pv, c.s));
      break;
    }
  }
  MDM_TRY(linear(c, att, c.M, D, l.sd_out, l.sd_out_b, D, w.t3, nullptr));
  MDM_TRY(ln_chain(w.t3, c.M, D, l.sd_ln_w, l.sd_ln_b, w.t4, fmt_mlp(c), nullptr, nullptr, nullptr, 0, c.s));
  return sd_ffn(c, l, x, out, out16);
}

const float* tc_at(const MdmModel& m, const MdmTextCache& tc, int layer) {
  const int dh = m.D / m.H;
  return tc.lin_at + (int64_t)layer * tc.B * m.H * dh * dh;
}
const float* tc_k(const MdmModel& m, const MdmTextCache& tc, int layer) {
  return tc.sd_k + (int64_t)layer * tc.B * tc.N * m.D;
}
const float* tc_v(const MdmModel& m, const MdmTextCache& tc, int layer) {
  return tc.sd_v + (int64_t)layer * tc.B * tc.N * m.D;
}
SdFold tc_fold(const MdmModel& m, const MdmTextCache& tc, int layer) {
  SdFold f;
  if (tc.sd_kfold && tc.sd_cb && tc.sd_vfold) {  // per layer: [B][passes][128][D], [B][passes][128], [B][passes][D][128]
    const int64_t np = sd_fold_passes(m.H, tc.N);
    f.kfold = tc.sd_kfold + (int64_t)layer * tc.B * np * 128 * m.D;
    f.cb = tc.sd_cb + (int64_t)layer * tc.B * np * 128;
    f.vfold = tc.sd_vfold + (int64_t)layer * tc.B * np * m.D * 128;
  }
  return f;
}

// one MoEExtendedDecoderLayer (transformer.py:55-64): x (+ bf16 shadow x16) is updated in place, (y, y16) is scratch
int decoder_layer(const Ctx& c, int layer, const MdmTextCache& tc, float* x, uint16_t* x16, float* y, uint16_t* y16,
                  const float* sc4, const int* forced, float* trace, int32_t* route_out = nullptr) {
  const MdmModel& m = *c.m;
  const MdmLayer& l = m.layers[layer];
  const int64_t scs = (int64_t)c.B * 2 * m.D, n = c.M * m.D;
  auto dump = [&](int slot, const float* p) -> int {
    if (!trace) return MDM_OK;
    return hipMemcpyAsync(trace + (int64_t)slot * n, p, n * sizeof(float), hipMemcpyDeviceToDevice, c.s) == hipSuccess
               ? MDM_OK
               : MDM_ERR_LAUNCH;
  };
  if (!c.bf) x16 = y16 = nullptr;  // the 16-bit shadows of the residual stream are read by the 16-bit modes only: do not write them here
  MDM_TRY(dual_block(c, l, x, x16, sc4, y, l.ca_norm_w, l.ca_norm_b));
  MDM_TRY(dump(0, y));
  const RoutePath rp = route_path(c, l);
  const MoeGateParams gp = gate_params(c, l, forced);
  StyleRoute sr;
  sr.gate = &gp, sr.E = m.E, sr.cursor = c.w.cursor;
  MDM_TRY(cross_block(c, l, tc_at(m, tc, layer), y, sc4 + 2 * scs, x, true, rp == RoutePath::FOLDED ? &sr : nullptr));
  MDM_TRY(dump(1, x));
  const SdFold fold = tc_fold(m, tc, layer);
  const TextPath tp = text_path(c, l, fold);
  const StyleText st = text_operands(c, l, fold);
  MDM_TRY(moe_block(c, l, x, sc4 + 3 * scs, forced, y, y16, route_out, rp, tp == TextPath::EPILOGUE ? &st : nullptr));
  MDM_TRY(dump(2, y));
  MDM_TRY(sdcross_block(c, l, tc_k(m, tc, layer), tc_v(m, tc, layer), y, y16, x, x16, fold, tp));
  return dump(3, x);
}

// fused time/text embedding + every stylization block's (scale|shift)  (transformer.py:313-321, stylization.py:22-27)
// gt = gated_fusion.proj_time(time_proj(time_embed(learnable_time_embed(t))))  [B, D] -> dst   (transformer.py:318-320)
int stem_time_branch(const Ctx& c, const int64_t* timesteps, int B, float* dst) {
  const MdmModel& m = *c.m;
  const int D = m.D, Te = 4 * D;
  const Work& w = c.w;
  LinOpts silu_o;
  silu_o.act = ACT_SILU;
  MDM_TRY(sinusoid(timesteps, B, D, w.s_a, c.s));
  MDM_TRY(linear(c, act_f32(w.s_a), B, D, m.tmlp0, m.tmlp0_b, 2 * D, w.s_b, nullptr, silu_o));
  MDM_TRY(linear(c, act_f32(w.s_b), B, 2 * D, m.tmlp2, m.tmlp2_b, D, w.s_a, nullptr));
  MDM_TRY(linear(c, act_f32(w.s_a), B, D, m.te0, m.te0_b, Te, w.s_b, nullptr, silu_o));
  MDM_TRY(linear(c, act_f32(w.s_b), B, Te, m.te2, m.te2_b, Te, w.s_c, nullptr));
  MDM_TRY(linear(c, act_f32(w.s_c), B, Te, m.tproj, m.tproj_b, D, w.s_a, nullptr));
  return linear(c, act_f32(w.s_a), B, D, m.gf_time, m.gf_time_b, D, dst, nullptr);
}

// gx = gated_fusion.proj_text([text_proj](xf_proj))  [B, D] -> dst      (transformer.py:313-315, gate.py:17)
int stem_text_branch(const Ctx& c, const float* xf_proj, int B, float* dst) {
  const MdmModel& m = *c.m;
  const float* tp = xf_proj;
  if (m.Dt != m.D) {  // the per-call random text_proj, captured
    if (!m.text_proj.hi) return MDM_ERR_ARG;
    MDM_TRY(linear(c, act_f32(xf_proj), B, m.Dt, m.text_proj, m.text_proj_b, m.D, c.w.s_c, nullptr));
    tp = c.w.s_c;
  }
  return linear(c, act_f32(tp), B, m.D, m.gf_text, m.gf_text_b, m.D, dst, nullptr);
}

// fused time/text embedding + every stylization block's (scale|shift)  (transformer.py:313-321, stylization.py:22-27)
int stem_embeddings(const Ctx& c, const int64_t* timesteps, const float* xf_proj, const MdmStemCache* sc_cache,
                    float* emb_out, float* sc_out) {
  const MdmModel& m = *c.m;
  const int D = m.D, Te = 4 * D, B = c.B, nblk = 8 * m.L;
  const Work& w = c.w;
  LinOpts silu_o;
  silu_o.act = ACT_SILU;
  // fused = sigmoid(t + x) * t + (1 - sigmoid) * x                  (gate.py:18-20) -> mix (fp32, or bf16 in throughput mode)
  float* mix = w.s_b;
  if (sc_cache && sc_cache->time_table && sc_cache->gx) {
    MDM_TRY(gated_mix_gather(sc_cache->time_table, timesteps, sc_cache->steps, sc_cache->gx, B, D, c.bf ? nullptr : mix,
                             c.bf ? (uint16_t*)mix : nullptr, c.h16, c.s));
  } else {
    // the two chains read fp32 rows and weights packed bf16 hi + lo in every mode: always the bf16x3 arithmetic, as the stem
    // cache tabulates them.  At the run's own `prec` the 16-bit modes made a single pass on the bf16 hi plane -- the fp16 mode
    // too, which has no fp16 image of these weights: a (scale | shift) row was then 5e-3 off in the mode whose rows hold 7e-4
    // (tests/frame_probe.py), and a forward with and without a stem cache differed by that much.
    Ctx c3 = c;
    c3.prec = 3;
    MDM_TRY(stem_time_branch(c3, timesteps, B, w.s_b));
    MDM_TRY(stem_text_branch(c3, xf_proj, B, w.s_a));
    MDM_TRY(gated_mix(w.s_b, w.s_a, (int64_t)B * D, w.s_c, c.s));
    if (c.bf) {
      MDM_TRY(to_bf16(w.s_c, (int64_t)B * D, (uint16_t*)w.s_b, c.h16, c.s));
    } else {
      mix = w.s_c;
    }
  }
  MDM_TRY(linear_to_act(c, act_of(c, mix), B, D, m.gf_post0, m.gf_post0_b, D, w.s_a, silu_o));
  float* emb = emb_out ? emb_out : w.emb;
  MDM_TRY(linear(c, act_of(c, w.s_a), B, D, m.gf_post2, m.gf_post2_b, D, emb, c.bf ? (uint16_t*)w.s_c : nullptr));
  // all 8L blocks at once: e1 = SiLU(emb Weph^T + beph) [B, 8L*Te]; sc[j] = e1[:, j] W1_j^T + b1_j [8L, B, 2D]
  MDM_TRY(linear_to_act(c, c.bf ? act_bf16((uint16_t*)w.s_c) : act_f32(emb), B, D, m.style_eph, m.style_eph_b, nblk * Te,
                        w.e1, silu_o));
  GemmArgs g = gd(c);
  if (c.bf) {
    g.A.p = w.e1, g.A.ld = (int64_t)nblk * Te, g.A.kind = OP_BF16_ROW, g.precision = 1;
  } else {
    g.A = op_f32(w.e1, (int64_t)nblk * Te);
  }
  g.A.bs1 = Te;
  g.W = packed(m.style_emb);
  g.W.bs1 = (int64_t)2 * D * m.style_emb.ld;
  g.M = B, g.N = 2 * D, g.K = Te;
  g.batch = nblk, g.nb2 = 1;
  g.bias = m.style_emb_b, g.bias_bs = 2 * D;
  g.C = sc_out, g.ldc = 2 * D, g.c_bs1 = (int64_t)B * 2 * D;
  return gemm(g, c.s);
}

int check_model(const MdmModel* m) {
  if (!m || !m->layers || m->D <= 0 || m->H <= 0 || m->D % m->H || m->L <= 0 || m->E < 2 || m->E > 16) return MDM_ERR_ARG;
  const int dh = m->D / m->H;
  if (dh != 16 && dh != 32 && dh != 64 && dh != 128 && dh != 256) return MDM_ERR_UNSUPPORTED;
  if (m->D > 1024 || m->Dt > 1024 || (m->D & 3) || (m->F & 3)) return MDM_ERR_UNSUPPORTED;
  return MDM_OK;
}

}  // namespace
}  // namespace mdm

using namespace mdm;

extern "C" {

int64_t mdm_workspace_bytes(const MdmModel* m, int32_t B, int32_t T, int32_t N) {
  if (check_model(m) != MDM_OK || B <= 0 || T <= 0) return -1;
  return carve(*m, B, T, N, nullptr).bytes;
}

int mdm_text_cache_build(const MdmModel* m, const float* xf_out, const MdmTextCache* tc, void* ws, int64_t ws_bytes,
                         int32_t precision, void* stream) {
  MDM_TRY(check_model(m));
  if (!xf_out || !tc || !tc->lin_at || !tc->sd_k || !tc->sd_v || tc->B <= 0 || tc->N <= 0 || tc->N > 128 || !ws)
    return MDM_ERR_ARG;
  Ctx c = {};
  // computed once per caption batch, never per step: always the bf16x3 arithmetic (its weights are packed bf16 hi + lo in
  // every mode); `precision` only selects the 16-bit format of the folded K' / V' images
  c.m = m, c.s = (hipStream_t)stream, c.prec = 3, c.bf = false, c.mix = false, c.B = tc->B, c.N = tc->N;
  c.ntok = tc->ntok;
  c.h16 = (precision == MDM_PREC_F16 || precision == MDM_PREC_MIXED || precision == MDM_PREC_FP8) ? MDM_H16_F16 : MDM_H16_BF16;
  c.w = carve(*m, tc->B, 2, tc->N, ws);
  if (c.w.bytes > ws_bytes) return MDM_ERR_ARG;
  const int D = m->D, H = m->H, dh = D / H, N = tc->N, B = tc->B;
  const int64_t BN = (int64_t)B * N;
  for (int layer = 0; layer < 2 * m->L; ++layer) {
    const MdmLayer& l = m->layers[layer];
    MDM_TRY(ln_chain(xf_out, BN, m->Dt, l.ca_tnorm_w, l.ca_tnorm_b, c.w.tn, 0, nullptr, nullptr, nullptr, 0, c.s));
    MDM_TRY(linear(c, act_f32(c.w.tn), BN, m->Dt, l.ca_k, l.ca_k_b, D, c.w.kb, nullptr));
    MDM_TRY(col_softmax(c.w.kb, B, N, D, c.s, tc->ntok));  // softmax over text tokens (fast_attention.py:249)
    MDM_TRY(linear(c, act_f32(c.w.tn), BN, m->Dt, l.ca_v, l.ca_v_b, D, c.w.vb, nullptr));
    GemmArgs g = gemm_defaults(3);  // A^T[b,h][l][d] = sum_n v[n,l] k[n,d]   (fast_attention.py:252)
    g.A = op_f32_kstride(c.w.vb, D);
    g.A.bs1 = (int64_t)N * D, g.A.bs2 = dh;
    g.W = op_f32_kstride(c.w.kb, D);
    g.W.bs1 = (int64_t)N * D, g.W.bs2 = dh;
    g.M = dh, g.N = dh, g.K = N;
    g.batch = B * H, g.nb2 = H;
    g.C = (float*)tc_at(*m, *tc, layer), g.ldc = dh, g.c_bs1 = (int64_t)H * dh * dh, g.c_bs2 = (int64_t)dh * dh;
    MDM_TRY(gemm(g, c.s));
    MDM_TRY(linear(c, act_f32(xf_out), BN, m->Dt, l.sd_k, l.sd_k_b, D, (float*)tc_k(*m, *tc, layer), nullptr));
    MDM_TRY(linear(c, act_f32(xf_out), BN, m->Dt, l.sd_v, l.sd_v_b, D, (float*)tc_v(*m, *tc, layer), nullptr));
    if (tc->sd_kfold && tc->sd_cb && tc->sd_vfold) {
      // fold the query / output projections into the text side (csrc/sdfold.hip), fp32-grade arithmetic, bf16 results
      if (!l.sd_q_w32 || !l.sd_out_w32 || sd_fold_policy(D, H, N) <= 0) return MDM_ERR_ARG;
      const SdFold f = tc_fold(*m, *tc, layer);
      const float scale = 1.f / sqrtf((float)dh);
      const float* kc = tc_k(*m, *tc, layer);
      const float* vc = tc_v(*m, *tc, layer);
      const int hpp = sd_fold_heads_per_pass(H, N), np = sd_fold_passes(H, N);
      for (int ps = 0; ps < np; ++ps) {  // one pass = hc whole heads, packed as rows / columns hs * N + n of a 128-wide image
        const int h0 = ps * hpp, hc = (H - h0) < hpp ? (H - h0) : hpp;
        {  // K'[b][ps][hs*N + n][j] = scale * sum_d key[b,n,h*dh+d] Wq[h*dh+d, j]
          GemmArgs g = gemm_defaults(3);
          g.A = op_f32(kc + h0 * dh, D);
          g.A.bs1 = (int64_t)N * D, g.A.bs2 = dh;
          g.W = op_f32_kstride(l.sd_q_w32 + (int64_t)h0 * dh * D, D);
          g.W.bs1 = 0, g.W.bs2 = (int64_t)dh * D;
          g.M = N, g.N = D, g.K = dh;
          g.batch = B * hc, g.nb2 = hc;
          g.alpha = scale;
          g.h16 = c.h16;
          g.C16 = (uint16_t*)f.kfold + (int64_t)ps * 128 * D, g.ldc = D, g.c_bs1 = (int64_t)np * 128 * D, g.c_bs2 = (int64_t)N * D;
          MDM_TRY(gemm(g, c.s));
        }
        {  // cb[b][ps][hs*N + n] = scale * key[b,n,h*dh:] . bq[h*dh:]
          GemmArgs g = gemm_defaults(3);
          g.A = op_f32(kc + h0 * dh, D);
          g.A.bs1 = (int64_t)N * D, g.A.bs2 = dh;
          g.W = op_f32(l.sd_q_b + h0 * dh, dh);
          g.W.bs1 = 0, g.W.bs2 = dh;
          g.M = N, g.N = 1, g.K = dh;
          g.batch = B * hc, g.nb2 = hc;
          g.alpha = scale;
          g.C = (float*)f.cb + ps * 128, g.ldc = 1, g.c_bs1 = (int64_t)np * 128, g.c_bs2 = N;
          MDM_TRY(gemm(g, c.s));
        }
        {  // V'^T[b][ps][j][hs*N + n] = sum_d Wout[j, h*dh+d] value[b,n,h*dh+d]
          GemmArgs g = gemm_defaults(3);
          g.A = op_f32(l.sd_out_w32 + h0 * dh, D);
          g.A.bs1 = 0, g.A.bs2 = dh;
          g.W = op_f32(vc + h0 * dh, D);
          g.W.bs1 = (int64_t)N * D, g.W.bs2 = dh;
          g.M = D, g.N = N, g.K = dh;
          g.batch = B * hc, g.nb2 = hc;
          g.h16 = c.h16;
          g.C16 = (uint16_t*)f.vfold + (int64_t)ps * D * 128, g.ldc = 128, g.c_bs1 = (int64_t)np * D * 128, g.c_bs2 = N;
          MDM_TRY(gemm(g, c.s));
        }
      }
      // per-sample token counts: the folded columns of a sample's padding tokens get a bias that makes their probability 0
      MDM_TRY(sd_fold_mask_cb((float*)f.cb, B, np, hpp, N, tc->ntok, c.s));
    }
  }
  return MDM_OK;
}

int mdm_stem_embeddings(const MdmModel* m, const int64_t* timesteps, const float* xf_proj, int32_t B, float* emb_out,
                        float* sc_out, void* ws, int64_t ws_bytes, int32_t precision, void* stream) {
  MDM_TRY(check_model(m));
  if (!timesteps || !xf_proj || !sc_out || !ws || B <= 0) return MDM_ERR_ARG;
  Ctx c = {};
  c.m = m, c.s = (hipStream_t)stream, c.B = B;
  if (!set_precision(c, m, precision)) return MDM_ERR_UNSUPPORTED;
  c.w = carve(*m, B, 2, 1, ws);
  if (c.w.bytes > ws_bytes) return MDM_ERR_ARG;
  return stem_embeddings(c, timesteps, xf_proj, nullptr, emb_out, sc_out);
}

int mdm_stem_cache_build(const MdmModel* m, int32_t steps, float* time_table, const float* xf_proj, int32_t B, float* gx,
                         void* ws, int64_t ws_bytes, int32_t precision, void* stream) {
  MDM_TRY(check_model(m));
  if (!ws || (time_table && steps <= 0) || (gx && (!xf_proj || B <= 0))) return MDM_ERR_ARG;
  constexpr int CH = 128;
  Ctx c = {};
  // tabulated in the fp32-grade arithmetic regardless of the run mode: it is computed once per loop
  c.m = m, c.s = (hipStream_t)stream, c.prec = 3, c.bf = false, c.mix = false, c.h16 = MDM_H16_BF16, c.B = CH;
  (void)precision;
  c.w = carve(*m, CH, 2, 1, ws);
  if (c.w.bytes > ws_bytes) return MDM_ERR_ARG;
  int64_t* ts = (int64_t*)c.w.hid;  // scratch for the timestep ramp
  if (time_table)
    for (int t0 = 0; t0 < steps; t0 += CH) {
      const int n = steps - t0 < CH ? steps - t0 : CH;
      MDM_TRY(iota_i64(ts, n, t0, c.s));
      MDM_TRY(stem_time_branch(c, ts, n, time_table + (int64_t)t0 * m->D));
    }
  if (gx)
    for (int b0 = 0; b0 < B; b0 += CH) {
      const int n = B - b0 < CH ? B - b0 : CH;
      MDM_TRY(stem_text_branch(c, xf_proj + (int64_t)b0 * m->Dt, n, gx + (int64_t)b0 * m->D));
    }
  return MDM_OK;
}

int mdm_denoiser_forward(const MdmModel* m, const MdmTextCache* tc, const float* x, const int64_t* timesteps,
                         const int32_t* length, const float* xf_proj, int32_t B, int32_t T, float* out, void* ws,
                         int64_t ws_bytes, const int32_t* forced_routing, float* trace, const MdmStemCache* stem,
                         int32_t precision, void* stream) {
  MDM_TRY(check_model(m));
  if (!tc || !x || !timesteps || !length || !xf_proj || !out || !ws || B <= 0 || T <= 0) return MDM_ERR_ARG;
  if (T % 2 || T > m->num_frames) return MDM_ERR_ARG;  // odd T breaks the U-shape (transformer.py:223-224,353)
  if (tc->B != B) return MDM_ERR_ARG;
  Ctx c = {};
  c.m = m, c.s = (hipStream_t)stream, c.B = B, c.N = tc->N;
  c.ntok = tc->ntok;
  if (!set_precision(c, m, precision)) return MDM_ERR_UNSUPPORTED;
  c.w = carve(*m, B, T, tc->N, ws);
  if (c.w.bytes > ws_bytes) return MDM_ERR_ARG;
  const Work& w = c.w;
  const int D = m->D, L = m->L;
  const int64_t Mfull = (int64_t)B * T, Mlow = Mfull / 2;
  const int64_t scl = (int64_t)4 * B * 2 * D;  // (scale|shift) floats per layer
  MDM_TRY(stem_embeddings(c, timesteps, xf_proj, stem, nullptr, w.sc));
  // h = joint_embed(x) + sequence_embedding[:T]                     (transformer.py:324-326)
  {
    LinOpts o;
    o.R1 = m->seq_emb, o.r1_mod = T;
    // the root of the residual stream (and of the U's skip connection): always the bf16x3 arithmetic -- 3.4 GFLOP, K = 263.
    // Measured at B = 32 / T = 196 / L = 4, fp16 mode, free routing: 1679 -> 596 of 75264 routing decisions differ from the
    // fp32-grade run, median frame error 4.7e-3 -> 1.8e-3 (tools/mode_compare.py).
    // The same treatment of down / up / the stem GEMMs bought another 14 % for +0.2 ms per step: not taken.
    Ctx cj = c;
    cj.prec = 3;
    MDM_TRY(linear(cj, act_f32(x), Mfull, m->feats, m->joint, m->joint_b, D, w.h0, c.bf ? w.h016 : nullptr, o));
  }
  // Conv1d(k=2,s=2) == Linear over pairs of frames                  (:332-337)
  MDM_TRY(linear(c, c.bf ? act_bf16(w.h016) : act_f32(w.h0), Mlow, 2 * D, m->down, m->down_b, D, w.xa,
                 c.bf ? w.xa16 : nullptr));
  MDM_TRY(halve_lengths(length, B, w.len_low, c.s));  // (:341-342)
  c.S = T / 2, c.M = Mlow, c.len = w.len_low;
  if (g_route_dump && g_route_cap < (int64_t)2 * L * 4 * Mfull) return MDM_ERR_ARG;  // the dump buffer is too small for this forward
  for (int i = 0; i < L; ++i) {  // coarse scale blocks, in place on xa (xb = scratch)      (:343-344)
    const int32_t* fr = forced_routing ? forced_routing + (int64_t)i * 4 * Mfull : nullptr;
    float* tr = trace ? trace + (int64_t)i * 4 * Mfull * D : nullptr;
    int32_t* rd = g_route_dump ? g_route_dump + (int64_t)i * 4 * Mfull : nullptr;
    MDM_TRY(decoder_layer(c, i, *tc, w.xa, w.xa16, w.xb, w.xb16, w.sc + i * scl, fr, tr, rd));
  }
  // ConvTranspose1d(k=2,s=2) == Linear D -> 2D per coarse frame, rows (B*T/2, 2D) == (B*T, D); + skip h  (:347-353)
  {
    LinOpts o;
    o.R1 = w.h0;
    MDM_TRY(linear(c, c.bf ? act_bf16(w.xa16) : act_f32(w.xa), Mlow, D, m->up, m->up_b2, 2 * D, w.xb,
                   c.bf ? w.xb16 : nullptr, o));
  }
  c.S = T, c.M = Mfull, c.len = length;
  for (int i = 0; i < L; ++i) {  // full scale blocks, in place on xb                        (:356-357)
    const int32_t* fr = forced_routing ? forced_routing + (int64_t)(L + i) * 4 * Mfull : nullptr;
    float* tr = trace ? trace + (int64_t)(L + i) * 4 * Mfull * D : nullptr;
    int32_t* rd = g_route_dump ? g_route_dump + (int64_t)(L + i) * 4 * Mfull : nullptr;
    MDM_TRY(decoder_layer(c, L + i, *tc, w.xb, w.xb16, w.xa, w.xa16, w.sc + (L + i) * scl, fr, tr, rd));
  }
  return linear(c, c.bf ? act_bf16(w.xb16) : act_f32(w.xb), Mfull, D, m->out, m->out_b, m->feats, out, nullptr);  // (:360)
}

int mdm_block_forward(const MdmModel* m, int32_t layer, int32_t block, const MdmTextCache* tc, const float* h,
                      const float* sc, const int32_t* len, int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes,
                      const int32_t* forced_routing, int32_t precision, void* stream) {
  MDM_TRY(check_model(m));
  if (!h || !sc || !len || !out || !ws || B <= 0 || S <= 0 || layer < 0 || layer >= 2 * m->L) return MDM_ERR_ARG;
  if ((block == MDM_BLOCK_CROSS || block == MDM_BLOCK_SDCROSS || block == MDM_BLOCK_LAYER) && (!tc || tc->B != B))
    return MDM_ERR_ARG;
  Ctx c = {};
  c.m = m, c.s = (hipStream_t)stream, c.B = B, c.S = S, c.M = (int64_t)B * S, c.len = len;
  if (!set_precision(c, m, precision)) return MDM_ERR_UNSUPPORTED;
  c.N = tc ? tc->N : 1;
  c.ntok = tc ? tc->ntok : nullptr;
  c.w = carve(*m, B, S, c.N, ws);
  if (c.w.bytes > ws_bytes) return MDM_ERR_ARG;
  const MdmLayer& l = m->layers[layer];
  const int64_t scs = (int64_t)B * 2 * m->D, n = c.M * m->D;
  if (c.bf && (n & 3)) return MDM_ERR_UNSUPPORTED;
  if (c.bf) MDM_TRY(to_bf16(h, n, c.w.h016, c.h16, c.s));  // callers hand over fp32 only: build the 16-bit shadow here
  switch (block) {
    case MDM_BLOCK_DUAL: return dual_block(c, l, h, c.w.h016, sc, out);
    case MDM_BLOCK_CROSS: return cross_block(c, l, tc_at(*m, *tc, layer), h, sc + 2 * scs, out);
    case MDM_BLOCK_MOE:
      if (g_route_dump && g_route_cap < 4 * c.M) return MDM_ERR_ARG;
      return moe_block(c, l, h, sc + 3 * scs, forced_routing, out, nullptr, g_route_dump);
    case MDM_BLOCK_SDCROSS:
      return sdcross_block(c, l, tc_k(*m, *tc, layer), tc_v(*m, *tc, layer), h, c.w.h016, out, nullptr,
                           tc_fold(*m, *tc, layer));
    case MDM_BLOCK_LAYER: {
      if (hipMemcpyAsync(c.w.xa, h, n * sizeof(float), hipMemcpyDeviceToDevice, c.s) != hipSuccess) return MDM_ERR_LAUNCH;
      if (c.bf) MDM_TRY(to_bf16(h, n, c.w.xa16, c.h16, c.s));
      MDM_TRY(decoder_layer(c, layer, *tc, c.w.xa, c.w.xa16, c.w.xb, c.w.xb16, sc, forced_routing, nullptr));
      return hipMemcpyAsync(out, c.w.xa, n * sizeof(float), hipMemcpyDeviceToDevice, c.s) == hipSuccess ? MDM_OK
                                                                                                         : MDM_ERR_LAUNCH;
    }
    default: return MDM_ERR_ARG;
  }
}

// ---- per-block entry points named as SURVEY.md §8(b) lists them: thin views of mdm_block_forward -----------------------
int mdm_moe_ffn_forward(const MdmModel* m, int32_t layer, const float* h, const float* sc4, const int32_t* len, int32_t B,
                        int32_t S, float* out, void* ws, int64_t ws_bytes, const int32_t* forced_routing,
                        int32_t precision, void* stream) {
  return mdm_block_forward(m, layer, MDM_BLOCK_MOE, nullptr, h, sc4, len, B, S, out, ws, ws_bytes, forced_routing, precision,
                           stream);
}
int mdm_dual_self_attn_forward(const MdmModel* m, int32_t layer, const float* h, const float* sc4, const int32_t* len,
                               int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes, int32_t precision,
                               void* stream) {
  return mdm_block_forward(m, layer, MDM_BLOCK_DUAL, nullptr, h, sc4, len, B, S, out, ws, ws_bytes, nullptr, precision, stream);
}
int mdm_linear_xattn_forward(const MdmModel* m, int32_t layer, const MdmTextCache* tc, const float* h, const float* sc4,
                             const int32_t* len, int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes,
                             int32_t precision, void* stream) {
  return mdm_block_forward(m, layer, MDM_BLOCK_CROSS, tc, h, sc4, len, B, S, out, ws, ws_bytes, nullptr, precision, stream);
}
int mdm_softmax_xattn_ffn_forward(const MdmModel* m, int32_t layer, const MdmTextCache* tc, const float* h,
                                  const float* sc4, const int32_t* len, int32_t B, int32_t S, float* out, void* ws,
                                  int64_t ws_bytes, int32_t precision, void* stream) {
  return mdm_block_forward(m, layer, MDM_BLOCK_SDCROSS, tc, h, sc4, len, B, S, out, ws, ws_bytes, nullptr, precision, stream);
}
// one PerformerSelfAttention (fast_attention.py:137-179): which = 0 local_attn, 1 global_attn; sc = that block's
// (scale|shift) rows [B, 2D]
int mdm_performer_attn_forward(const MdmModel* m, int32_t layer, int32_t which, const float* h, const float* sc,
                               const int32_t* len, int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes,
                               int32_t precision, void* stream) {
  MDM_TRY(check_model(m));
  if (!h || !sc || !len || !out || !ws || B <= 0 || S <= 0 || layer < 0 || layer >= 2 * m->L || which < 0 || which > 1)
    return MDM_ERR_ARG;
  Ctx c = {};
  c.m = m, c.s = (hipStream_t)stream, c.B = B, c.S = S, c.M = (int64_t)B * S, c.len = len, c.N = 1;
  if (!set_precision(c, m, precision)) return MDM_ERR_UNSUPPORTED;
  c.w = carve(*m, B, S, 1, ws);
  if (c.w.bytes > ws_bytes) return MDM_ERR_ARG;
  const MdmLayer& l = m->layers[layer];
  const MdmPerformer& p = which ? l.global : l.local;
  MDM_TRY(ln_chain(h, c.M, m->D, p.pre_w, p.pre_b, c.w.t3, fmt16(c), nullptr, nullptr, nullptr, 0, c.s));
  return performer(c, p, h, act_of(c, c.w.t3), sc, out);
}

int mdm_stylization_forward(const MdmStyle* st, const float* h, const float* sc, int32_t B, int32_t S, int32_t D,
                            float* tmp, float* out, int32_t precision, void* stream) {
  if (!st || !h || !sc || !tmp || !out || B <= 0 || S <= 0) return MDM_ERR_ARG;
  MdmModel fake = {};
  fake.D = D;
  Ctx c = {};
  fake.F = D;
  c.m = &fake, c.s = (hipStream_t)stream, c.B = B, c.S = S, c.M = (int64_t)B * S;
  if (!set_precision(c, &fake, precision)) return MDM_ERR_UNSUPPORTED;
  return style_apply(c, *st, h, nullptr, nullptr, nullptr, sc, tmp, nullptr, 1.f, nullptr, out);
}

int64_t mdm_text_head_workspace_bytes(int32_t B, int32_t N0, int32_t P, int32_t Hs, int32_t Dt) {
  if (B <= 0 || N0 < 0 || P < 0 || Hs <= 0 || Dt <= 0) return -1;
  const int64_t fl = (int64_t)B * N0 * Hs + (int64_t)P * Hs + (int64_t)B * N0 * Dt + (int64_t)P * Dt;
  return ((fl * 4 + 255) & ~(int64_t)255) + 1024;
}

// EnhancedTextEncoder's projection head (text_encoder.py:13-18,39-43) on the hidden states of any text encoder
int mdm_text_head_forward(const float* hidden, const float* prompts, const float* ln_w, const float* ln_b,
                          const MdmPacked* w, const float* bias, int32_t B, int32_t N0, int32_t P, int32_t Hs,
                          int32_t Dt, float* xf_out, float* xf_proj, void* ws, int64_t ws_bytes, int32_t precision,
                          void* stream) {
  if (!ln_w || !ln_b || !w || !w->hi || !xf_out || !xf_proj || !ws || B <= 0 || N0 < 0 || P < 0 || N0 + P <= 0 ||
      (N0 > 0 && !hidden) || (P > 0 && !prompts))
    return MDM_ERR_ARG;
  if (precision != 1 && precision != 3) return MDM_ERR_ARG;
  if (precision == 3 && !w->lo) return MDM_ERR_ARG;
  if (ws_bytes < mdm_text_head_workspace_bytes(B, N0, P, Hs, Dt)) return MDM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  Bump b(ws);
  float* lnh = b.take<float>((int64_t)B * N0 * Hs);
  float* lnp = b.take<float>((int64_t)P * Hs);
  float* ph = b.take<float>((int64_t)B * N0 * Dt);
  float* pp = b.take<float>((int64_t)P * Dt);
  MdmModel fake = {};
  Ctx c = {};
  c.m = &fake, c.s = s, c.prec = precision, c.bf = false, c.mix = false, c.h16 = MDM_H16_BF16;
  LinOpts o;
  o.act = ACT_GELU;
  if (N0 > 0) {
    MDM_TRY(ln_chain(hidden, (int64_t)B * N0, Hs, ln_w, ln_b, lnh, 0, nullptr, nullptr, nullptr, 0, s));
    MDM_TRY(linear(c, act_f32(lnh), (int64_t)B * N0, Hs, *w, bias, Dt, ph, nullptr, o));
  }
  if (P > 0) {  // the prompt rows are the same for every caption: projected once, broadcast by the assemble kernel
    MDM_TRY(ln_chain(prompts, P, Hs, ln_w, ln_b, lnp, 0, nullptr, nullptr, nullptr, 0, s));
    MDM_TRY(linear(c, act_f32(lnp), P, Hs, *w, bias, Dt, pp, nullptr, o));
  }
  return text_assemble(pp, ph, B, N0, P, Dt, xf_out, xf_proj, s);
}

// generated motions -> joint positions (tools/visualization.py:21-27,89; utils/motion_process.py:362-416; utils/utils.py:125-130)
int mdm_motion_postprocess(const float* motion, const int32_t* length, const float* mean, const float* std, int32_t B,
                           int32_t T, int32_t feats, int32_t joints, int32_t radius, const double* weights,
                           float* scratch, float* joints_out, void* stream) {
  if (!motion || !mean || !std || !scratch || !joints_out || B <= 0 || T <= 0 || joints < 1 || radius < 0 ||
      (radius > 0 && !weights))
    return MDM_ERR_ARG;
  if (feats < 4 + 3 * (joints - 1)) return MDM_ERR_ARG;
  return motion_post(motion, length, mean, std, B, T, feats, joints, radius, weights, scratch, joints_out,
                     (hipStream_t)stream);
}

// passes of <= 128 folded text columns that sd_fold takes for (H heads, N text tokens); 0 = unsupported: sizes the
// MdmTextCache.sd_kfold / sd_cb / sd_vfold buffers ([L2][B][passes][128][D], [L2][B][passes][128], [L2][B][passes][D][128])
int mdm_sd_fold_passes(int32_t D, int32_t H, int32_t N) { return sd_fold_policy(D, H, N); }

int mdm_route_workspace(const MdmModel* m, int32_t B, int32_t T, int32_t N, int64_t* off) {
  if (check_model(m) != MDM_OK || B <= 0 || T <= 0 || !off) return MDM_ERR_ARG;
  uint8_t* const base = (uint8_t*)4096;  // (never dereferenced: carve() only adds to it)
  const Work w = carve(*m, B, T, N, base);
  const void* p[8] = {w.hn, w.top_idx, w.top_val, w.perm, w.rowscale, w.pos4, w.goff, w.cursor};
  for (int i = 0; i < 8; ++i) off[i] = (const uint8_t*)p[i] - base;
  return MDM_OK;
}

int mdm_expert_workspace(const MdmModel* m, int32_t B, int32_t T, int32_t N, int64_t* off) {
  if (check_model(m) != MDM_OK || B <= 0 || T <= 0 || !off) return MDM_ERR_ARG;
  uint8_t* const base = (uint8_t*)4096;  // (never dereferenced: carve() only adds to it)
  const Work w = carve(*m, B, T, N, base);
  const void* p[3] = {w.hn_scale, w.hid, w.y2};
  for (int i = 0; i < 3; ++i) off[i] = (const uint8_t*)p[i] - base;
  return MDM_OK;
}

int mdm_workspace_layout(const MdmModel* m, int32_t B, int32_t T, int32_t N, int64_t* off, int64_t* bytes, int32_t* kind,
                         int32_t cap) {
  if (check_model(m) != MDM_OK || B <= 0 || T <= 0 || cap < 0 || (cap > 0 && (!off || !bytes || !kind))) return -1;
  WorkLayout lay{off, bytes, kind, cap};
  carve(*m, B, T, N, nullptr, &lay);  // (measuring mode: nothing is dereferenced)
  return lay.count;
}

const char* mdm_workspace_field_name(int32_t i) { return i >= 0 && i < kWorkFields ? kWorkFieldNames[i] : ""; }

int mdm_route_dump(int32_t* buf, int64_t capacity) {
  if (buf && capacity <= 0) return MDM_ERR_ARG;
  g_route_dump = buf, g_route_cap = buf ? capacity : 0;
  return MDM_OK;
}

int mdm_probe_enable(int32_t enable) {
  if (enable && !g_probe.made) {
    for (int i = 0; i < PROBE_MAX; ++i)
      if (hipEventCreate(&g_probe.a[i]) != hipSuccess || hipEventCreate(&g_probe.b[i]) != hipSuccess) return MDM_ERR_LAUNCH;
    g_probe.made = true;
  }
  g_probe.on = enable != 0;
  if (enable) g_probe.n = 0;
  return MDM_OK;
}

int mdm_probe_read(float* us, int32_t* rows, int32_t cap) {
  const int n = g_probe.n;
  for (int i = 0; i < n && i < cap; ++i) {
    if (hipEventSynchronize(g_probe.b[i]) != hipSuccess) return -1;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_probe.a[i], g_probe.b[i]) != hipSuccess) return -1;
    if (us) us[i] = ms * 1e3f;
    if (rows) rows[i] = g_probe.rows[i];
  }
  return n;
}

int mdm_cfg_posterior_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, int64_t n,
                           const float* tab, int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale,
                           int32_t clip_denoised, float* x_out, float* x0_out, void* stream) {
  if (steps <= 0 || (!t_dev && (t_imm < 0 || t_imm >= steps))) return MDM_ERR_ARG;
  return cfg_step(x, eps_c, eps_u, noise, n, tab, steps, t_dev, t_imm, cfg_scale, clip_denoised, x_out, x0_out,
                  (hipStream_t)stream);
}

int mdm_ddim_step(const float* x, const float* eps, const float* noise, int64_t n, const float* tab, int32_t steps,
                  const int32_t* t_dev, int32_t t_imm, float eta, int32_t clip_denoised, float* x_out, float* x0_out,
                  void* stream) {
  if (steps <= 0 || (!t_dev && (t_imm < 0 || t_imm >= steps))) return MDM_ERR_ARG;
  return ddim_step(x, eps, noise, n, tab, steps, t_dev, t_imm, eta, clip_denoised, x_out, x0_out, (hipStream_t)stream);
}

int mdm_xattn_gate(const float* gate, const float* adaptive_gate, int32_t D, float* out, void* stream) {
  if (!gate || !adaptive_gate || !out || D <= 0) return MDM_ERR_ARG;
  return xattn_gate(gate, adaptive_gate, D, out, (hipStream_t)stream);
}

}  // extern "C"
