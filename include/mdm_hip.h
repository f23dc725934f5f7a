/* mdm_hip.h -- C ABI of libmdm_hip.so: the MI355X (gfx950) denoising hot path of
 * ltdoanh2004/MotionDiffusion-MoE.
 *
 * Conventions (every entry point):
 *   - raw DEVICE pointers + sizes, no torch types; `stream` is a hipStream_t passed as void*;
 *   - returns 0 on success (MDM_OK), non-zero status otherwise; never allocates, never synchronises,
 *     never copies to the host: safe to capture into a hipGraph;
 *   - tensors are fp32 row-major unless stated; "packed" weights are bf16 planes produced by
 *     mdm_pack_bf16 (hi plane, optional lo plane for the bf16x3 fp32-grade mode);
 *   - `precision`: 1 = single bf16 MFMA pass, 3 = bf16x3 split (hi*hi + hi*lo + lo*hi), fp32-grade.
 *
 * The reference has no FFI: its boundary is the Python call `model(x, t, **kwargs)`
 * (text2motion/models/gaussian_diffusion.py:493) resolved by MotionTransformer.forward
 * (text2motion/models/transformer.py:291-361).  Each entry point below names the reference lines it replaces;
 * the Python side that binds them (ctypes) is motiondiffusion-moe_amd/_lib.py, see INTEGRATION.md.
 */
#ifndef MDM_HIP_H
#define MDM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MDM_OK = 0, MDM_ERR_ARG = 1, MDM_ERR_LAUNCH = 2, MDM_ERR_UNSUPPORTED = 3 };
enum { MDM_OP_F32_ROW = 0, MDM_OP_F32_KSTRIDE = 1, MDM_OP_BF16_ROW = 2, MDM_OP_FP8_ROW = 3 /* e4m3 bytes, csrc/gemm8.hip */,
       /* activation rows PRE-SPLIT for the fp32-grade kernel (csrc/gemm3.hip): per row and per block of 32 k, 32 bf16 "hi" then 32
        * bf16 "lo" = rn(x - hi) -- 128 bytes, exactly the bytes of the 32 fp32 values they replace, so `ld` (in 4-byte units, as for
        * MDM_OP_F32_ROW) and every buffer size stay what they are for fp32 rows.  Written by the producers (MdmGemmDesc.Cx2 and the
        * row-wise / attention kernels) so that the GEMM's K loop does not re-split each fp32 fragment in every wave that reads it */
       MDM_OP_X2_ROW = 4 };
enum { MDM_ACT_NONE = 0, MDM_ACT_GELU = 1, MDM_ACT_SILU = 2, MDM_ACT_FEAT = 3,
       /* fp32-grade kernel only (precision 3, N % 128 == 0): every 128-column slice of a row is one attention head --
        * LayerNorm over the slice with hn_w / hn_b (eps 1e-5), L2-normalised when the slice index is < hn_l2_tiles
        * (fast_attention.py:44-55 on the q | k | v projection), written as bf16 hi / lo planes C16 / C16_lo */
       MDM_ACT_HEADNORM = 4,
       /* the same kernel: softmax over every 128-column slice (the head_dim softmax of the linear cross-attention's query,
        * fast_attention.py:248), written as bf16 hi / lo planes C16 / C16_lo */
       MDM_ACT_HEADSOFTMAX = 5 };
/* 16-bit operand / storage format of the single-pass MFMA kernels: bf16, or IEEE fp16 (same MFMA rate on gfx950, 8x finer
 * rounding, |x| <= 65504: used where the value range is known). */
enum { MDM_H16_BF16 = 1, MDM_H16_F16 = 2 };
/* `precision` of the model-level entry points:
 *   1  single bf16 MFMA pass, GEMM-only tensors stored bf16 (throughput; BASELINE configs[1] names bf16)
 *   2  single fp16 MFMA pass, GEMM-only tensors stored fp16 (same speed, ~8x smaller error)
 *   3  bf16x3 split products everywhere, fp32 activations (fp32-grade: the mode that meets the 1e-3 parity bar)
 *   4  mixed: bf16x3 for everything that feeds the fp32 residual stream and the MoE router, single fp16 pass for the
 *      MFMA-bound GEMMs only (expert MLPs, the 4x FFN of the text cross-attention block)
 *   5  as 2, with the expert GEMMs on fp8 (e4m3) operands: activations quantised per row by the router kernel, weights per
 *      output channel at pack time, block-scaled MFMA with unit block scales (csrc/gemm8.hip); BASELINE configs[4]
 * The packed weights must be in the matching format (packing.py: weight_format).
 * Widths: 2 and 4 need D and F in multiples of 64 (the k-tile of the 16-bit kernels), 5 in multiples of 128; a model-level entry
 * point called with another shape returns MDM_ERR_UNSUPPORTED before any launch and writes nothing.  1 runs on fp32 rows there. */
enum { MDM_PREC_BF16 = 1, MDM_PREC_F16 = 2, MDM_PREC_X3 = 3, MDM_PREC_MIXED = 4, MDM_PREC_FP8 = 5 };

/* One GEMM operand: a [rows x K] matrix seen through a loader kind (see csrc/gemm.h). */
typedef struct MdmOperand {
  const void* p;
  const void* p_lo;      /* BF16_ROW: lo plane (precision 3) or NULL */
  int64_t ld;            /* F32_ROW/BF16_ROW: elements between rows; F32_KSTRIDE: elements between k */
  int64_t gstride;       /* F32_ROW: row r -> (r / rpg) * gstride + (r % rpg) * ld when rpg > 0 */
  const int32_t* gather; /* F32_ROW: optional row gather */
  int64_t bs1, bs2;      /* batch strides: z -> (z / nb2) * bs1 + (z % nb2) * bs2 */
  int32_t rpg;
  int32_t kind;
} MdmOperand;

/* C = epilogue(A[M,K] * W[N,K]^T):
 *   v = alpha * (acc + bias[n]);  v = act(v);  v *= out_scale * colscale[n] * rowscale[m];
 *   v += r1_scale * R1[m (mod r1_mod), n] + R2[m, n]
 * Replaces every nn.Linear / einsum on the path (transformer.py:319-360, fast_attention.py:59-78,
 * 145-147,165,248-253,305-329, switch_moe.py:104, stylization.py:26-30).
 * Alignment: when ldc, ldr1 and ldr2 are all multiples of 4 the MFMA tile kernels move four columns per lane, so C, R1, R2 must then be
 * 16-byte aligned, C16 / C16_lo 8-byte and C8 4-byte aligned, and with batch > 1 c_bs1 / c_bs2 multiples of 4; a launch that
 * only those kernels can run (16-bit, pre-split or fp8 rows, plane / Cx2 outputs) returns MDM_ERR_UNSUPPORTED otherwise and writes
 * nothing, a Linear on fp32 rows runs on the element-wise kernel.  With an odd leading dimension any 4-byte (C16: 2-byte) aligned
 * base is taken.  A.p of 16-bit, pre-split and fp8 rows is 16-byte aligned with A.ld * element size a multiple of 16. */
typedef struct MdmGemmDesc {
  MdmOperand A, W;
  int32_t M, N, K;
  int32_t batch, nb2;
  const int32_t* goff; /* grouped mode: row ranges [goff[g], goff[g+1]) use W + g*W.bs1, bias + g*bias_bs */
  int32_t ngroups;
  int32_t act;
  float* C;       /* fp32 output (may be NULL when C16 is set) */
  int64_t ldc, c_bs1, c_bs2;
  uint16_t* C16;  /* optional bf16 copy of the output (same ldc / batch strides, in elements) */
  const float* bias;
  int64_t bias_bs;
  float alpha, out_scale, r1_scale;
  int32_t r1_mod;
  const float* colscale;
  const float* rowscale;
  const float* R1;
  int64_t ldr1;
  const float* R2;
  int64_t ldr2;
  const int32_t* feat_len; /* ACT_FEAT key masking (fast_attention.py:69-74) */
  int32_t feat_S, feat_rpt, feat_kslot;
  int32_t precision; /* 1 single pass, 3 bf16x3; 2 = single pass with fp16 operands (sets h16) */
  int32_t h16;       /* MDM_H16_*: format of BF16_ROW activation / weight planes in the single-pass kernels and of C16 */
  /* fp8 GEMM (A.kind == W.kind == MDM_OP_FP8_ROW): acc * a_scale_u * a_scale[src row of m] * w_scale[n] (+ bias, act, ...) */
  const float* a_scale; /* per activation row (indexed by the GATHERED source row), or NULL */
  const float* w_scale; /* per output channel; grouped like bias (bias_bs), or NULL */
  float a_scale_u;      /* uniform activation scale (1 by default) */
  uint8_t* C8;          /* optional fp8 output e4m3(v * c8_scale), same ldc */
  float c8_scale;
  /* weight-gradient mode (both operands MDM_OP_F32_KSTRIDE, no goff): batch z reduces over the K range
   * [kgoff[z], kgoff[z+1]) -- the routed rows of expert group z -- instead of [0, K); an empty range writes epilogue(0) */
  const int32_t* kgoff;
  /* MDM_ACT_HEADNORM: LayerNorm weight / bias over head_dim = 128, number of leading 128-column slices that are also
   * L2-normalised (2 H for q | k | v), and the lo plane of the output (C16 = hi plane; hi + lo = the fp32 value to ~2^-17).
   * C16_lo with MDM_ACT_NONE / HEADSOFTMAX on the fp32-grade kernel: the result leaves as bf16 hi / lo planes (C must be NULL) */
  const float* hn_w;
  const float* hn_b;
  uint16_t* C16_lo;
  int32_t hn_l2_tiles;
  /* fp32-grade kernel: the result as MDM_OP_X2_ROW rows (row stride 2 * ldc 16-bit elements; N % 32 == 0, ldc % 4 == 0), beside or
   * instead of C.  Must be 16-byte aligned (each lane stores 16 bytes): otherwise mdm_gemm returns MDM_ERR_UNSUPPORTED */
  uint16_t* Cx2;
  /* optional fragment stream of W (mdm_gemm_stream1_pack, format h16): a plain Linear on 16-bit rows (precision 1 / 2, no batch /
   * groups / gather, act NONE or GELU, N % 256 == K % 256 == 0) then runs on the streamed-weight kernel (csrc/gemm_stream.hip);
   * anything else ignores it */
  const uint16_t* w_stream;
  /* fp32-grade mode (precision 3) with MDM_OP_X2_ROW activations: w_stream = the (bf16 hi, lo) fragment-pair stream of W
   * (mdm_gemm_stream3x_pack; K in {512, 1024}, N % 512 == 0) selects the streamed-weight bf16x3 kernel (csrc/gemm_stream3.hip);
   * grouped launches (goff) give the stream's elements per group (mdm_gemm_stream3x_elems(1, N, K) minus the tail pad) here */
  int64_t w_stream_gs;
} MdmGemmDesc;

int mdm_gemm(const MdmGemmDesc* desc, void* stream);

/* Fused two-layer MLP (throughput mode, bf16 operands, fp32 accumulation):
 *   Y[m,:] = ( GELU(X[src(m),:] W1^T + b1) W2^T + b2 ) * rowscale[m] + r1_scale * R1[m,:] + R2[m,:]
 * the hidden activations stay on chip.  Replaces the Linear-GELU-Linear pairs of the path: the expert MLPs
 * (switch_moe.py:19-25, grouped by goff with per-expert strides w?_gs / b?_gs), the 4x FFN of the text cross-attention
 * block (fast_attention.py:293-299) and the Performer output projection (fast_attention.py:121-126).
 * Supported shapes: Dout == 512, Din % 64 == 0, F % 256 == 0 (LDS-staged kernel); with a weight stream (below) Dout == 512 and
 * Din in {128, 256, 512}, or Dout == Din == 1024; anything else returns MDM_ERR_UNSUPPORTED.
 * Both kernels move 16 bytes per lane: X, C, R1, R2, b1, b2 must be 16-byte aligned (C16 8-byte), ldx a multiple of 8, ldc / ldr1 /
 * ldr2 and b1_gs / b2_gs multiples of 4; otherwise MDM_ERR_UNSUPPORTED before any launch, and nothing is written. */
typedef struct MdmMlpDesc {
  const uint16_t* X; /* bf16 rows [*, Din] */
  int64_t ldx;
  const int32_t* gather; /* optional: row m reads X[gather[m]] */
  int32_t M, Din, F, Dout;
  const int32_t* goff;
  int32_t ngroups;
  const uint16_t* w1; /* bf16 [F, Din] (row stride ldw1) */
  int64_t ldw1, w1_gs;
  const float* b1;
  int64_t b1_gs;
  const uint16_t* w2; /* bf16 [Dout, F] (row stride ldw2) */
  int64_t ldw2, w2_gs;
  const float* b2;
  int64_t b2_gs;
  const float* rowscale;
  const float* R1;
  int64_t ldr1;
  float r1_scale;
  const float* R2;
  int64_t ldr2;
  float* C;      /* fp32 output (may be NULL when C16 is set) */
  uint16_t* C16; /* optional 16-bit copy */
  int64_t ldc;
  int32_t h16;   /* MDM_H16_*: format of X, w1, w2 and C16 (0 = bf16) */
  /* optional weight STREAM built by mdm_mlp_stream_pack from the same w1 / w2 (same 16-bit format): per (group, wave) one
   * linear run of 1-KiB MFMA fragments in consumption order (csrc/mlp_stream.hip).  When set and the shape is one of the
   * streamed kernel's (above; F % 256 == 0, ngroups <= 64) that kernel runs and w1 / w2 are not read; wstream_gs = elements
   * per group = F * Din + Dout * F.  The buffer must have mdm_mlp_stream_elems() elements (16 KiB of tail padding). */
  const uint16_t* wstream;
  int64_t wstream_gs;
} MdmMlpDesc;

int mdm_fused_mlp(const MdmMlpDesc* desc, void* stream);
/* Weight stream of the fused MLP: elements the buffer needs, and the packer (fp32 row-major w1 [G, F, Din], w2 [G, Dout, F]
 * -> h16-format stream; once at load time). */
int64_t mdm_mlp_stream_elems(int32_t G, int32_t F, int32_t Din, int32_t Dout);
int mdm_mlp_stream_pack(const float* w1, const float* w2, int32_t G, int32_t F, int32_t Din, int32_t Dout, int32_t h16,
                        uint16_t* out, void* stream);
/* Weight stream of ONE Linear [N, K] fp32 for the fused stylization kernel (csrc/style_gemm.hip; N = K = 512): elements
 * the buffer needs (0 = shape not taken) and the packer. */
int64_t mdm_gemm_stream_elems(int32_t N, int32_t K);
int mdm_gemm_stream_pack(const float* w, int32_t N, int32_t K, int32_t h16, uint16_t* out, void* stream);
/* Fragment stream of a [N, K] fp32 weight for the streamed-weight GEMM (MdmGemmDesc.w_stream / MdmPacked.ws): [N / 16][K / 32]
 * MFMA operand fragments of 1 KiB in the 16-bit format h16, plus the read-ahead pad.  elems: 16-bit elements to allocate, 0 when the
 * shape is not covered (N % 256, K % 256). */
int64_t mdm_gemm_stream1_elems(int32_t N, int32_t K);
/* ... and of G stacked [N, K] fp32 weights (the experts of one layer) as (bf16 hi, lo) fragment PAIRS for the streamed-weight
 * bf16x3 GEMM (MdmGemmDesc.w_stream with MDM_OP_X2_ROW activations); group_elems = the stride between groups (w_stream_gs) */
int64_t mdm_gemm_stream3x_elems(int32_t G, int32_t N, int32_t K);
int64_t mdm_gemm_stream3x_group_elems(int32_t N, int32_t K);
int mdm_gemm_stream3x_pack(const float* w, int64_t ldw, int32_t G, int32_t N, int32_t K, uint16_t* out, void* stream);
int mdm_gemm_stream1_pack(const float* w, int64_t ldw, int32_t N, int32_t K, int32_t h16, uint16_t* out, void* stream);

/* the same for the fp32-grade (bf16x3) form of that kernel: (bf16 hi, lo = rn(w - hi)) fragment PAIRS in consumption order,
 * 2 * N * K + 16 KiB of tail padding elements (0 = shape not taken) */
int64_t mdm_gemm_stream3_elems(int32_t N, int32_t K);
int mdm_gemm_stream3_pack(const float* w, int32_t N, int32_t K, uint16_t* out, void* stream);

/* fp32 [rows, K] (row stride ld_src) -> bf16 planes [rows, Kpad] (Kpad = ld_dst, multiple of 32, zero padded);
 * lo may be NULL.  Weight packing happens once at load time (not on the hot path). */
int mdm_pack_bf16(const float* src, int64_t ld_src, int64_t rows, int64_t K, uint16_t* hi, uint16_t* lo,
                  int64_t ld_dst, void* stream);
/* fp32 [rows, K] -> e4m3 bytes [rows, ld_dst] (ld_dst multiple of 128, zero padded) + scales[rows] = amax / 448 */
int mdm_pack_fp8(const float* src, int64_t ld_src, int64_t rows, int64_t K, uint8_t* dst, int64_t ld_dst, float* scales,
                 void* stream);
/* same layout, one IEEE fp16 plane (MDM_H16_F16 weights of the single-pass kernels) */
int mdm_pack_f16(const float* src, int64_t ld_src, int64_t rows, int64_t K, uint16_t* dst, int64_t ld_dst, void* stream);

/* ---- packed weights of one denoiser (built once at load time by motiondiffusion-moe_amd/packing.py) ------------ */
typedef struct MdmPacked { /* 16-bit planes of an fp32 [N,K] weight, K padded to ld (multiple of 32) */
  const uint16_t* hi; /* bf16 hi plane, or the fp16 plane of a weight packed for a single fp16 pass */
  const uint16_t* lo; /* bf16 lo plane (bf16x3); for an fp8-packed weight (hi = e4m3 bytes): its per-row fp32 scales; else NULL */
  int64_t ld;
  const uint16_t* ws; /* optional fragment stream of the same weight in the model's 16-bit format (mdm_gemm_stream1_pack), or NULL */
} MdmPacked;

typedef struct MdmStyle { /* StylizationBlock minus its emb_layers (those are stacked model-wide), stylization.py:5-31 */
  const float *norm_w, *norm_b;
  MdmPacked out; /* out_layers.2 [D,D] */
  const float* out_b;
  const uint16_t* out_ws; /* optional weight stream of out_layers.2 (mdm_gemm_stream_pack; 16-bit modes, D == 512), or NULL */
  const uint16_t* out_ws3; /* optional (hi, lo) pair stream of out_layers.2 (mdm_gemm_stream3_pack; fp32-grade modes, D == 512), or NULL */
} MdmStyle;

typedef struct MdmPerformer { /* PerformerSelfAttention, fast_attention.py:94-179 */
  const float *pre_w, *pre_b, *post_w, *post_b;
  MdmPacked qkv; /* query|key|value stacked [3D, D] (fast_attention.py:145-147) */
  const float* qkv_b;
  const float *hn_w, *hn_b; /* fast_attention.norm over head_dim */
  MdmPacked feat;           /* projection_matrix^T [m, dh] (captured random state, fast_attention.py:19-36) */
  MdmPacked proj0, proj3;
  const float *proj0_b, *proj3_b;
  const uint16_t* proj_ws; /* optional weight stream of proj_out.0 / proj_out.3 (mdm_mlp_stream_pack, G = 1), or NULL */
  MdmStyle style;
} MdmPerformer;

typedef struct MdmLayer { /* MoEExtendedDecoderLayer, transformer.py:17-64 */
  const float *dual_pre_w, *dual_pre_b, *dual_post_w, *dual_post_b;
  MdmPerformer local, global;
  MdmPacked skip;
  const float* skip_b;
  /* GatedCrossAttention / LinearTemporalCrossAttention, fast_attention.py:227-272 */
  const float *ca_norm_w, *ca_norm_b, *ca_tnorm_w, *ca_tnorm_b;
  MdmPacked ca_q, ca_k, ca_v;
  const float *ca_q_b, *ca_k_b, *ca_v_b;
  const float* ca_gvec; /* sigmoid(gate) * sigmoid(adaptive_gate), [D] */
  MdmStyle ca_style;
  /* MoEMultiBranchFFN / SwitchMoELayer, multi_branch.py:31-61, switch_moe.py:7-111; experts stacked branch-major */
  const float *moe_ln_w[2], *moe_ln_b[2], *gate_w[2], *gate_b[2];
  MdmPacked w1; /* [2*E*F, D] */
  MdmPacked w2; /* [2*E*D, F] */
  const uint16_t* wstream;   /* optional weight stream of the 2E expert MLPs (mdm_mlp_stream_pack; 16-bit expert modes), or NULL */
  int64_t wstream_gs;        /* elements per expert group: F * D + D * F */
  const float *b1, *b2;
  float *usage[2], *importance[2]; /* expert_usage / expert_importance buffers, updated in place; may be NULL */
  MdmStyle ffn_style;
  /* MemoryEfficientCrossAttentionBlock, fast_attention.py:274-330 */
  MdmPacked sd_q, sd_k, sd_v, sd_out, sd_f1, sd_f2;
  const float *sd_q_b, *sd_k_b, *sd_v_b, *sd_out_b, *sd_ln_w, *sd_ln_b, *sd_f1_b, *sd_f2_b;
  /* optional fp32 copies of sd_cross_attn.query / .out weights [D, D]: needed only to build the folded text cache */
  const float *sd_q_w32, *sd_out_w32;
  const uint16_t* sd_ffn_ws; /* optional weight stream of sd_cross_attn.ffn.1 / .3 (mdm_mlp_stream_pack, G = 1), or NULL */
} MdmLayer;

typedef struct MdmModel { /* MotionTransformer, transformer.py:166-361 */
  int32_t D, F, Dt, H, E, L, feats, num_frames;
  MdmPacked tmlp0, tmlp2, te0, te2, tproj, gf_time, gf_text, gf_post0, gf_post2, text_proj, joint, down, up, out;
  const float *tmlp0_b, *tmlp2_b, *te0_b, *te2_b, *tproj_b, *gf_time_b, *gf_text_b, *gf_post0_b, *gf_post2_b,
      *text_proj_b, *joint_b, *down_b, *up_b2, *out_b;
  const float* seq_emb;  /* [num_frames, D] */
  MdmPacked style_eph;   /* the 8L per-call random emb projections stacked [8L*Te, D] (stylization.py:22-24) */
  const float* style_eph_b;
  MdmPacked style_emb;   /* emb_layers.1 of the 8L StylizationBlocks stacked [8L*2D, Te] */
  const float* style_emb_b;
  const MdmLayer* layers; /* 2L entries: low blocks then high blocks; style slot of layer i = 4*i + {local,global,cross,ffn} */
} MdmModel;

/* x/t-independent text-side state, one slab per decoder layer (2L of them) */
typedef struct MdmTextCache {
  float* lin_at; /* [2L, B, H, dh, dh]  A^T of fast_attention.py:252 */
  float* sd_k;   /* [2L, B, N, D]       key(xf)   of fast_attention.py:306 */
  float* sd_v;   /* [2L, B, N, D]       value(xf) of fast_attention.py:307 */
  int32_t B, N;
  /* optional (all three or none; throughput mode, D == 512, H * N <= 128): the query / output projections of the text
   * cross-attention folded into the text side, see csrc/sdfold.hip.  Zero-initialised by the caller (padding). */
  uint16_t* sd_kfold; /* 16-bit [2L, B, P, 128, D]  K'[hs*N + n, :] = key_h[n, :] Wq_h / sqrt(dh); P = mdm_sd_fold_passes, hs = h mod heads-per-pass */
  float* sd_cb;       /* fp32   [2L, B, P, 128]     key_h[n, :] . bq_h / sqrt(dh) */
  uint16_t* sd_vfold; /* 16-bit [2L, B, P, D, 128]  V'^T[:, hs*N + n] = Wout[:, h] value_h[n, :]^T */
  /* optional int32 [B] on the device, 1 <= ntok[b] <= N: sample b's own text token count; rows ntok[b] .. N-1 of its xf_out
   * are padding that neither cross-attention sees (weight exactly 0 in both softmaxes).  NULL = every sample has N tokens.
   * The reference has no text mask (fast_attention.py:249,317-320): this exists so that forwards the reference runs
   * separately because their captions tokenise to different lengths -- the cond and uncond halves of a guided step,
   * gaussian_diffusion.py:1060-1073 -- can travel as rows of one batch and still see exactly their own tokens. */
  const int32_t* ntok;
} MdmTextCache;

/* Optional per-loop stem cache: the time-embedding chain (time.py:15-31 -> time_embed -> time_proj -> gated_fusion.proj_time,
 * transformer.py:318-320, gate.py:16) depends only on the integer timestep, and gated_fusion.proj_text(text_proj(xf_proj))
 * only on the text: both are tabulated once per sampling loop instead of being recomputed by 8 tiny GEMMs every step. */
typedef struct MdmStemCache {
  const float* time_table; /* [steps, D], row t = proj_time(...(t)) */
  const float* gx;         /* [B, D] = proj_text(text_proj(xf_proj)) */
  int32_t steps;
} MdmStemCache;

/* Fill time_table [steps, D] (t = 0..steps-1) and gx [B, D]; either output may be NULL.  ws as for (B=128, T=2, N=1). */
int mdm_stem_cache_build(const MdmModel* m, int32_t steps, float* time_table, const float* xf_proj, int32_t B, float* gx,
                         void* ws, int64_t ws_bytes, int32_t precision, void* stream);

/* Bytes of scratch mdm_denoiser_forward / the block entry points need for (B, T, N). */
int64_t mdm_workspace_bytes(const MdmModel* m, int32_t B, int32_t T, int32_t N);

/* Build the text cache from xf_out [B, N, Dt] (hoists fast_attention.py:249-252,306-307 out of the step loop). */
int mdm_text_cache_build(const MdmModel* m, const float* xf_out, const MdmTextCache* tc, void* ws, int64_t ws_bytes,
                         int32_t precision, void* stream);

/* MotionTransformer.forward (transformer.py:291-361) with text already encoded:
 * x [B,T,feats], timesteps int64 [B], length int32 [B], xf_proj [B,Dt] -> out [B,T,feats].
 * forced_routing: NULL, or int32 [2L][2][B*S_layer][2] expert indices (parity tests); trace: NULL or per-block dumps;
 * stem: NULL or a cache built by mdm_stem_cache_build for integer timesteps in [0, steps). */
int mdm_denoiser_forward(const MdmModel* m, const MdmTextCache* tc, const float* x, const int64_t* timesteps,
                         const int32_t* length, const float* xf_proj, int32_t B, int32_t T, float* out, void* ws,
                         int64_t ws_bytes, const int32_t* forced_routing, float* trace, const MdmStemCache* stem,
                         int32_t precision, void* stream);

/* One decoder layer / its four blocks on h [B,S,D] in place semantics (out may alias nothing);
 * sc = the layer's 4 style (scale|shift) rows [4, B, 2D]; len int32 [B] (already halved for the low scale). */
enum { MDM_BLOCK_DUAL = 0, MDM_BLOCK_CROSS = 1, MDM_BLOCK_MOE = 2, MDM_BLOCK_SDCROSS = 3, MDM_BLOCK_LAYER = 4 };
int mdm_block_forward(const MdmModel* m, int32_t layer, int32_t block, const MdmTextCache* tc, const float* h,
                      const float* sc, const int32_t* len, int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes,
                      const int32_t* forced_routing, int32_t precision, void* stream);

/* The same blocks under the names SURVEY.md 8(b) lists (thin views of mdm_block_forward; sc4 = the layer's four
 * (scale|shift) rows [4, B, 2D] as above), plus one PerformerSelfAttention alone (fast_attention.py:137-179; which = 0
 * local_attn, 1 global_attn; sc = that block's (scale|shift) rows [B, 2D]; out = x + 0.1 * style(...)). */
int mdm_moe_ffn_forward(const MdmModel* m, int32_t layer, const float* h, const float* sc4, const int32_t* len, int32_t B,
                        int32_t S, float* out, void* ws, int64_t ws_bytes, const int32_t* forced_routing,
                        int32_t precision, void* stream);
int mdm_dual_self_attn_forward(const MdmModel* m, int32_t layer, const float* h, const float* sc4, const int32_t* len,
                               int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes, int32_t precision,
                               void* stream);
int mdm_linear_xattn_forward(const MdmModel* m, int32_t layer, const MdmTextCache* tc, const float* h, const float* sc4,
                             const int32_t* len, int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes,
                             int32_t precision, void* stream);
int mdm_softmax_xattn_ffn_forward(const MdmModel* m, int32_t layer, const MdmTextCache* tc, const float* h,
                                  const float* sc4, const int32_t* len, int32_t B, int32_t S, float* out, void* ws,
                                  int64_t ws_bytes, int32_t precision, void* stream);
int mdm_performer_attn_forward(const MdmModel* m, int32_t layer, int32_t which, const float* h, const float* sc,
                               const int32_t* len, int32_t B, int32_t S, float* out, void* ws, int64_t ws_bytes,
                               int32_t precision, void* stream);

/* StylizationBlock.forward given (scale|shift) = emb_layers(emb): out = Lin(SiLU(LN(h)*(1+scale)+shift)) */
int mdm_stylization_forward(const MdmStyle* st, const float* h, const float* sc, int32_t B, int32_t S, int32_t D,
                            float* tmp, float* out, int32_t precision, void* stream);

/* Stem: fused time/text embedding (transformer.py:313-321) and all 8L stylization (scale|shift) rows.
 * emb_out [B,D] (may be NULL), sc_out [8L, B, 2D]. */
int mdm_stem_embeddings(const MdmModel* m, const int64_t* timesteps, const float* xf_proj, int32_t B, float* emb_out,
                        float* sc_out, void* ws, int64_t ws_bytes, int32_t precision, void* stream);

/* Sampler updates on n = B*T*feats elements.  tab = fp32 schedule table [7][steps] with rows
 * sqrt_recip_acp, sqrt_recipm1_acp, coef1, coef2, post_logvar_clipped, acp, acp_prev
 * (gaussian_diffusion.py:405-431); t from *t_dev when non-NULL else t_imm.
 * CFG DDPM step (gaussian_diffusion.py:1042-1098; eps_u NULL = unguided p_sample :582-614; noise NULL = no noise;
 * clip_denoised clamps each pred_xstart to [-1,1] before guidance, :523-528). */
int mdm_cfg_posterior_step(const float* x, const float* eps_c, const float* eps_u, const float* noise, int64_t n,
                           const float* tab, int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale,
                           int32_t clip_denoised, float* x_out, float* x0_out, void* stream);
/* DDIM step (gaussian_diffusion.py:699-742). */
int mdm_ddim_step(const float* x, const float* eps, const float* noise, int64_t n, const float* tab, int32_t steps,
                  const int32_t* t_dev, int32_t t_imm, float eta, int32_t clip_denoised, float* x_out, float* x0_out,
                  void* stream);

/* Few-step samplers on a respaced schedule (csrc/solver.hip).  t = *t_dev when non-NULL else t_imm, an index into the
 * SPACED schedule of `steps` entries.
 * dst[r] = map[clamp(t, 0, steps-1)] for r < n: the original timestep of the spaced step, for the denoiser.
 * Guided update: x0_c = tab[0][t]*x - tab[1][t]*eps_c and x0_u likewise from eps_u, each clamped to [-1,1] when
 * clip_denoised; x0 = x0_u + cfg_scale*(x0_c - x0_u) (eps_u NULL = unguided, x0 = x0_c); then
 * x_out = cx*x + c0*x0 + c1*x0_prev + cn*noise and x0_out = x0, with {cx, c0, c1, cn} = coef[t][0..3] (fp32 [steps][4]).
 * x0_prev NULL or c1 == 0: no x0_prev term and no read; noise NULL: no noise term; x0_out may be NULL.  x_out may be x
 * and x0_out may be x0_prev (in place).  Guided DDIM at any eta and DPM-Solver++(2M) differ only in coef. */
int mdm_fill_timesteps_mapped(int64_t* dst, int64_t n, const int32_t* t_dev, const int64_t* map, int32_t steps,
                              void* stream);
int mdm_guided_update(const float* x, const float* eps_c, const float* eps_u, const float* x0_prev, const float* noise,
                      int64_t n, const float* tab, const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm,
                      float cfg_scale, int32_t clip_denoised, float* x_out, float* x0_out, void* stream);
/* Motion editing: mdm_guided_update with the guided x0 replaced by (1 - mask)*x0 + mask*known before the update, so
 * x_out uses that x0 and x0_out receives it.  known (normalised motion, never clamped) and mask (in [0, 1]) are dense [n];
 * NULL is an argument error.  mask = 0 gives exactly the x0 of mdm_guided_update, mask = 1 exactly known. */
int mdm_guided_update_inpaint(const float* x, const float* eps_c, const float* eps_u, const float* x0_prev,
                              const float* noise, const float* known, const float* mask, int64_t n, const float* tab,
                              const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale,
                              int32_t clip_denoised, float* x_out, float* x0_out, void* stream);
/* Composed guidance: nconds = K prompts per sample.  eps is [(K + 1) * n]: the K condition blocks in order, then the
 * unconditional block; weights is [K * n], condition-major (block k = w_k).  With x0_k and x0_u as in mdm_guided_update
 * (each clamped when clip_denoised): x0 = x0_u + cfg_scale * sum_k w_k (x0_k - x0_u), then, when known and mask are both
 * set, x0 = (1 - mask)*x0 + mask*known, then x_out = cx*x + c0*x0 + c1*x0_prev + cn*noise and x0_out = x0 as above.
 * K = 1 with weights 1 equals mdm_guided_update (known / mask NULL) and mdm_guided_update_inpaint bit for bit.
 * MDM_ERR_ARG: K outside [1, MDM_COMPOSE_MAX_K], only one of known / mask, or the checks of mdm_guided_update. */
enum { MDM_COMPOSE_MAX_K = 8 };
int mdm_composed_update(const float* x, const float* eps, int32_t nconds, const float* weights, const float* x0_prev,
                        const float* noise, const float* known, const float* mask, int64_t n, const float* tab,
                        const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale,
                        int32_t clip_denoised, float* x_out, float* x0_out, void* stream);

/* Counter-based gaussian noise (Philox4x32-10 + Box-Muller, csrc/noise.hip): out[s, e] for s < nsamples, e < per_sample is
 * a function of (seed, sample0 + s, stream, e) only, where stream = *stream_dev when non-NULL (the device-resident timestep
 * of a captured step) else stream_imm (MDM_NOISE_STREAM_XT for the initial x_T).  Replaces th.randn(*shape) /
 * th.randn_like(x) of gaussian_diffusion.py:1119,1094 where results must not depend on how the batch is sharded. */
enum { MDM_NOISE_STREAM_XT = 0x7fffffff };
int mdm_noise_normal(float* out, int64_t per_sample, int32_t nsamples, int64_t sample0, uint64_t seed,
                     const int32_t* stream_dev, int32_t stream_imm, void* stream);
/* the same with one explicit global sample index per row (device int64 [nsamples]): length-bucketed batches whose rows are
 * not consecutive samples (trainer.generate_bucketed) */
int mdm_noise_normal_ids(float* out, int64_t per_sample, int32_t nsamples, const int64_t* sample_ids, uint64_t seed,
                         const int32_t* stream_dev, int32_t stream_imm, void* stream);
/* Forward diffusion of a given motion to an intermediate level of the schedule, the start of a partial sampling loop
 * (csrc/noise.hip): out[r, e] = a * x_start[r, e] + s * n[r, e] for r < nsamples, e < per_sample.
 * n is read from noise when it is non-NULL; otherwise it is drawn in registers and equals what mdm_noise_normal (sample_ids
 * NULL: global sample sample0 + r) or mdm_noise_normal_ids (global sample sample_ids[r]) writes under seed on the
 * MDM_NOISE_STREAM_XT stream.  a = sqrt(abar) and s = sqrt(1 - abar) of the level, evaluated in f64 on the host and rounded
 * once.  out may be x_start.  MDM_ERR_ARG: NULL x_start or out, a negative size or sample0, a or s not finite. */
int mdm_diffuse_start(const float* x_start, const float* noise, float* out, int64_t per_sample, int32_t nsamples,
                      int64_t sample0, const int64_t* sample_ids, uint64_t seed, float a, float s, void* stream);

/* Text projection head of the reference's EnhancedTextEncoder (text_encoder.py:13-18,31-43), applied to the
 * last_hidden_state of any text encoder (the DeBERTa weights themselves are third-party and stay outside this library):
 *   projected[b] = GELU(Linear(LayerNorm(cat(prompt_tokens, hidden[b]))))   (B, P + N0, Dt) -> xf_out
 *   pooled[b]    = mean over the P + N0 tokens of projected[b]              (B, Dt)         -> xf_proj
 * hidden fp32 (B, N0, Hs), prompts fp32 (P, Hs), Hs <= 1024.  ws >= mdm_text_head_workspace_bytes(...). */
int64_t mdm_text_head_workspace_bytes(int32_t B, int32_t N0, int32_t P, int32_t Hs, int32_t Dt);
int mdm_text_head_forward(const float* hidden, const float* prompts, const float* ln_w, const float* ln_b,
                          const MdmPacked* w, const float* bias, int32_t B, int32_t N0, int32_t P, int32_t Hs,
                          int32_t Dt, float* xf_out, float* xf_proj, void* ws, int64_t ws_bytes, int32_t precision,
                          void* stream);

/* Post-processing of generated motions on the device (tools/visualization.py:21-27,89): de-normalise (x * std + mean),
 * recover_from_ric (utils/motion_process.py:362-416: root rotation / translation by prefix sums, joints rotated back by
 * the inverse root rotation) and the temporal gaussian filter of motion_temporal_filter (utils/utils.py:125-130).
 * motion (B, T, feats) fp32, length (B) int32 or NULL (= T), mean / std (feats).  weights[0..radius]: the normalised
 * gaussian taps w[k] = w[-k] as fp64 (radius 0 = no filter).  scratch and joints_out: (B, T, joints, 3) fp32; frames
 * past a sample's length are written as zeros. */
int mdm_motion_postprocess(const float* motion, const int32_t* length, const float* mean, const float* std, int32_t B,
                           int32_t T, int32_t feats, int32_t joints, int32_t radius, const double* weights,
                           float* scratch, float* joints_out, void* stream);

/* Joints -> feature rows on the device (csrc/motion_features.hip): the inverse of mdm_motion_postprocess,
 * restating utils/motion_process.py process_file / extract_features.  The skeleton is data: parent-ordered kinematic chains
 * (chain c is chain_joints[chain_offsets[c] .. chain_offsets[c + 1]); it starts at joint 0 or at a joint an earlier chain
 * reached), one axis direction per bone (raw_offsets, (joints, 3)), the face joints in the reference's list order
 * (r_hip, l_hip, sdr_r, sdr_l), the four foot joints in contact-column order and the two leg joints whose bone lengths give
 * the uniform skeleton's scale.  A host struct, checked before the launch (every index inside [0, joints)). */
enum { MDM_SKEL_MAX_JOINTS = 32, MDM_SKEL_MAX_CHAINS = 8, MDM_SKEL_MAX_CHAIN_ENTRIES = 48 };
typedef struct {
  int32_t joints, nchains;
  int32_t chain_offsets[MDM_SKEL_MAX_CHAINS + 1];
  int32_t chain_joints[MDM_SKEL_MAX_CHAIN_ENTRIES];
  float raw_offsets[MDM_SKEL_MAX_JOINTS * 3];
  int32_t face[4], feet[4], legs[2];
} MdmSkeleton;
/* joints (B, T, J, 3) fp32, length (B) int32 or NULL (= T), mean / std (F = 12 J - 1) or both NULL (rows not normalised).
 * features_out (B, T - 1, F): a clip of n frames gives n - 1 rows (the last frame only supplies velocities); rows at or past
 * length[b] - 1 are zero.  canonicalize != 0: the clip is first put on the floor, frame 0's root XZ moved to the origin and
 * frame 0 turned to face Z+; with target_offsets (J, 3) it is before that re-posed on those bone offsets (uniform_skeleton).
 * The canonical positions go to positions_out (B, T, J, 3), which is then required (frames past the length zero).
 * canonicalize == 0: the joints are taken as they are, positions_out is not touched and target_offsets must be NULL.
 * weights[0..radius]: fp64 taps of the facing-direction filter (sigma 20: radius 80), as for mdm_motion_postprocess.
 * feet_thre: squared displacement per frame under which a foot joint is in contact.
 * MDM_ERR_ARG: a null pointer, T < 2, a malformed skeleton; MDM_ERR_UNSUPPORTED: T > mdm_motion_features_max_frames(). */
int mdm_motion_features_max_frames(void);
int mdm_motion_features(const float* joints, const int32_t* length, const float* mean, const float* std,
                        const MdmSkeleton* skeleton, const float* target_offsets, int32_t B, int32_t T, double feet_thre,
                        int32_t canonicalize, int32_t radius, const double* weights, float* positions_out,
                        float* features_out, void* stream);

/* Joints from rotations (csrc/motion_fk.hip): recover_from_rot of utils/motion_process.py:384-398 on normalised
 * rows.  motion (B, T, F) fp32 with F = 12 joints - 1 (263 t2m, 251 KIT), length (B) int32 or NULL (= T), mean / std (F):
 * de-normalise, recover the root heading and XZ path exactly as mdm_motion_postprocess, turn the root quaternion and the rot6d
 * columns 4 + 3 (J - 1) .. of joints 1 .. J - 1 into matrices (cont6d_to_matrix, no clamp and no epsilon: a zero-norm or
 * parallel pair gives non-finite joints down that frame's chain) and accumulate them down the skeleton's chains, every chain
 * from the ROOT matrix: R <- R M[c], joint[c] = R offset[c] + joint[previous].  offsets: (J, 3) shared by the batch
 * (offsets_per_sample == 0), (B, J, 3) (!= 0), or NULL: each sample's own, bone length = mean over its valid frames of the
 * bone's length on the recover_from_ric joints (summed in double in frame order) times the skeleton's raw_offsets axis.  The
 * offsets used go to offsets_out (B, J, 3) when non-NULL.  joints_out (B, T, J, 3); rotations_out (B, T, J, 3, 3) or NULL:
 * the accumulated global matrices, row-major, the root's at joint 0.  weights[0..radius]: temporal gaussian filter of the
 * joints (never of the rotations) as for mdm_motion_postprocess.  Frames at or past length[b] are zero in every output and
 * are never read.  scratch (B, T, J, 3) is needed when radius > 0 or offsets is NULL.  Of the skeleton, the chains and
 * raw_offsets are used.  MDM_ERR_ARG: a null pointer, T < 1, F != 12 joints - 1, a malformed skeleton (the check of
 * mdm_motion_features); MDM_ERR_UNSUPPORTED: T > mdm_motion_fk_max_frames() (20 bytes of LDS per frame). */
int mdm_motion_fk_max_frames(void);
int mdm_motion_fk(const float* motion, const int32_t* length, const float* mean, const float* std,
                  const MdmSkeleton* skeleton, const float* offsets, int32_t offsets_per_sample, int32_t B, int32_t T,
                  int32_t F, int32_t radius, const double* weights, float* scratch, float* joints_out,
                  float* rotations_out, float* offsets_out, void* stream);

/* Foot-skate clean-up (csrc/foot_skate.hip): pin planted feet with two-bone leg IK.  joints (B, T, J, 3) fp32,
 * length (B) int32 or NULL (= T).  Four contact labels per frame, in the order of skeleton->feet (ankle, toe, ankle, toe):
 * contact != NULL: label f of frame t of sample b is on iff contact[(b T + t) contact_stride + f] > contact_thre[f] (a host
 * array of 4; a (B, T, 4) tensor has stride 4, the contact columns of normalised rows (B, T, F) are read in place with
 * stride F from column F - 4 and thresholds (0.5 - mean) / std); contact == NULL: detected as mdm_motion_features has them,
 * frame t < n - 1 on iff the fp32 squared displacement of the joint to frame t + 1 is < feet_thre, frame n - 1 repeating
 * frame n - 2, none at n = 1.  A leg is hip, knee, ankle, toe: the last four entries of the chain that ends in feet[1] /
 * feet[3], whose entry before is feet[0] / feet[2].  Per foot joint and maximal run of frames with the label on, the anchor
 * is the joint's mean (X, Z) over the run (double, frame order, rounded once) and delta = anchor - p_xz inside the run; up
 * to `blend` frames outside, delta = (wL dL + wR dR) / max(1, wL + wR) of the nearest contact frame within `blend` on
 * either side, w = 1 - smoothstep(k / (blend + 1)).  The ankle goes to its target by two-bone IK with the hip fixed (reach
 * clamped to [|l1 - l2| (1 + 1e-4) + 1e-6, (l1 + l2) (1 - 1e-4)], the knee kept in its bend plane), the toe is aimed from
 * the new ankle at its own target on its own bone length.  Heights of the targets never change.  A (frame, leg) neither of
 * whose two labels is on or within `blend` of a run, and every other joint, is copied bit for bit.  rotations_in
 * (B, T, J, 3, 3), the layout of mdm_motion_fk's rotations_out, or NULL: rotations_out = Q R for knee, ankle and toe, Q the
 * shortest arc from the old bone to the new one (R copied where the bone keeps every bit); all others copied.  slide_out
 * (B, 2, 4) or NULL: per foot joint the mean |step in XZ| over the pairs of neighbouring frames that are both in contact,
 * before [0] and after [1] (double, frame order; 0 without a pair); pairs_out (B, 4) int32 or NULL: the pair counts.
 * scratch: (B, T, 4, 2) fp32.  Frames at or past length[b] are zero in every output and are never read.  Nothing is
 * updated in place: joints_out != joints, rotations_out != rotations_in.
 * MDM_ERR_ARG: a null required pointer (joints, skeleton, joints_out, scratch; contact_thre with contact), T < 1, blend < 0,
 * contact_stride < 4, feet_thre not >= 0 when detecting, a malformed skeleton or leg, rotations_in without rotations_out or
 * the reverse, an output that is its input; MDM_ERR_UNSUPPORTED: T > mdm_foot_skate_max_frames() (5 bytes of LDS per frame). */
int mdm_foot_skate_max_frames(void);
int mdm_foot_skate(const float* joints, const int32_t* length, const MdmSkeleton* skeleton, const float* contact,
                   int64_t contact_stride, const float* contact_thre, double feet_thre, int32_t blend, int32_t B, int32_t T,
                   const float* rotations_in, float* joints_out, float* rotations_out, float* slide_out, int32_t* pairs_out,
                   float* scratch, void* stream);

/* Exact reach (csrc/limb_pin.hip): pin the end joints of two-bone limbs to 3-D targets by limb IK.  joints,
 * targets and weights (B, T, J, 3) fp32 (targets and weights in the units and frame of joint control's), length (B) int32 or
 * NULL (= T).  limbs: a HOST array (L, 4) int32 of rows (root, mid, end, tip), 1 <= L <= 8, tip = -1 where the end joint has
 * no child.  Frame t < length[b] is a pin frame of a limb iff weights[b, t, end, c] > 0 for c = 0, 1, 2; targets are read
 * nowhere else, weights on other joints and their magnitudes do not matter.  In a pin frame delta = target[end] - p[end];
 * up to `blend` frames outside, delta = (wL dL + wR dR) / max(1, wL + wR) of the nearest pin frame within `blend` on either
 * side, w = 1 - smoothstep(k / (blend + 1)).  The end joint goes to end + delta by mdm_foot_skate's two-bone solve with the
 * limb root fixed (the same reach clamp, bend plane and fallbacks; out of reach the limb goes as far as it goes), the tip is
 * carried rigidly: tip' = end' + Q2 (tip - end), Q2 the shortest arc from the old mid -> end bone to the new one.  A
 * (frame, limb) that is neither a pin frame nor within `blend` of one, and every joint outside the limbs, is copied bit for
 * bit.  rotations_in (B, T, J, 3, 3), the layout of mdm_motion_fk's rotations_out, or NULL: rotations_out[mid] = Q1 R[mid]
 * (Q1 the shortest arc of the root -> mid bone), [end] = Q2 R[end], [tip] = Q2 R[tip]; all others copied.  error_out
 * (B, L, 4) or NULL: per limb over its pin frames the mean (double, frame order) and the maximum of |p[end] - target[end]|
 * before [0], [1] and after [2], [3] (0 without a pin frame); counts_out (B, L, 2) int32 or NULL: the pin frames and those of
 * them whose target lay outside the reach clamp.  scratch: (B, T, L, 3) fp32.  Frames at or past length[b] are zero in the
 * outputs and are never read.  Nothing is updated in place.
 * MDM_ERR_ARG: a null required pointer (joints, targets, weights, limbs, joints_out, scratch), T < 1, blend < 0, L outside
 * 1 .. 8, J outside 3 .. 32, a limb index out of range or repeated within a limb, a joint that two limbs move or that one
 * moves and another starts at, rotations_in without rotations_out or the reverse, an output that is an input;
 * MDM_ERR_UNSUPPORTED: T > mdm_limb_pin_max_frames() (9 bytes of LDS per frame). */
int mdm_limb_pin_max_frames(void);
int mdm_limb_pin(const float* joints, const int32_t* length, const float* targets, const float* weights,
                 const int32_t* limbs, int32_t L, int32_t J, int32_t blend, int32_t B, int32_t T, const float* rotations_in,
                 float* joints_out, float* rotations_out, float* error_out, int32_t* counts_out, float* scratch,
                 void* stream);

/* Rig export (csrc/motion_rig.hip): global rotations -> the channels of a node tree, retimed.  joints
 * (B, T, J, 3) and rotations (B, T, J, 3, 3) fp32 in the layout of mdm_motion_fk's outputs (R[c] orients the bone
 * parent(c) -> c), length (B) int32 or NULL (= T).  The node tree is three host arrays of n_nodes <= 64 entries, parents before
 * their nodes: parent[n] (the root's is -1, node 0 is the root) and carried[n], the joint whose R is the node's global rotation
 * G, or -1: G = the parent node's G (the identity at a root that carries nothing).  Output frame k < length_out[b] (device,
 * (B) int32, or NULL = T_out) lies at source time k den / num in integers: t0 = (k den) / num, frac = ((k den) % num) / num.  Per
 * node the local rotation G[parent]^T G[node] (the root: its G) at t0 and t0 + 1 -> unit quaternions, w >= 0 -> the second
 * flipped onto the first one's hemisphere -> slerp at frac (lerp where they nearly coincide) -> normalised -> matrix -> Euler
 * angles a, b, c of L = R_axis0(a) R_axis1(b) R_axis2(c), axes 0 / 1 / 2 = X / Y / Z, a permutation; where cos b is within
 * rounding of 0, c = 0 and a takes the rest.  channels_out (B, T_out, 3 + 3 n_nodes): scale * lerp(joint 0 at t0, t0 + 1; frac),
 * then a, b, c in degrees per node, in node order.  quaternions_out (B, T_out, n_nodes, 4) or NULL: the local (w, x, y, z).
 * Where frac == 0 frame t0 + 1 is not read and nothing is interpolated: at num == den the result is the frame's own rotation.
 * Output frames at or past length_out[b], or whose t0 is at or past length[b], are zero; source frames at or past length[b]
 * are never read.  Any T (no LDS).  MDM_ERR_ARG: a null pointer (length, length_out, quaternions_out excepted), T, J or T_out
 * < 1, n_nodes outside [1, 64], a parent not smaller than its node, a carried joint outside [-1, J), axes that are no
 * permutation, num or den < 1, (T_out - 1) den > (T - 1) num (the last output frame past the source). */
int mdm_rig_channels(const float* joints, const float* rotations, const int32_t* length, int32_t B, int32_t T, int32_t J,
                     int32_t n_nodes, const int32_t* parent, const int32_t* carried, int32_t axis0, int32_t axis1,
                     int32_t axis2, float scale, int32_t num, int32_t den, int32_t T_out, const int32_t* length_out,
                     float* channels_out, float* quaternions_out, void* stream);

/* Rig import (csrc/motion_rig_import.hip): the channel values of a BVH file -> joint positions at picked
 * nodes, retimed.  values (B, T, C) fp32 on the device: the MOTION rows, zero-padded to T frames; length (B) int32 or NULL (= T).
 * The node tables are host arrays, parents before their nodes: parent[n] (n_nodes <= 128; the root's is -1, node 0 is the
 * root), offsets (n_nodes, 3), rot_col / rot_axis (n_nodes, 3): the column and the axis (0 / 1 / 2 = X / Y / Z) of the node's
 * rotation channels in the order the file lists them, column -1 where it has fewer than three; pos_col[3]: the columns of the
 * root's X, Y, Z position, or -1; pick[n_pick] (n_pick <= 128): the nodes whose positions are wanted.  A node's local rotation
 * is L = R_axis0(v0) R_axis1(v1) R_axis2(v2) over its channels, angles in degrees, held as a unit quaternion with w >= 0.
 * Output frame k < length_out[b] (device, (B) int32, or NULL = T_out) lies at source time k den / num in integers, as in
 * mdm_rig_channels: where frac == 0 one frame is read and nothing is interpolated, otherwise the local quaternions at t0 and
 * t0 + 1 are slerped (the second flipped onto the first one's hemisphere, lerp where they nearly coincide) and the root's
 * position is lerped.  Position of a picked node j: p = OFFSET[j]; for each ancestor a up to the root p = OFFSET[a] + L[a] p;
 * at the root its position channels are added.  joints_out (B, T_out, n_pick, 3) = scale * basis * p, basis[9] a row-major
 * 3 x 3 host matrix.  quaternions_out (B, T_out, n_nodes, 4) or NULL: the retimed local (w, x, y, z) of every node.  Output
 * frames at or past length_out[b], or whose t0 is at or past length[b], are zero; source frames at or past length[b] are
 * never read.  Any T (no LDS).  MDM_ERR_ARG, before any launch: a null pointer (length, length_out, quaternions_out
 * excepted), T, T_out or C < 1, C > 32767, n_nodes or n_pick outside [1, 128], a parent not smaller than its node, a chain
 * deeper than 128, a column outside [-1, C), an axis outside 0..2, a pick outside [0, n_nodes), num or den < 1,
 * (T_out - 1) den > (T - 1) num (the last output frame past the source), quaternions_out not 16-byte aligned.
 * MDM_ERR_UNSUPPORTED: B T_out (n_pick + n_nodes) or (T_out - 1) den at or beyond 2^31 (the kernel counts in 32 bits). */
int mdm_rig_joints(const float* values, const int32_t* length, int32_t B, int32_t T, int32_t C, int32_t n_nodes,
                   const int32_t* parent, const float* offsets, const int32_t* rot_col, const int32_t* rot_axis,
                   const int32_t* pos_col, const int32_t* pick, int32_t n_pick, const float* basis, float scale, int32_t num,
                   int32_t den, int32_t T_out, const int32_t* length_out, float* joints_out, float* quaternions_out,
                   void* stream);

/* Rig retargeting (csrc/motion_retarget.hip): joints (B, T, J, 3), rotations (B, T, J, 3, 3) and offsets
 * (B, J, 3) fp32 in the layout of mdm_motion_fk's outputs -> the channels of a given hierarchy of n_nodes <= 128 nodes, retimed
 * as in mdm_rig_channels (the same integers, quaternions, slerp and Euler angles).  The target is one table of
 * mdm_retarget_table_words() 32-bit words that motion_rig.target_rig derives: tables_host is the host copy, which is checked,
 * tables_dev the same words on the device, which the kernels read.  Integers: [0] n_nodes, [1] J <= 32, [2] whether the legs
 * can take IK, [4 + 6 l ..] per leg the source's hip, knee and ankle joint and the target's thigh and shin node; then 16 per
 * node from word 16: parent, res (the nearest node at or above that has a rule, or -1), kind (0 none, 1 copy, 2 fit), src (the
 * joint whose R is copied; a fitted node's own joint), fa, fb (a = x[fa] - x[fb]), nb <= 8 and bj[8] (b = the sum of the unit
 * directions from x[src] to x[bj[.]]).  Floats from word 16 + 16 * 128: basis[9] row-major, the target's leg length, per leg l1,
 * l2 and the rest unit directions of thigh and shin (8 floats); then 12 per node from float 32: OFFSET[3] and M[9] row-major.
 * Launch 1 writes globals_out (B, T, n_nodes, 3, 3), the nodes' global rotations in the file's axes at the source frames: I
 * where res < 0, basis^T R[src] M for a copy, basis^T F(a, b) M for a fit (F: columns e1 = unit(a), e2 = e3 x e1, e3 =
 * unit(e1 x b); basis^T R[src] basis in a frame where a or e1 x b has no length), and with leg_ik = 1 thigh and shin turned by
 * the two-bone IK that puts the ankle node at s basis^T x[ankle], s = the target's leg length over the sample's (offsets).
 * Launch 2 writes channels_out (B, T_out, 3 + 3 n_nodes): s basis^T lerp(x[0]) - OFFSET[0], then per node the angles in
 * degrees of G[parent]^T G[node] in the order axis0, axis1, axis2.  Globals at or past length[b] and channels at or past
 * length_out[b] are zero; source frames at or past length[b] are never read.  Any T (no LDS).  MDM_ERR_ARG, before any launch: a
 * null pointer (length and length_out excepted), T or T_out < 1, num or den < 1, axes that are no permutation, leg_ik other than
 * 0 / 1 or 1 where the table has no legs, (T_out - 1) den > (T - 1) num, and a malformed table: n_nodes outside [1, 128], J
 * other than the table's or above 32, a parent not smaller than its node, a res, kind, joint or node index out of range, nb
 * outside [1, 8], a non-finite float, a leg length that is not > 0. */
int64_t mdm_retarget_table_words(void);
int mdm_retarget_channels(const float* joints, const float* rotations, const float* offsets, const int32_t* length, int32_t B,
                          int32_t T, int32_t J, const int32_t* tables_host, const int32_t* tables_dev, int32_t leg_ik,
                          int32_t axis0, int32_t axis1, int32_t axis2, int32_t num, int32_t den, int32_t T_out,
                          const int32_t* length_out, float* globals_out, float* channels_out, void* stream);

/* Linear blend skinning (csrc/motion_skin.hip): joints and global rotations move the vertices of a mesh.
 * joints (B, T, J, 3) and rotations (B, T, J, 3, 3) fp32 in the layout of mdm_motion_fk's outputs, length (B) int32 or NULL
 * (= T); parent[J], a host array (parent[0] is not read).  Bone 0 is the root: rotation R[0], pivot joint 0.  Bone c >= 1 is
 * the segment parent(c) -> c: rotation R[c], pivot joint parent(c).  The mesh, on the device: vertices (V, 3), or (B, V, 3)
 * with vertices_per_sample != 0; normals in the same shape, or NULL; bind_joints G (J, 3), or (B, J, 3) with bind_per_sample
 * != 0: the joints in the mesh's bind pose; bind_rotations Q (J, 3, 3) row-major or NULL (= identity): the bones' orientation
 * in the bind pose relative to the rest pose of the rotations; bone_index (V, 4) int32 and bone_weight (V, 4), shared by the
 * batch, the weights of a vertex summing to 1.  For t < length[b]:
 *   A_c(x) = P[t, pivot(c)] + R[t, c] Q[c]^T (x - G[pivot(c)])
 *   vertices_out[b, t, i] = sum_k w[i, k] A_{idx[i, k]}(v[i]), evaluated as v[i] + sum_k w[i, k] (A(v[i]) - v[i]): identity
 *   rotations with P = G give v[i] bit for bit;
 *   normals_out[b, t, i] = normalise(sum_k w[i, k] R[t, idx[i, k]] Q[idx[i, k]]^T n[i]), a zero sum staying zero.
 * vertices_out (B, T, V, 3); normals_out the same or NULL (it needs normals).  A slot of weight 0 contributes nothing and its
 * index is not used; a live index is clamped into [0, J).  Frames at or past length[b] are zero in both outputs and are never
 * read.  Every sample equals its own run alone bit for bit.  Any T and V: J <= 32 maps of 16 frames per workgroup in LDS, 64-bit
 * offsets into the outputs.  MDM_ERR_ARG: a null pointer (length, normals, bind_rotations, normals_out excepted), normals_out
 * without normals, T, J or V < 1, B < 0, a parent[c >= 1] outside [0, J) or equal to c.  MDM_ERR_UNSUPPORTED: J > 32, B or
 * T / 16 above 65535. */
int mdm_skin_vertices(const float* joints, const float* rotations, const int32_t* length, int32_t B, int32_t T, int32_t J,
                      const int32_t* parent, const float* vertices, const float* normals, int32_t V, int32_t vertices_per_sample,
                      const float* bind_joints, int32_t bind_per_sample, const float* bind_rotations, const int32_t* bone_index,
                      const float* bone_weight, float* vertices_out, float* normals_out, void* stream);

/* Motion preview (csrc/motion_render.hip): joints -> image frames.  joints (B, T, J, 3) fp32, length (B) int32 or
 * NULL (= T); of the skeleton the chains are used (group 2 + c draws the links of chain c) and J must be its joint count.
 * The image is defined in DESIGN.md §21: the scene of the reference's plot_3d_motion (floor rectangle from the clip's extent,
 * root trajectory up to the frame before, the chains) relative to the frame's root, a look-at pinhole camera, capsules and a
 * floor polygon with a one-pixel coverage ramp, groups composited once each in fp32, uint8 = floor(255 c + 0.5).
 * camera[8]: elevation and azimuth in degrees, distance, vertical field of view in degrees, target x, y, z, near plane.
 * style[3 + 5 (2 + nchains)]: the background's r, g, b, then r, g, b, alpha, full width in points (of a figure 720 points
 * high) of the floor (width unused), the trajectory and every chain, colours in [0, 1].  mode 0: out (B, NF, H, W, 3) uint8;
 * mode 1: out (B, NF, H, W) uint8, indices into the 6 x 7 x 6 colour cube (r6 42 + g7 6 + b6 of the 8-bit colour).
 * frames: device int32 [n_frames], the frame index behind each of the NF = n_frames output frames, or NULL: NF = T, all frames
 * in order (n_frames is not read).  An output frame whose index is outside [0, length[b]) is all zero; source frames at or
 * past length[b] are never read.  scratch: mdm_motion_render_scratch_floats(B, T) floats (8 + 2 T per sample: the clip's
 * extent and its root path).  Any T (the trajectory goes through LDS in chunks).  Two launches, stream-ordered, no allocation.
 * MDM_ERR_ARG, before the device is touched: a null pointer (length, frames excepted), B < 0, T < 1, H or W < 4, W % 4 != 0, a
 * mode other than 0 / 1, frames with n_frames < 1, out not 4-byte aligned, a malformed skeleton, J != skeleton->joints, a
 * non-finite camera or style value, |elevation| >= 89.9, distance, near or field of view <= 0, field of view >= 180,
 * near >= distance, a negative width.  MDM_ERR_UNSUPPORTED: B or NF above 65535 (grid dimensions). */
int64_t mdm_motion_render_scratch_floats(int32_t B, int32_t T);
int mdm_motion_render(const float* joints, const int32_t* length, const MdmSkeleton* skeleton, int32_t B, int32_t T, int32_t J,
                      int32_t H, int32_t W, const float* camera, const float* style, int32_t mode, const int32_t* frames,
                      int32_t n_frames, uint8_t* out, float* scratch, void* stream);

/* World view of the motion preview (csrc/motion_world_render.hip): C <= 4 characters and the primitives of a
 * scene in one picture per frame, in world coordinates (no root subtraction).  joints (B, C, T, J, 3) fp32, lengths (B, C)
 * int32 or NULL (= T): a character of length 0 is absent, a character is not drawn at or past its own length, the world's
 * length is the longest character's.  scene (B, K, MDM_SCENE_REC), K <= MDM_SCENE_MAX_PRIMS, and tracks
 * (B, T, Km, MDM_SCENE_REC), Km <= MDM_SCENE_MAX_TRACKS: the records of the scene calls below (kind 0 draws nothing; margins
 * and weights are not read).  mdm_world_extent: extent_out (B, 6) = per-axis minimum (3) and maximum (3) over the valid
 * frames of every character, the boxes around static spheres, capsules and boxes, and those around the same kinds among the
 * track records of frames below the world's length; +inf / -inf for a world with none of these.
 * mdm_world_render: camera[8], mode, frames / n_frames and out as in mdm_motion_render, an output frame whose index is outside
 * [0, the world's length) being all zero.  ground (B) device fp32: the height of each world's ground, the extent's XZ
 * rectangle grown by 0.5 m.  style[18 + 5 C (1 + nchains)]: background r, g, b; floor r, g, b, alpha; solid r, g, b, alpha
 * (primitives); edge r, g, b and full width in points (a box's edges); the shade factors of a box's top, its local-x sides
 * and its local-z sides; then per character r, g, b, alpha, width of its trajectory and of every chain.  After the ground and
 * the trajectories the drawn primitives (static, then tracks) and the (character, chain) groups are composited far to near by
 * the view depth of a reference point, ties to the lower index: a painter's order per item (DESIGN.md §26 defines every
 * item's picture).  scratch: mdm_world_render_scratch_floats(B, C, T, n_frames, K, Km) floats (n_frames = T without frames;
 * -1 for bad arguments).  Three launches, stream-ordered, no allocation, no host synchronisation.
 * MDM_ERR_ARG, before the device is touched: a null pointer (lengths, frames, and scene / tracks with K / Km == 0 excepted),
 * B < 0, C outside [1, 4], T < 1, J outside [1, 32], K or Km outside their limits, and for mdm_world_render everything
 * mdm_motion_render refuses (sizes, mode, frames, alignment of out, skeleton, camera, non-finite style, a negative width).
 * MDM_ERR_UNSUPPORTED: B or NF above 65535 (grid dimensions). */
int mdm_world_extent(const float* joints, const int32_t* lengths, const float* scene, int32_t K, const float* tracks, int32_t Km,
                     int32_t B, int32_t C, int32_t T, int32_t J, float* extent_out, void* stream);
int64_t mdm_world_render_scratch_floats(int32_t B, int32_t C, int32_t T, int32_t n_frames, int32_t K, int32_t Km);
int mdm_world_render(const float* joints, const int32_t* lengths, const MdmSkeleton* skeleton, const float* scene, int32_t K,
                     const float* tracks, int32_t Km, int32_t B, int32_t C, int32_t T, int32_t J, int32_t H, int32_t W,
                     const float* camera, const float* style, const float* ground, int32_t mode, const int32_t* frames,
                     int32_t n_frames, uint8_t* out, float* scratch, void* stream);

/* Body view of the motion preview (csrc/motion_mesh_render.hip): the vertices of a mesh -> image frames, a
 * triangle rasteriser with a depth test per pixel and shading from normals over the floor and trajectory of
 * mdm_motion_render.  vertices (B, T, V, 3) fp32, as mdm_skin_vertices writes them; normals the same or NULL; faces (F, 3)
 * int32 on the device, shared by the batch; root (B, T, 3) fp32: the point each frame's x, z are relative to, and the
 * trajectory; length (B) int32 or NULL (= T).  The image is defined in DESIGN.md §32: MINS / MAXS over the valid frames'
 * vertices (a NaN or infinite coordinate is no part of them); a face with a non-finite vertex, an index outside [0, V), a vertex in front of the near plane or no area on the
 * screen is not drawn (no clipping); coverage by edge functions that two faces sharing an edge evaluate to the same bits, so a
 * closed surface has no cracks; two-sided; the covering face with the largest perspective-correct 1/z wins, ties to the lower
 * face index; I = ambient + (1 - ambient) max(0, n . l) with n the face's normal (mode bit 1 clear) or the interpolated vertex
 * normal (mode bit 1 set, needs normals), turned towards the eye.  camera[8], frames / n_frames and out as in
 * mdm_motion_render; mode bit 0: palette indices.  style[20]: background r, g, b; floor r, g, b, alpha; trajectory r, g, b,
 * alpha, full width in points; body r, g, b, alpha; ambient; light x, y, z (any length > 0) in the camera's (right, up,
 * towards the eye).  scratch: mdm_mesh_render_scratch_floats(B, T, n_frames, V, F, with_normals) floats, 16-byte aligned
 * (n_frames = T without frames; -1 for bad arguments): the extent's slices, and per drawn frame the projected vertices
 * (8 floats each), the view-space normals (4, with normals) and each face's pixel box (2 dwords).  Three launches,
 * stream-ordered, no allocation, no host synchronisation, no atomics on global memory; 64-bit offsets.  Every sample equals
 * its own run alone bit for bit.  MDM_ERR_ARG, before the device is touched: a null pointer (normals, length, frames
 * excepted), B < 0, T < 1, V or F outside [1, 2^24], H or W outside [4, 8192], W % 4 != 0, a mode outside [0, 3], mode bit 1
 * without normals, frames with n_frames < 1, out not 4-byte or scratch not 16-byte aligned, a camera mdm_motion_render
 * refuses, a non-finite style value, a negative width, a light without length.  MDM_ERR_UNSUPPORTED: B or NF above 65535 (grid
 * dimensions).  B = 0 or NF = 0: nothing is launched. */
int64_t mdm_mesh_render_scratch_floats(int32_t B, int32_t T, int32_t n_frames, int32_t V, int32_t F, int32_t with_normals);
int mdm_mesh_render(const float* vertices, const float* normals, const int32_t* faces, const float* root, const int32_t* length,
                    int32_t B, int32_t T, int32_t V, int32_t F, int32_t H, int32_t W, const float* camera, const float* style,
                    int32_t mode, const int32_t* frames, int32_t n_frames, uint8_t* out, float* scratch, void* stream);

/* Joint-position control (csrc/motion_control.hip).  For sample b, with J = (F + 1) / 12 joints (F must be
 * 12 J - 1: 263 -> 22, 251 -> 21), targets G and weights W dense fp32 (B, T, J, 3), W >= 0 and finite, mean / std fp32
 * (B, F) (one row per sample), and P = recover_from_ric(x0 * std + mean) without temporal filter (as mdm_motion_postprocess
 * computes it at radius 0):
 *   L_b = sum_{t < length[b], j, c} W[t, j, c] (P[t, j, c] - G[t, j, c])^2
 * (entries with W == 0 contribute nothing, whatever G holds).  Only the steerable columns, root 0..3 and ric 4 .. 3J, enter
 * recover_from_ric; every other column, and every frame at or past length[b], has gradient exactly 0.
 * mdm_joint_loss_grad: loss_out (B) and grad_out (B, T, F) = dL_b / dx0, with respect to the normalised features (so it
 * carries the std factor).  mdm_joint_guidance: runs after a sampler step's update kernel, on the same stream and before the
 * step counter moves; x0 is the (guided / composed / edited) x0 that update wrote, x its x_{t-1}.  It runs `iters`
 * iterations x0' = x0' - scale * (1 - mask) * dL/dx0' (mask (B, T, F) in [0, 1], or NULL = 0) from x0' = x0, recomputing P
 * each time, then with delta = x0' - x0 writes x0 = x0' and x = x + c0[t] * delta, c0[t] = coef[4 t + 1] (the runner's
 * coefficient table, t = *t_dev when non-NULL else t_imm): every update is linear in x0, so this is the update run on x0'.
 * Nothing is stored where delta == 0 (an all-zero W leaves x and x0 bit for bit, -0.0 included); nothing is re-clamped.
 * T is limited by the LDS that holds the steerable columns: mdm_joint_control_max_frames(F) (205 at F = 263, 211 at 251;
 * 0 for an F not of the form 12 J - 1).  MDM_ERR_ARG: a null pointer (mask excepted), a bad F, T < 1 or over that limit,
 * B < 0, iters outside [1, MDM_CONTROL_MAX_ITERS], a non-finite scale, steps <= 0 or t_imm outside [0, steps) without t_dev. */
enum { MDM_CONTROL_MAX_ITERS = 32 };
int mdm_joint_control_max_frames(int32_t feats);
int mdm_joint_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                        const float* weights, int32_t B, int32_t T, int32_t F, float* loss_out, float* grad_out,
                        void* stream);
int mdm_joint_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                       const float* targets, const float* weights, int32_t B, int32_t T, int32_t F, float scale,
                       int32_t iters, const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm,
                       void* stream);

/* Joint-position control over the canvas of a long motion (csrc/motion_control_canvas.hip): the loss above
 * over canvas frames.  Motion m < M owns canvas frames c in [motion_offsets[m], motion_offsets[m + 1]) (int32 (M + 1), rising
 * from 0 to total_frames); the feature row of frame c is row frame_rows[c] of the (rows, F) buffers x / x0 / mask
 * (frame_rows[c] = window_row * T + frame in a sampler batch); targets and weights are dense (total_frames, J, 3) in canvas
 * order, mean / std (M, F).  L_m = sum over the motion's frames of W (P - G)^2 with P = recover_from_ric over the motion's
 * rows in canvas order: a target late in the canvas reaches the root velocities of every earlier frame, whatever row holds
 * them.  Any canvas length: per-frame state lives in `workspace`, mdm_canvas_control_workspace_floats(total_frames, F)
 * floats (0 for an F not of the form 12 J - 1), the caller's, used by one call at a time.
 * mdm_canvas_joint_loss_grad: loss_out (M) and grad_out (total_frames, F) dense in canvas order.  mdm_canvas_joint_guidance:
 * as mdm_joint_guidance, x0 and x updated at the rows frame_rows names and nowhere else, nothing stored where delta == 0.
 * The scans are wave-parallel fp64 sums: P agrees with mdm_motion_postprocess to rounding, not bit for bit.
 * frame_rows must be in range and distinct and the offsets must rise: the caller's tables, not checked here.  No allocation,
 * no host sync, graph-capturable.  MDM_ERR_ARG: a null pointer (mask excepted), a bad F, M < 0, iters outside
 * [1, MDM_CONTROL_MAX_ITERS], a non-finite scale, steps <= 0 or t_imm outside [0, steps) without t_dev.
 * MDM_ERR_UNSUPPORTED: more than 77 joints (the LDS tile the rows are transposed through).  M == 0 and empty motions are
 * no-ops. */
int64_t mdm_canvas_control_workspace_floats(int32_t total_frames, int32_t F);
int mdm_canvas_joint_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                               const float* std, const float* targets, const float* weights, int32_t M, int32_t F,
                               float* loss_out, float* grad_out, float* workspace, void* stream);
int mdm_canvas_joint_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                              const float* mean, const float* std, const float* targets, const float* weights, int32_t M,
                              int32_t F, float scale, int32_t iters, const float* coef, int32_t steps, const int32_t* t_dev,
                              int32_t t_imm, float* workspace, void* stream);

/* Scene constraints (csrc/scene_sdf.h inside both control kernels): keep joints out of obstacles and above
 * the floor.  A scene is K <= MDM_SCENE_MAX_PRIMS primitives per sample (or per long motion), fixed in the frame of
 * recover_from_ric (the canvas frame of a long motion): `scene` dense fp32 (B or M, K, MDM_SCENE_REC), a record being
 *   kind, sigma, weight a >= 0, margin m, and eight parameters:
 *   MDM_SCENE_SPHERE      centre[3], radius                    d = |p - c| - r
 *   MDM_SCENE_CAPSULE     end a[3], end b[3], radius           d = distance to the segment - r  (a == b: a sphere)
 *   MDM_SCENE_BOX         centre[3], half extents[3], cos yaw, sin yaw (yaw about Y)
 *                                                              d = |max(q, 0)| + min(max(q_x, q_y, q_z), 0), q = |local p| - h
 *   MDM_SCENE_HALF_SPACE  unit normal[3], offset               d = n . p - o
 *   MDM_SCENE_PAD (0) and any other kind: skipped.
 * sigma = +1 keeps joints out, -1 keeps them in.  `joint_params` dense fp32 (B or M, J, 2): radius r_j >= 0 and weight
 * u_j >= 0 of every joint (u_j == 0 exempts it).  The loss of the existing calls gains
 *   L_scene = sum_{t < length, j} u_j sum_k a_k max(0, m_k + r_j - sigma_k d_k(P[t, j]))^2
 * and everything else about them holds: the gradient, the guidance iterations, the update of x, what is left untouched.
 * Where the gradient of d is undefined (the exact centre or axis) it is taken as 0.  targets and weights may both be NULL
 * (no target term).  With K == 0 and targets the calls are the existing ones, launch for launch.
 * The window calls keep the records in LDS: T <= mdm_joint_scene_max_frames(F, K) (202 at F = 263 and 208 at 251 with K = 16;
 * 0 for a bad F or K).  MDM_ERR_ARG: K outside [0, MDM_SCENE_MAX_PRIMS], a null scene with K > 0, null joint_params, one of
 * targets / weights without the other, T over the limit, and everything the existing calls refuse.  The values are the
 * caller's (finite, a >= 0, radii and half extents > 0): not checked here. */
enum { MDM_SCENE_MAX_PRIMS = 16, MDM_SCENE_REC = 12 };
enum { MDM_SCENE_PAD = 0, MDM_SCENE_SPHERE = 1, MDM_SCENE_CAPSULE = 2, MDM_SCENE_BOX = 3, MDM_SCENE_HALF_SPACE = 4 };
int mdm_joint_scene_max_frames(int32_t feats, int32_t prims);
int mdm_joint_scene_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                              const float* weights, const float* scene, int32_t K, const float* joint_params, int32_t B,
                              int32_t T, int32_t F, float* loss_out, float* grad_out, void* stream);
int mdm_joint_scene_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                             const float* targets, const float* weights, const float* scene, int32_t K,
                             const float* joint_params, int32_t B, int32_t T, int32_t F, float scale, int32_t iters,
                             const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, void* stream);
int mdm_canvas_scene_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                               const float* std, const float* targets, const float* weights, const float* scene, int32_t K,
                               const float* joint_params, int32_t M, int32_t F, float* loss_out, float* grad_out,
                               float* workspace, void* stream);
int mdm_canvas_scene_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                              const float* mean, const float* std, const float* targets, const float* weights,
                              const float* scene, int32_t K, const float* joint_params, int32_t M, int32_t F, float scale,
                              int32_t iters, const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm,
                              float* workspace, void* stream);

/* Tracks: primitives that move.  A track is a primitive of the scene whose record may differ in every frame
 * (a swinging bar, a rolling ball, the bones of another character); kind MDM_SCENE_PAD makes it absent in a frame.  `tracks`
 * dense fp32 (B, T, Km, MDM_SCENE_REC) for the window calls, (total canvas frames, Km, MDM_SCENE_REC) in canvas order for
 * the canvas calls, Km <= MDM_SCENE_MAX_TRACKS, records and frame as above.  The loss of the scene calls gains
 *   L_tracks = sum_{t < length, j} u_j sum_k a_{t,k} max(0, m_{t,k} + r_j - sigma_{t,k} d(R[t, k]; P[t, j]))^2
 * with R[t, k] the record of track k at frame t.  Records are data: no gradient reaches them.  The records stay in global
 * memory (the LDS layout and mdm_joint_scene_max_frames are those of the scene calls).
 * `track_bounds` (B, T, 4) / (total, 4) or NULL: per frame a ball (centre[3], radius) that contains every keep-out track of
 * weight > 0 of that frame inflated by its margin.  A joint with |P - centre| > radius + r_j skips the frame's records, which
 * changes no result as long as the ball does contain them: inflate it against fp32 rounding.  Radius +inf (a frame with a
 * half-space or a keep-in track) never skips, -inf (no live track) always; NULL never skips.
 * tracks and track_bounds are read 16 bytes at a time.  `scene` with K == 0, targets / weights and track_bounds may be NULL.
 * With Km == 0 the calls are the scene calls, launch for launch.  MDM_ERR_ARG: Km outside [0, MDM_SCENE_MAX_TRACKS], null
 * tracks with Km > 0, tracks or track_bounds not 16-byte aligned, and everything the scene calls refuse (the T limit is
 * theirs). */
enum { MDM_SCENE_MAX_TRACKS = 24 };
int mdm_joint_tracks_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                               const float* weights, const float* scene, int32_t K, const float* joint_params,
                               const float* tracks, int32_t Km, const float* track_bounds, int32_t B, int32_t T, int32_t F,
                               float* loss_out, float* grad_out, void* stream);
int mdm_joint_tracks_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                              const float* targets, const float* weights, const float* scene, int32_t K,
                              const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds, int32_t B,
                              int32_t T, int32_t F, float scale, int32_t iters, const float* coef, int32_t steps,
                              const int32_t* t_dev, int32_t t_imm, void* stream);
int mdm_canvas_tracks_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                                const float* std, const float* targets, const float* weights, const float* scene, int32_t K,
                                const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds, int32_t M,
                                int32_t F, float* loss_out, float* grad_out, float* workspace, void* stream);
int mdm_canvas_tracks_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                               const float* mean, const float* std, const float* targets, const float* weights,
                               const float* scene, int32_t K, const float* joint_params, const float* tracks, int32_t Km,
                               const float* track_bounds, int32_t M, int32_t F, float scale, int32_t iters, const float* coef,
                               int32_t steps, const int32_t* t_dev, int32_t t_imm, float* workspace, void* stream);

/* Terrain (csrc/terrain.h inside both control kernels): a height-map ground that joints stay above and planted
 * feet stand on.  `terrain` dense fp32 (B or M, Gz, Gx): per sample (per long motion) a grid of heights in metres, row major
 * (the sample of cell column i, row k at k Gx + i), 2 <= Gx, Gz <= MDM_TERRAIN_MAX_GRID.  `terrain_rec` dense fp32
 * (B or M, MDM_TERRAIN_REC): origin x, origin z, cos yaw, sin yaw, 1 / cell_x, 1 / cell_z, weight a >= 0, margin m, in the
 * frame of recover_from_ric (the canvas frame of a long motion).  For a point p:
 *   (lx, lz) = R_y(-yaw) (p_xz - origin),  u = clamp(lx / cell_x, 0, Gx - 1),  v = clamp(lz / cell_z, 0, Gz - 1),
 *   i = min(floor(u), Gx - 2),  k = min(floor(v), Gz - 2),  h(p) bilinear in the four samples around (i, k);
 *   outside the grid the nearest edge's height holds, with zero slope in the clamped direction;
 *   e = p_y - h(p): the vertical clearance, not the true distance to the surface.
 * `stand` dense fp32 (B, T, J) for the window calls, (total canvas frames, J) in canvas order for the canvas calls, or NULL
 * (all 0): S[t, j] >= 0 says how strongly joint j is planted in frame t.  The loss of the tracks calls gains
 *   L_terrain = sum_{t < length, j} u_j a (max(0, m + r_j - e)^2 + S[t, j] max(0, e - r_j - m)^2)
 * with (r_j, u_j) the joint_params of the scene calls (required here as well).  The grid and S are data: no gradient reaches
 * them.  On a grid line, where the slope of h jumps, the cell that floor() gives is taken.  The grid stays in global memory
 * (the LDS layout and mdm_joint_scene_max_frames are those of the scene calls); scene with K == 0, tracks with Km == 0,
 * targets / weights, track_bounds and stand may be NULL.  With terrain == NULL the calls are the tracks calls, launch for
 * launch, and the other terrain arguments are not looked at.  MDM_ERR_ARG: Gx or Gz outside [2, MDM_TERRAIN_MAX_GRID], a
 * NULL terrain_rec with a grid, terrain_rec not 16-byte aligned (it is read 16 bytes at a time), terrain or stand not 4-byte
 * aligned, and everything the tracks calls refuse (the T limit is the scene's).  The values are the caller's (finite,
 * a >= 0, S >= 0, cells > 0): not checked here. */
enum { MDM_TERRAIN_MAX_GRID = 512, MDM_TERRAIN_REC = 8 };
int mdm_joint_terrain_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                                const float* weights, const float* scene, int32_t K, const float* joint_params,
                                const float* tracks, int32_t Km, const float* track_bounds, const float* terrain,
                                const float* terrain_rec, int32_t Gx, int32_t Gz, const float* stand, int32_t B, int32_t T,
                                int32_t F, float* loss_out, float* grad_out, void* stream);
int mdm_joint_terrain_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                               const float* targets, const float* weights, const float* scene, int32_t K,
                               const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds,
                               const float* terrain, const float* terrain_rec, int32_t Gx, int32_t Gz, const float* stand,
                               int32_t B, int32_t T, int32_t F, float scale, int32_t iters, const float* coef, int32_t steps,
                               const int32_t* t_dev, int32_t t_imm, void* stream);
int mdm_canvas_terrain_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                                 const float* std, const float* targets, const float* weights, const float* scene, int32_t K,
                                 const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds,
                                 const float* terrain, const float* terrain_rec, int32_t Gx, int32_t Gz, const float* stand,
                                 int32_t M, int32_t F, float* loss_out, float* grad_out, float* workspace, void* stream);
int mdm_canvas_terrain_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                                const float* mean, const float* std, const float* targets, const float* weights,
                                const float* scene, int32_t K, const float* joint_params, const float* tracks, int32_t Km,
                                const float* track_bounds, const float* terrain, const float* terrain_rec, int32_t Gx,
                                int32_t Gz, const float* stand, int32_t M, int32_t F, float scale, int32_t iters,
                                const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, float* workspace,
                                void* stream);
/* Stand weights from a step's foot-contact labels (csrc/terrain.hip): out (n_frames, J) = 1 at foot joint feet[k] of a frame
 * whose de-normalised contact column (x0[row, F - 4 + k] * std[F - 4 + k] + mean[F - 4 + k], two fp32 operations) exceeds
 * threshold, 0 at every other joint.  x0 rows of F floats; frame f reads row frame_rows[f], or row f with frame_rows NULL;
 * mean / std on the device: (F,) with stat_group == 0, else one row of F per stat_group frames (frame f takes row
 * f / stat_group: a batch of windows of T frames with per-sample statistics is stat_group = T, one launch); feet: four joint
 * indices in host memory, read before the call returns.  Stream-ordered, allocation free, graph-capturable.  MDM_ERR_ARG: a
 * null pointer (frame_rows excepted), n_frames < 0, stat_group < 0, F + 1 no multiple of 12, a foot outside [0, J), a
 * non-finite threshold; n_frames == 0 is a no-op. */
int mdm_terrain_stand_weights(const float* x0, const int32_t* frame_rows, int32_t n_frames, const float* mean, const float* std,
                              int32_t F, int32_t stat_group, const int32_t* feet, float threshold, float* out, void* stream);

/* Characters sampled together (csrc/motion_partners.hip): from a step's x0 (B, T, F), the tracks and targets of
 * the tracks / terrain guidance calls above, so that every row avoids and reaches for its partners' current estimate.  Row b
 * has length[b], mean / std rows (B, F) and a placement placements[b] = (x, z, cos yaw, sin yaw) (fp32 (B, 4), 16-byte
 * aligned).  With P_b = recover_from_ric(x0[b] * std + mean) unfiltered (mdm_motion_postprocess at radius 0 on x0 * std + mean
 * as two fp32 roundings, bit for bit: the launch of that call is reused; `scratch`, the caller's, holds
 * mdm_partner_tracks_scratch_floats(B, T, F) floats, 0 for a bad size):
 *   world (B, T, J, 3), the caller's scratch: W_b[t, j] = R_y(yaw_b) P_b[t, j] + (x_b, 0, z_b) in fp32, zero at t >= length[b];
 *   L_b(w) = R_y(-yaw_b) (w - (x_b, 0, z_b)).
 * partner_rows int32 (B, Pm): the rows that row b avoids, or -1 for an empty slot.  bones int32 (nb, 2) in host memory, read
 * before the call returns.  Behind the Ks static records of `tracks` (B, T, Km, MDM_SCENE_REC), Km = Ks + Pm nb, which are
 * only read, record Ks + q nb + i of frame t is written: for p = partner_rows[b, q] >= 0 and t < min(length[b], length[p]) a
 * keep-out MDM_SCENE_CAPSULE with ends L_b(W_p[t, bones[i, 0]]), L_b(W_p[t, bones[i, 1]]) and the call's radius, margin and
 * weight, else twelve zero floats.  track_bounds (B, T, 4): per frame the ball of the tracks calls' broad phase over all Km
 * records of the frame, in fp32 and inflated by 1e-3 of its radius plus 1e-3 m (+inf with a live half-space or keep-in
 * record, -inf without a live record).  Both are written 16 bytes at a time.
 * contacts: Nc entries of eight 32-bit words: row a, joint a, row b, joint b, first, last (int32), meet (fp32), 0.  For
 * first <= t < min(last, length[a], length[b]), m = W_a[t, joint a] + meet (W_b[t, joint b] - W_a[t, joint a]) and
 * targets[a, t, joint a] = L_a(m), targets[b, t, joint b] = L_b(m), targets (B, T, J, 3); nothing else of targets is written.
 * partner_rows and contacts are on the device; partner_rows_host and contacts_host are the same tables in host memory, which
 * are what is checked here, before any launch (keeping the two equal is the caller's).  Every record is built from the x0 the
 * call is given: the result depends on no order among the rows.  Up to five launches, stream-ordered, allocation free, no
 * atomics, graph-capturable.  MDM_ERR_ARG: a null required pointer (tracks / track_bounds with Km == 0, the partner tables
 * with Pm nb == 0 and contacts / targets with Nc == 0 excepted), Km outside [0, MDM_SCENE_MAX_TRACKS], Ks + Pm nb != Km, F + 1
 * no multiple of 12, a bone or a contact joint outside [0, J), a partner row outside [-1, B) or equal to its own row, a contact
 * row outside [0, B), placements, tracks or track_bounds not 16-byte aligned, first > last, meet outside [0, 1] or not finite,
 * radius <= 0, weight < 0, a non-finite radius, margin or weight.  MDM_ERR_UNSUPPORTED: T > mdm_partner_tracks_max_frames()
 * (20 bytes of LDS per frame).  B == 0 or T == 0 is a no-op. */
int mdm_partner_tracks_max_frames(void);
int64_t mdm_partner_tracks_scratch_floats(int32_t B, int32_t T, int32_t F);
int mdm_partner_tracks(const float* x0, const int32_t* length, const float* mean, const float* std, const float* placements,
                       const int32_t* partner_rows, const int32_t* partner_rows_host, int32_t Pm, const int32_t* bones,
                       int32_t nb, float radius, float margin, float weight, int32_t Ks, int32_t Km, const int32_t* contacts,
                       const int32_t* contacts_host, int32_t Nc, int32_t B, int32_t T, int32_t F, float* world, float* scratch,
                       float* tracks, float* track_bounds, float* targets, void* stream);

/* Self-collision avoidance (csrc/motion_self.hip): keep a character's joints out of the capsules of its own
 * bones, as per-step targets of the guidance calls above.  bones int32 (nb, 2) in host memory, read before the call returns:
 * bone i is the segment P[t, bones[i, 0]] ... P[t, bones[i, 1]] of the same frame, with radius bone_radius[i] (nb, device);
 * joint_params (J, 2) on the device: the joint's radius r_j and weight u_j; pair_mask int32 (J) on the device: bit i of
 * pair_mask[j] says that bone i acts on joint j.  For t < length[b], with d_i the distance of P[t, j] to the segment of bone i,
 * c_i the closest point on it, pen_i = max(0, margin + r_j + bone_radius[i] - d_i) and n_i = (P[t, j] - c_i) / d_i (0 where
 * d_i < 1e-12):
 *   push[b, t, j] = sum_i pen_i n_i,  depth[b, t, j] = sum_i pen_i   over the allowed bones in ascending i (a fixed order:
 *   the same bits run after run); both are zero at t >= length[b].  Bones are data: nothing is differentiated.
 * mdm_self_push: joints (B, T, J, 3) -> push_out (B, T, J, 3) and depth_out (B, T, J) or NULL.  One launch.
 * mdm_self_targets: P = recover_from_ric(x0 * std + mean) unfiltered, bit for bit, by the two launches mdm_partner_tracks starts
 * with (mean / std rows (B, F); `scratch`, the caller's, holds mdm_self_targets_scratch_floats(B, T, F) floats, 0 for a bad
 * size), written to joints_out (B, T, J, 3); then the push launch with the merge fused, writing targets_out and weights_out,
 * both (B, T, J, 3) as the guidance calls read them: where one of static_weights[b, t, j, :] is not zero, and in every frame at
 * or past length[b], the static target and weights bit for bit (zeros without a static pair); elsewhere
 * targets = P + push and all three weights = depth > 0 ? weight * u_j : 0.  The gradient of sum w |P - g|^2 at these targets
 * is the gradient of weight * sum_j u_j sum_i pen_i^2 with the bones held fixed.  static_targets / static_weights (B, T, J, 3):
 * both or neither.  Stream-ordered, allocation free, no atomics, graph-capturable.  MDM_ERR_ARG, before any launch: a null
 * required pointer (depth_out and the static pair excepted), J outside [2, 32], nb outside [1, 31], a bone end outside [0, J),
 * F + 1 no multiple of 12, one of the static pair without the other, a non-finite margin or weight, weight < 0.
 * MDM_ERR_UNSUPPORTED: T > mdm_self_max_frames() (the recovery's LDS limit).  B == 0 or T == 0 is a no-op. */
int mdm_self_max_frames(void);
int64_t mdm_self_targets_scratch_floats(int32_t B, int32_t T, int32_t F);
int mdm_self_push(const float* joints, const int32_t* length, const int32_t* bones, int32_t nb, const float* bone_radius,
                  const float* joint_params, const int32_t* pair_mask, float margin, int32_t B, int32_t T, int32_t J,
                  float* push_out, float* depth_out, void* stream);
int mdm_self_targets(const float* x0, const int32_t* length, const float* mean, const float* std, const int32_t* bones, int32_t nb,
                     const float* bone_radius, const float* joint_params, const int32_t* pair_mask, float margin, float weight,
                     const float* static_targets, const float* static_weights, int32_t B, int32_t T, int32_t F,
                     float* joints_out, float* scratch, float* targets_out, float* weights_out, void* stream);

/* ---- long-motion handshakes ---------------------------------------------------------------------
 * In place over the shared canvas frames only.  For every group g < groups, shared frame c < nshared and feature j < F:
 *   v = sum over entries e in [offsets[c], offsets[c+1]) of weights[e] * x[g*group_stride + rows[e]*F + j]
 *   (fp32 fmaf chain in entry order, from 0), then x[... rows[e] ...] = v for every e.
 * weights == NULL: copy mode; every entry receives entry offsets[c]'s value bit for bit.
 * rows[e] = window_row * T + frame; the rows of all entries must be distinct (each element is owned by one thread) and in
 * range: both are the caller's tables, not checked here.  No allocation, no host sync, graph-capturable.
 * MDM_ERR_ARG on null x / offsets / rows with nshared > 0, F < 1, groups < 1, nshared < 0 or group_stride < 0;
 * nshared == 0 is a no-op. */
int mdm_handshake_blend(float* x, int32_t groups, int64_t group_stride, int32_t F, int32_t nshared,
                        const int32_t* offsets, const int32_t* rows, const float* weights, void* stream);

/* ---- training step of the MoE feed-forward block --------------------------------------------
 * MoEMultiBranchFFN.forward (multi_branch.py:52-61) with both SwitchMoELayers (switch_moe.py:44-111) and the StylizationBlock
 * (stylization.py:20-31) in training mode, and its backward: what loss.backward() does for this block inside
 * DDPMTrainer.update (ddpm_trainer.py:228-244).  fp32 master parameters in the state_dict layouts, the two branches stacked on
 * a leading dimension; the same struct holds the gradients (same shapes, OVERWRITTEN by the backward).  Dropout
 * (multi_branch.py:57 on each branch's output, stylization.py:16 after the SiLU): dropout_p in [0, 1), masks from the
 * counter-based generator keyed on (seed, site, row, element), regenerated by the backward (pass the same p and seed);
 * p > 0 needs D in {256, 512, 1024}.  The GEMMs are the bf16x3 (fp32-grade) kernel; gradients match fp32 autograd to ~1e-5. */
typedef struct MdmMoeTensors {
  float* ln_w;      /* [2][D]        branches.{b}.layernorm.weight */
  float* ln_b;      /* [2][D] */
  float* gate_w;    /* [2][E][D]     branches.{b}.moe.gate.weight */
  float* gate_b;    /* [2][E] */
  float* w1;        /* [2][E][F][D]  branches.{b}.moe.experts.{e}.0.weight */
  float* b1;        /* [2][E][F] */
  float* w2;        /* [2][E][D][F]  branches.{b}.moe.experts.{e}.2.weight */
  float* b2;        /* [2][E][D] */
  float* st_emb_w;  /* [2D][Te]      proj_out.emb_layers.1.weight */
  float* st_emb_b;  /* [2D] */
  float* st_norm_w; /* [D]           proj_out.norm */
  float* st_norm_b;
  float* st_out_w;  /* [D][D]        proj_out.out_layers.2.weight */
  float* st_out_b;  /* [D] */
} MdmMoeTensors;

int64_t mdm_moe_train_workspace_bytes(int32_t B, int32_t S, int32_t D, int32_t F, int32_t E, int32_t Te);
/* out = x + proj_out(mean_b moe_b(LN_b(x)), emb): x [B*S, D], emb [B, De]; when De != Te the captured per-call projection
 * eph_w [Te, De], eph_b [Te] of stylization.py:22-24 is applied first (not trained).  lb_loss (optional, device [2]):
 * get_load_balancing_loss (switch_moe.py:113-145) of the two layers from this forward's counters.  route_out (optional):
 * the top-2 decisions, int32 [2][B*S][2].  Activations needed by the backward stay in ws. */
int mdm_moe_ffn_train_forward(const MdmMoeTensors* params, int32_t D, int32_t F, int32_t E, int32_t Te, int32_t De,
                              const float* eph_w, const float* eph_b, const float* x, const float* emb, int32_t B, int32_t S,
                              float dropout_p, uint64_t seed, float* out, float* lb_loss, int32_t* route_out, void* ws,
                              int64_t ws_bytes, void* stream);
/* given dout = dL/dout [B*S, D] and the workspace of the matching forward: dx [B*S, D], demb [B, De] (optional) and every
 * parameter gradient in `grads`. */
int mdm_moe_ffn_train_backward(const MdmMoeTensors* params, int32_t D, int32_t F, int32_t E, int32_t Te, int32_t De,
                               const float* eph_w, const float* x, const float* emb, int32_t B, int32_t S, float dropout_p,
                               uint64_t seed, const float* dout, float* dx, float* demb, const MdmMoeTensors* grads, void* ws,
                               int64_t ws_bytes, void* stream);
/* optimizer plumbing of ddpm_trainer.py:228-244 on flat fp32 buffers: squared gradient norm (device scalar, for
 * clip_grad_norm_) and one Adam step with the clip factor min(1, max_norm / (sqrt(*sumsq) + 1e-6)) folded in (sumsq NULL or
 * max_norm <= 0: no clip). */
int mdm_sumsq(const float* x, int64_t n, float* out, void* stream);
int mdm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  int32_t step, const float* sumsq, float max_norm, void* stream);

/* small helpers used by the host module */
int mdm_xattn_gate(const float* gate, const float* adaptive_gate, int32_t D, float* out, void* stream);
int mdm_fill_i64(int64_t* dst, int64_t n, const int32_t* src_dev, void* stream);
int mdm_add_i32(int32_t* dst, int32_t delta, void* stream);

/* Kernel-selection knob (mdm_set_gemm_variant): the reference path that a test holds another path against.  0 = default;
 * process-global, not thread-safe, never part of the data path.  The numbers are part of the ABI (tests and bench.py --variant
 * pass them); every other value is refused with MDM_ERR_ARG and leaves the knob unchanged. */
enum MdmVariant {
  MDM_VAR_DEFAULT = 0,
  MDM_VAR_GEMM_256 = 6,          /* the 256 x 256 tile of the 16-bit GEMM wherever it is eligible */
  MDM_VAR_SD_UNFOLDED = 22,      /* text cross-attention unfolded (attention-core kernel) */
  MDM_VAR_GENERIC_DH256 = 23,    /* the generic (GEMM-composed) head_dim-256 paths */
  MDM_VAR_SD_FOLD_ANY = 24,      /* text cross-attention folded at any pass count */
  MDM_VAR_ROUTER_CONST_E = 26,   /* router with compile-time expert count wherever it exists */
  MDM_VAR_ROUTER_RUNTIME_E = 27, /* router with run-time expert count everywhere */
  MDM_VAR_MLP_LDS = 34,          /* fused expert MLP on the LDS-staged kernel (csrc/mlp.hip), not the streamed-weight one */
  MDM_VAR_TAIL_SPLIT = 35,       /* the Performer tail as its own launches, not inside the proj_out pair's launch */
  MDM_VAR_X3_REG = 36,           /* fp32-grade Linears on the register-staged kernel */
  MDM_VAR_QKV_SPLIT = 50,        /* the Performer's q | k | v projection as its own GEMM launch */
  MDM_VAR_XQ_SPLIT = 51,         /* the query of the linear cross-attention as its own GEMM launch */
  MDM_VAR_X3_ATTN_CHAIN = 52,    /* fp32-grade: the attention chain as separate launches */
  MDM_VAR_X3_XATTN_CHAIN = 56,   /* fp32-grade: the cross-attention chains as separate launches */
  MDM_VAR_X3_STYLE_SPLIT = 60,   /* fp32-grade: stylization input and its Linear as two launches */
  MDM_VAR_X3_TAILS_SPLIT = 61,   /* fp32-grade: the LayerNorms / block tails behind the stylization as their own launches */
  MDM_VAR_X3_F32_ROWS = 62,      /* fp32-grade: fp32 rows instead of pre-split rows between the bf16x3 GEMMs */
  MDM_VAR_STREAM_NEVER = 63,     /* streamed-weight GEMM (MdmGemmDesc.w_stream): never */
  MDM_VAR_STREAM_ALWAYS = 68,    /*   wherever it is eligible */
  MDM_VAR_STREAM3_NEVER = 69,    /* its bf16x3 form (pre-split rows x a pair stream): never */
  MDM_VAR_STREAM3_ALWAYS = 70    /*   wherever it is eligible */
};
/* One more value of the same knob, kept apart from the enum above, whose values (all below 128) are a closed set that
 * tests/test_abi.py pins: the MoE router as its own three launches, not inside the stylization launch in front of the block. */
enum MdmRouteVariant { MDM_VAR_ROUTE_LAUNCH = 171 };
/* Likewise: the dual block's skip projection as its own GEMM launch, not on the idle CUs of its first Performer's pair + tail
 * launch. */
enum MdmSkipVariant { MDM_VAR_SKIP_LAUNCH = 172 };
/* Likewise: no launch touches the weights of the launch behind it (csrc/warm.h); the results are the same either way. */
enum MdmWarmVariant { MDM_VAR_NO_WARM = 173 };
/* Likewise: the folded text cross-attention (sd_fold) as its own launch, not in the epilogue of the MoE block's stylization launch
 * in front of it; the results are the same either way. */
enum MdmTextVariant { MDM_VAR_TEXT_LAUNCH = 174 };
int mdm_set_gemm_variant(int variant);

/* Measurement probe for bench.py: while enabled, every launch of the dominant kernel (the fused expert MLP inside
 * mdm_denoiser_forward / mdm_block_forward) is bracketed by a pair of HIP events recorded on the launch stream (do not
 * enable during hipGraph capture).  mdm_probe_read synchronises the events and returns the number of launches recorded
 * since the last enable, writing up to `cap` durations (microseconds) and row counts. */
int mdm_probe_enable(int32_t enable);
/* Test aid: while buf is non-NULL, mdm_denoiser_forward copies the router's decisions into it, laid out like
 * forced_routing: int32 [2L][2 branches][B*S_layer (padded to B*T)][2] (mdm_block_forward(MDM_BLOCK_MOE): one layer's worth).
 * capacity = int32 elements buf holds: a forward that needs more (2L * 4 * B * T) returns MDM_ERR_ARG instead of writing past it.
 * Used to count routing flips against the oracle; pass NULL to switch it off.  Process-global, not thread-safe. */
int mdm_route_dump(int32_t* buf, int64_t capacity);
/* Test aid: where, inside a workspace carved for (m, B, T, N), the LAST MoE block that ran left its routing.  Byte offsets:
 * off[0] hn rows (2, M, D; the mode's expert-operand format), off[1] top_idx (2, M, 2) int32, off[2] top_val (2, M, 2) fp32,
 * off[3] perm (4 M) int32, off[4] rowscale (4 M) fp32, off[5] pos4 (M, 4) int32, off[6] goff (2 E + 1) int32, off[7] cursor
 * (2 E) int32; M = the rows of that block (B * T / 2 at the coarse scale). */
int mdm_route_workspace(const MdmModel* m, int32_t B, int32_t T, int32_t N, int64_t* off);
/* Test aid, the sibling of mdm_route_workspace: where the expert stage of that block left its buffers.  Byte offsets:
 * off[0] hn_scale (2, M) fp32, the per-row scales of e4m3 hn rows (MDM_PREC_FP8 only), off[1] hid (4 M, F), the hidden layer in
 * slab order (e4m3 bytes at MDM_PREC_FP8; not written where both expert GEMMs run in one launch), off[2] y2 (4 M, D), the
 * experts' outputs times their gate probabilities in slab order (fp16 at MDM_PREC_FP8 and MDM_PREC_F16, bf16 at MDM_PREC_BF16,
 * else fp32).  Rows at or past goff[2 E] are never written. */
int mdm_expert_workspace(const MdmModel* m, int32_t B, int32_t T, int32_t N, int64_t* off);
/* Test aid: the sub-buffers of a workspace carved for (m, B, T, N), in carve order, from the table that carves it.  Returns
 * their number (-1: bad model or shape); for the first `cap` of them writes the byte offset (a multiple of 256), the byte size
 * and the kind: 0 = data (fp32, or a narrower float format in the modes that keep one there), 1 = int32 indices and counters
 * (top_idx, perm, pos4, hist, goff, cursor, len_low).  The end of the last one, rounded up to 256, is mdm_workspace_bytes.
 * mdm_workspace_field_name(i): the name of sub-buffer i ("" outside the table). */
int mdm_workspace_layout(const MdmModel* m, int32_t B, int32_t T, int32_t N, int64_t* off, int64_t* bytes, int32_t* kind,
                         int32_t cap);
const char* mdm_workspace_field_name(int32_t i);
/* Number of passes (of <= 128 folded text columns, whole heads) the fused text cross-attention takes for H heads and N text
 * tokens, 0 when the folded path is not taken (D != 512, or more than two passes: N > 64 at H = 4, where the GEMM chain
 * measures faster).  Sizes the optional MdmTextCache buffers:
 * sd_kfold [2L][B][passes][128][D] (16-bit), sd_cb [2L][B][passes][128] (fp32), sd_vfold [2L][B][passes][D][128] (16-bit). */
int mdm_sd_fold_passes(int32_t D, int32_t H, int32_t N);
int mdm_probe_read(float* us, int32_t* rows, int32_t cap);

/* ---- Text-motion evaluator (csrc/evaluator.hip): the reference's datasets1/evaluator_models.py (MovementConvEncoder :79-99,
 * TextEncoderBiGRUCo :311-350, MotionEncoderBiGRUCo :353-386), EvaluatorModelWrapper (datasets1/evaluator.py:418-503) and the
 * formulas of utils/metrics.py.  Every Linear / Conv1d of the three networks runs on mdm_gemm (precision 3); these are the rest. */

/* Bidirectional single-layer GRU over packed sequences (nn.GRU(bidirectional=True) on pack_padded_sequence, evaluator_models.py
 * :344-346 / :380-382), returning the final states out [B][2H] = [forward | backward].
 *   gx    [B][T][2][3H]  x W_ih^T + b_ih of each direction (gate rows r, z, n as in PyTorch); b_hh is added here
 *   w_hh  [2][3H][H], b_hh [2][3H]  weight_hh_l0 / _reverse, bias_hh_l0 / _reverse
 *   h0    [2][H]         the learned initial state (`hidden`, broadcast over the batch)
 *   lens_dev / lens_host the same int32 lengths [B] on the device and on the host: any order (no enforce_sorted), each in [1, T]
 *   ws    mdm_gru_bidir_workspace_bytes(B, H) bytes (two state buffers)
 * One launch per step (max(lens) launches), both directions per launch.  MDM_ERR_ARG: null pointers, a length outside [1, T],
 * a short workspace, w_hh / h0 / ws not 16-byte aligned (checked before any launch); MDM_ERR_UNSUPPORTED: H % 16 != 0 or H > 1024. */
int64_t mdm_gru_bidir_workspace_bytes(int32_t B, int32_t H);
int mdm_gru_bidir(const float* gx, const float* w_hh, const float* b_hh, const float* h0, const int32_t* lens_dev,
                  const int32_t* lens_host, int32_t B, int32_t T, int32_t H, float* out, float* ws, int64_t ws_bytes, void* stream);
/* Row copy of the movement encoder (Conv1d k4 s2 p1 as a GEMM, evaluator_models.py:82-99):
 * dst [B][T + 2 pad][Cp] = act(src row (b T + t), first C columns), zero columns [C, Cp) and zero pad frames at each end;
 * act = LeakyReLU(0.2) when leaky != 0.  With pad = 0 and Cp = C the copy may be in place (dst == src, ld_src == C). */
int mdm_eval_pad_rows(const float* src, int64_t ld_src, int32_t B, int32_t T, int32_t C, int32_t Cp, int32_t pad, int32_t leaky,
                      float* dst, void* stream);
/* y[M][N] = LeakyReLU_0.2(LayerNorm(x; w, b, eps)): the middle of the encoders' output_net (evaluator_models.py:320-325, 360-365) */
int mdm_eval_ln_leaky(const float* x, int32_t M, int32_t N, const float* w, const float* b, float eps, float* y, void* stream);
/* Matching of B text / motion embedding pairs [B][D] (tools/evaluation.py:163-176, utils/metrics.py:6-46):
 * dist [B][B] = euclidean distances (optional, may be NULL), rank[i] = #{j : d_ij < d_ii} (R-precision top-k counts the
 * rows with rank < k), diag[i] = d_ii (the matching score sums it).  One launch.  MDM_ERR_UNSUPPORTED when (D + B) * 4 > 64 KiB. */
int mdm_eval_matching(const float* text, const float* motion, int32_t B, int32_t D, float* dist, int32_t* rank, float* diag,
                      void* stream);
/* Column means of x [N][D] (fp64 sums) and the centred rows xc = x - mean (utils/metrics.py:60-70; the covariance is then
 * xc^T xc / (N - 1) on mdm_gemm with F32_KSTRIDE operands). */
int mdm_eval_center(const float* x, int32_t N, int32_t D, float* mean, float* xc, void* stream);

const char* mdm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MDM_HIP_H */
