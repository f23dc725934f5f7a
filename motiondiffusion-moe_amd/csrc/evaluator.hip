// Text-motion evaluator (the reference's datasets1/evaluator_models.py + utils/metrics.py): the bidirectional GRU
// recurrence, the row-wise helpers around the GEMMs (movement-encoder padding / LeakyReLU, LayerNorm + LeakyReLU of the
// output heads), the matching kernel (distance matrix, rank of the true pair, diagonal) and the centring pass of the
// mean / covariance.  Every Linear / Conv1d of the evaluator runs on mdm_gemm (precision 3) from the host side.
//
// The GRU is one launch per time step: both directions in the same launch, the hidden state ping-ponging between two
// buffers.  No grid barrier, no cross-workgroup waits: a step's launch only reads what the previous launch wrote.
#include "mdm_common.h"

namespace mdm {
namespace {

constexpr int GRU_NT = 256;  // threads per workgroup
constexpr int GRU_KS = 8;    // lanes that split one dot product's k range (float4 columns j, j + 8, ...)
constexpr int GRU_BR = GRU_NT / GRU_KS;  // batch rows per pass

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// One step s of the bidirectional GRU.  Workgroup (slice, d) owns hidden units [u0, u0 + U) of direction d: it stages the
// 3U recurrent-weight rows (r, z, n of those units) in LDS, computes their dot products with h[b] for every batch row b and
// applies the gates (PyTorch order r, z, n):
//   r = sig(gx_r + W_hr h + b_hr),  z = sig(gx_z + W_hz h + b_hz),  n = tanh(gx_n + r * (W_hn h + b_hn)),  h' = (1 - z) n + z h
// Sample b consumes frame s (forward) / len_b - 1 - s (backward) while s < len_b and carries h unchanged afterwards.
// h_in / h_out: [B][2][H] (h_in row stride hb_stride: 0 for the learned initial state [2][H]).
template <int U>
__global__ __launch_bounds__(GRU_NT) void gru_step_kernel(const float* __restrict__ gx, const float* __restrict__ w_hh,
                                                          const float* __restrict__ b_hh, const float* __restrict__ h_in,
                                                          int64_t hb_stride, const int32_t* __restrict__ lens,
                                                          float* __restrict__ h_out, int B, int T, int H, int s) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // [3U][H]
  const int slices = H / U;
  const int d = blockIdx.x / slices;
  const int u0 = (blockIdx.x - d * slices) * U;
  const int tid = threadIdx.x;
  const int H4 = H >> 2;
  const float* wd = w_hh + (int64_t)d * 3 * H * H;
  for (int i = tid; i < 3 * U * H4; i += GRU_NT) {
    const int row = i / H4, c = i - row * H4;
    const int g = row / U, u = row - g * U;
    ((f32x4*)wl)[i] = *(const f32x4*)(wd + ((int64_t)g * H + u0 + u) * H + 4 * c);
  }
  __syncthreads();
  const int j = tid % GRU_KS;
  const float* bd = b_hh + (int64_t)d * 3 * H;
  for (int b0 = 0; b0 < B; b0 += GRU_BR) {
    const int b = b0 + tid / GRU_KS;
    const bool valid = b < B;  // uniform across the 8 lanes of one row
    const float* hb = h_in + (valid ? (int64_t)b * hb_stride : 0) + (int64_t)d * H;
    float acc[3 * U];
#pragma unroll
    for (int r = 0; r < 3 * U; ++r) acc[r] = 0.f;
    if (valid) {
      for (int c = j; c < H4; c += GRU_KS) {
        const f32x4 hv = *(const f32x4*)(hb + 4 * c);
#pragma unroll
        for (int r = 0; r < 3 * U; ++r) {
          const f32x4 w = ((const f32x4*)wl)[r * H4 + c];
          acc[r] = fmaf(w.x, hv.x, fmaf(w.y, hv.y, fmaf(w.z, hv.z, fmaf(w.w, hv.w, acc[r]))));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 3 * U; ++r) {
      acc[r] += __shfl_xor(acc[r], 1);
      acc[r] += __shfl_xor(acc[r], 2);
      acc[r] += __shfl_xor(acc[r], 4);
    }
    if (!valid) continue;
    const int len = lens[b];
    // lane j finishes units j, j + 8, ... of the slice (all lanes hold every reduced sum)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u % GRU_KS != j) continue;
      const int unit = u0 + u;
      const float hprev = hb[unit];
      float hn = hprev;
      if (s < len) {
        const int t = d == 0 ? s : len - 1 - s;
        const float* g = gx + (((int64_t)b * T + t) * 2 + d) * 3 * H;
        const float r = sigmoidf(g[unit] + (acc[u] + bd[unit]));
        const float z = sigmoidf(g[H + unit] + (acc[U + u] + bd[H + unit]));
        const float n = tanhf(g[2 * H + unit] + r * (acc[2 * U + u] + bd[2 * H + unit]));
        hn = (1.f - z) * n + z * hprev;
      }
      h_out[((int64_t)b * 2 + d) * H + unit] = hn;
    }
  }
}

// dst[b][pad + t][c] = act(src[(b T + t) ld_src + c]) for c < C, zero for c in [C, Cp) and for the pad frames at each end.
__global__ void pad_rows_kernel(const float* src, int64_t ld_src, int B, int T, int C, int Cp, int pad, int leaky,
                                float* dst) {  // (may alias src: pad = 0, Cp = C)
  const int Tp = T + 2 * pad;
  const int64_t total = (int64_t)B * Tp * Cp;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / Cp;
    const int c = (int)(i - row * Cp);
    const int b = (int)(row / Tp), tp = (int)(row - (int64_t)b * Tp);
    const int t = tp - pad;
    float v = 0.f;
    if (c < C && t >= 0 && t < T) {
      v = src[((int64_t)b * T + t) * ld_src + c];
      if (leaky && v < 0.f) v *= 0.2f;
    }
    dst[i] = v;
  }
}

// y[m] = LeakyReLU_0.2(LayerNorm(x[m]; w, b, eps)), one workgroup per row (two-pass mean / variance)
__global__ __launch_bounds__(256) void ln_leaky_kernel(const float* x, int N, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float eps, float* y) {  // y may alias x
  __shared__ float red[256 / 64];
  const float* xr = x + (int64_t)blockIdx.x * N;
  float* yr = y + (int64_t)blockIdx.x * N;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto block_sum = [&](float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
  };
  float s = 0.f;
  for (int i = tid; i < N; i += 256) s += xr[i];
  const float mean = block_sum(s) / N;
  float q = 0.f;
  for (int i = tid; i < N; i += 256) {
    const float dv = xr[i] - mean;
    q += dv * dv;
  }
  const float rstd = rsqrtf(block_sum(q) / N + eps);
  for (int i = tid; i < N; i += 256) {
    float v = (xr[i] - mean) * rstd * w[i] + bias[i];
    yr[i] = v < 0.f ? 0.2f * v : v;
  }
}

// Row i of the matching matrix: d_ij = || text_i - motion_j ||_2 for every j, rank_i = #{j : d_ij < d_ii}, diag_i = d_ii.
__global__ __launch_bounds__(256) void matching_kernel(const float* __restrict__ text, const float* __restrict__ motion, int B,
                                                       int D, float* __restrict__ dist, int32_t* __restrict__ rank,
                                                       float* __restrict__ diag) {
  extern __shared__ __attribute__((aligned(16))) float sm[];  // [D] text_i, then [B] distances
  float* ti = sm;
  float* dl = sm + D;
  __shared__ int cnt;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int k = tid; k < D; k += 256) ti[k] = text[(int64_t)i * D + k];
  if (tid == 0) cnt = 0;
  __syncthreads();
  for (int jj = wv; jj < B; jj += 4) {
    const float* mj = motion + (int64_t)jj * D;
    float q = 0.f;
    for (int k = lane; k < D; k += 64) {
      const float dv = ti[k] - mj[k];
      q = fmaf(dv, dv, q);
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (lane == 0) dl[jj] = sqrtf(q);
  }
  __syncthreads();
  const float dii = dl[i];
  int c = 0;
  for (int jj = tid; jj < B; jj += 256) {
    c += dl[jj] < dii ? 1 : 0;
    if (dist) dist[(int64_t)i * B + jj] = dl[jj];
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) atomicAdd(&cnt, c);
  __syncthreads();
  if (tid == 0) {
    rank[i] = cnt;
    diag[i] = dii;
  }
}

// Column means of x [N][D] (fp64 accumulation) and the centred copy xc = x - mean.  A workgroup owns 32 columns; its 8 row
// lanes per column sum rows n, n + 8, ... and meet in LDS.
__global__ __launch_bounds__(256) void center_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ mean,
                                                     float* __restrict__ xc) {
  __shared__ double part[8][32];
  __shared__ float mcol[32];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  double s = 0.0;
  if (c < D)
    for (int n = rl; n < N; n += 8) s += (double)x[(int64_t)n * D + c];
  part[rl][cl] = s;
  __syncthreads();
  if (rl == 0) {
    double t = 0.0;
    for (int k = 0; k < 8; ++k) t += part[k][cl];
    mcol[cl] = (float)(t / N);
    if (c < D) mean[c] = mcol[cl];
  }
  __syncthreads();
  if (c >= D) return;
  const float m = mcol[cl];
  for (int n = rl; n < N; n += 8) xc[(int64_t)n * D + c] = x[(int64_t)n * D + c] - m;
}

int grid_for(int64_t total) {
  int64_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

template <int U>
int gru_launch(const float* gx, const float* w_hh, const float* b_hh, const float* h0, const int32_t* lens, int B, int T, int H,
               int steps, float* out, float* ws, hipStream_t st) {
  const size_t smem = (size_t)3 * U * H * sizeof(float);
  static DevInt set;
  if ((int)smem > 65536 && (int)set < (int)smem) {
    if (hipFuncSetAttribute((const void*)gru_step_kernel<U>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
      return MDM_ERR_LAUNCH;
    set = (int)smem;
  }
  const dim3 grid((unsigned)(2 * (H / U)));
  float* buf[2] = {ws, ws + (int64_t)B * 2 * H};
  for (int s = 0; s < steps; ++s) {
    const float* hin = s == 0 ? h0 : buf[(s - 1) & 1];
    const int64_t hbs = s == 0 ? 0 : 2 * (int64_t)H;
    float* hout = s == steps - 1 ? out : buf[s & 1];
    hipLaunchKernelGGL(gru_step_kernel<U>, grid, dim3(GRU_NT), smem, st, gx, w_hh, b_hh, hin, hbs, lens, hout, B, T, H, s);
    MDM_RETURN_IF_LAUNCH_FAILED();
  }
  return MDM_OK;
}

}  // namespace
}  // namespace mdm

extern "C" {

int64_t mdm_gru_bidir_workspace_bytes(int32_t B, int32_t H) {
  if (B <= 0 || H <= 0) return -1;
  return (int64_t)2 * B * 2 * H * (int64_t)sizeof(float);
}

int mdm_gru_bidir(const float* gx, const float* w_hh, const float* b_hh, const float* h0, const int32_t* lens_dev,
                  const int32_t* lens_host, int32_t B, int32_t T, int32_t H, float* out, float* ws, int64_t ws_bytes,
                  void* stream) {
  if (!gx || !w_hh || !b_hh || !h0 || !lens_dev || !lens_host || !out || !ws || B <= 0 || T <= 0 || H <= 0) return MDM_ERR_ARG;
  if (H % 16 != 0 || H > 1024) return MDM_ERR_UNSUPPORTED;
  if (ws_bytes < mdm_gru_bidir_workspace_bytes(B, H)) return MDM_ERR_ARG;
  if ((((uintptr_t)w_hh) | ((uintptr_t)h0) | ((uintptr_t)ws)) & 15) return MDM_ERR_ARG;  // float4 loads of weights / states
  int steps = 0;
  for (int b = 0; b < B; ++b) {
    if (lens_host[b] < 1 || lens_host[b] > T) return MDM_ERR_ARG;
    steps = lens_host[b] > steps ? lens_host[b] : steps;
  }
  hipStream_t st = (hipStream_t)stream;
  // hidden-unit slices sized so that 2 H / U workgroups cover the 256 CUs at H = 512 and H = 1024
  if (H >= 1024) return mdm::gru_launch<8>(gx, w_hh, b_hh, h0, lens_dev, B, T, H, steps, out, ws, st);
  return mdm::gru_launch<4>(gx, w_hh, b_hh, h0, lens_dev, B, T, H, steps, out, ws, st);
}

int mdm_eval_pad_rows(const float* src, int64_t ld_src, int32_t B, int32_t T, int32_t C, int32_t Cp, int32_t pad, int32_t leaky,
                      float* dst, void* stream) {
  if (!src || !dst || B <= 0 || T <= 0 || C <= 0 || Cp < C || pad < 0 || ld_src < C) return MDM_ERR_ARG;
  if (pad > 0 && (const void*)src == (const void*)dst) return MDM_ERR_ARG;  // in place only without re-layout
  const int64_t total = (int64_t)B * (T + 2 * pad) * Cp;
  hipLaunchKernelGGL(mdm::pad_rows_kernel, dim3(mdm::grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, ld_src, B, T, C, Cp,
                     pad, leaky, dst);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int mdm_eval_ln_leaky(const float* x, int32_t M, int32_t N, const float* w, const float* b, float eps, float* y, void* stream) {
  if (!x || !w || !b || !y || M < 0 || N <= 0) return MDM_ERR_ARG;
  if (M == 0) return MDM_OK;
  hipLaunchKernelGGL(mdm::ln_leaky_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, x, N, w, b, eps, y);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int mdm_eval_matching(const float* text, const float* motion, int32_t B, int32_t D, float* dist, int32_t* rank, float* diag,
                      void* stream) {
  if (!text || !motion || !rank || !diag || B <= 0 || D <= 0) return MDM_ERR_ARG;
  const size_t smem = (size_t)(D + B) * sizeof(float);
  if (smem > 65536) return MDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mdm::matching_kernel, dim3((unsigned)B), dim3(256), smem, (hipStream_t)stream, text, motion, B, D, dist, rank,
                     diag);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int mdm_eval_center(const float* x, int32_t N, int32_t D, float* mean, float* xc, void* stream) {
  if (!x || !mean || !xc || N <= 0 || D <= 0) return MDM_ERR_ARG;
  hipLaunchKernelGGL(mdm::center_kernel, dim3((unsigned)((D + 31) / 32)), dim3(256), 0, (hipStream_t)stream, x, N, D, mean, xc);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
