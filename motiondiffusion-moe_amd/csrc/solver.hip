// Few-step samplers on a respaced schedule (diffusion.py: SpacedDiffusion, ddim_sample_loop_with_cfg,
// dpm_solver_sample_loop_with_cfg).  Two launches per step besides the forward:
//   fill_mapped:    ts[r] = timestep_map[*t_dev]  -- the denoiser sees the ORIGINAL timestep of the spaced step
//   guided_update:  x0 = guide(x0_c, x0_u) in x0 space, then x_out = cx*x + c0*x0 + c1*x0_prev + cn*noise, x0_out = x0
// Both read the step counter from device memory, so one captured hipGraph serves the whole loop.  The per-step
// coefficients {cx, c0, c1, cn} are tabulated on the host in f64 and rounded to f32 (GaussianDiffusion.solver_coefficients):
// guided DDIM at any eta and DPM-Solver++(2M) share this one kernel and differ only in the table.
// Motion editing (mdm_guided_update_inpaint) replaces the guided x0 by (1 - m)*x0 + m*k before the update, with the known
// motion k and the mask m dense [n]: two more reads per element, in a second instantiation of the same kernel.
// Composed guidance (mdm_composed_update) takes K conditions instead of one: x0 = x0_u + s * sum_k w_k (x0_k - x0_u) under
// dense per-prompt weights, then the same (optionally edited) update.
#include "kernels.h"

namespace mdm {
namespace {

__global__ void fill_mapped_kernel(int64_t* __restrict__ dst, int64_t n, const int* __restrict__ t_ptr,
                                   const int64_t* __restrict__ map, int ts) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) dst[i] = map[min(max(*t_ptr, 0), ts - 1)];  // a stale device counter must not index outside the map
}

// x / x_out and x0_prev / x0_out may be the same buffers (in-place update): each element is read before it is written,
// by the same thread, so those four carry no __restrict__.  VEC: every pointer 16-byte aligned -> dwordx4 loads / stores
// on whole quads; the last quad of an n that is not a multiple of 4 is done element by element.  EDIT: known / mask are
// read and the guided x0 is replaced on the masked entries (known is data: never clamped); without it they are not touched.
template <bool VEC, bool EDIT>
__global__ void __launch_bounds__(256) guided_update_kernel(
    const float* x, const float* __restrict__ eps_c, const float* __restrict__ eps_u, const float* x0_prev,
    const float* __restrict__ noise, const float* __restrict__ known, const float* __restrict__ mask, int64_t n,
    const float* __restrict__ tab, const float* __restrict__ coef, int ts, const int* __restrict__ t_ptr, int t_imm,
    float cfg_scale, int clip, float* x_out, float* x0_out) {
  int t = t_ptr ? *t_ptr : t_imm;
  t = min(max(t, 0), ts - 1);
  const float a = tab[TAB_SQRT_RECIP * ts + t], b = tab[TAB_SQRT_RECIPM1 * ts + t];
  const float cx = coef[4 * t], c0 = coef[4 * t + 1];
  const float c1 = x0_prev ? coef[4 * t + 2] : 0.f, cn = noise ? coef[4 * t + 3] : 0.f;
  // c1 == 0 (first and last DPM-Solver++ steps, every DDIM step) skips the x0_prev read: its buffer may hold anything then
  const bool use_prev = c1 != 0.f, use_noise = cn != 0.f;
  auto one = [&](float xv, float ec, float eu, float xp, float nz, float kv, float mv, float& xo) {
    float x0 = a * xv - b * ec;
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    if (eps_u) {  // classifier-free guidance on pred_xstart (gaussian_diffusion.py:1075-1091)
      float x0u = a * xv - b * eu;
      if (clip) x0u = fminf(fmaxf(x0u, -1.f), 1.f);
      x0 = x0u + cfg_scale * (x0 - x0u);
    }
    // m = 0 gives x0 and m = 1 gives k exactly (finite operands), with or without fma contraction
    if (EDIT) x0 = (1.f - mv) * x0 + mv * kv;
    float y = cx * xv + c0 * x0;
    if (use_prev) y += c1 * xp;
    if (use_noise) y += cn * nz;
    xo = y;
    return x0;
  };
  const int64_t quads = (n + 3) >> 2;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 4 * q;
    if (VEC && i + 4 <= n) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const f32x4 xv = *(const f32x4*)(x + i), ec = *(const f32x4*)(eps_c + i);
      const f32x4 eu = eps_u ? *(const f32x4*)(eps_u + i) : z;
      const f32x4 xp = use_prev ? *(const f32x4*)(x0_prev + i) : z;
      const f32x4 nz = use_noise ? *(const f32x4*)(noise + i) : z;
      const f32x4 kv = EDIT ? *(const f32x4*)(known + i) : z, mv = EDIT ? *(const f32x4*)(mask + i) : z;
      f32x4 xo, x0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float o;
        x0[k] = one(xv[k], ec[k], eu[k], xp[k], nz[k], kv[k], mv[k], o);
        xo[k] = o;
      }
      *(f32x4*)(x_out + i) = xo;
      if (x0_out) *(f32x4*)(x0_out + i) = x0;
    } else {
      for (int64_t j = i; j < i + 4 && j < n; ++j) {
        float o;
        const float x0 = one(x[j], eps_c[j], eps_u ? eps_u[j] : 0.f, use_prev ? x0_prev[j] : 0.f,
                             use_noise ? noise[j] : 0.f, EDIT ? known[j] : 0.f, EDIT ? mask[j] : 0.f, o);
        x_out[j] = o;
        if (x0_out) x0_out[j] = x0;
      }
    }
  }
}

// K condition blocks of eps, then the unconditional block: eps + k*n, eps + K*n; weights w + k*n.  K = 1 with w = 1 is
// guided_update_kernel bit for bit: contraction is off here and every fma is written out, in the rounding that kernel
// compiles to on gfx950 (x0_c = a*x - b*eps with both products rounded, x0_u = fma(-b, eps_u, a*x), x0 = fma(s, x0_c - x0_u,
// x0_u), the edit blend fma(m, k, (1 - m)*x0), y = cx*x + c0*x0 then one fma per further term); the sum over prompts
// starts from its first term, and w*d is d at w = 1.  VEC: every pointer 16-byte aligned and n % 4 == 0 (so every block is
// aligned too).  In-place rules, EDIT and the skipped zero-coefficient reads are those of guided_update_kernel.
template <bool VEC, bool EDIT>
__global__ void __launch_bounds__(256) composed_update_kernel(
    const float* x, const float* __restrict__ eps, int K, const float* __restrict__ w, const float* x0_prev,
    const float* __restrict__ noise, const float* __restrict__ known, const float* __restrict__ mask, int64_t n,
    const float* __restrict__ tab, const float* __restrict__ coef, int ts, const int* __restrict__ t_ptr, int t_imm,
    float cfg_scale, int clip, float* x_out, float* x0_out) {
#pragma clang fp contract(off)
  int t = t_ptr ? *t_ptr : t_imm;
  t = min(max(t, 0), ts - 1);
  const float a = tab[TAB_SQRT_RECIP * ts + t], b = tab[TAB_SQRT_RECIPM1 * ts + t];
  const float cx = coef[4 * t], c0 = coef[4 * t + 1];
  const float c1 = x0_prev ? coef[4 * t + 2] : 0.f, cn = noise ? coef[4 * t + 3] : 0.f;
  const bool use_prev = c1 != 0.f, use_noise = cn != 0.f;
  const float* eps_u = eps + (int64_t)K * n;
  auto lim = [&](float v) { return clip ? fminf(fmaxf(v, -1.f), 1.f) : v; };
  auto finish = [&](float xv, float x0u, float acc, float xp, float nz, float kv, float mv, float& xo) {
    float x0 = fmaf(cfg_scale, acc, x0u);
    if (EDIT) x0 = fmaf(mv, kv, (1.f - mv) * x0);
    float y = cx * xv + c0 * x0;
    if (use_prev) y = fmaf(c1, xp, y);
    if (use_noise) y = fmaf(cn, nz, y);
    xo = y;
    return x0;
  };
  const int64_t quads = (n + 3) >> 2;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 4 * q;
    if (VEC && i + 4 <= n) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const f32x4 xv = *(const f32x4*)(x + i), eu = *(const f32x4*)(eps_u + i);
      f32x4 ax, x0u, acc;
      {
        const f32x4 e = *(const f32x4*)(eps + i), wk = *(const f32x4*)(w + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ax[j] = a * xv[j];
          x0u[j] = lim(fmaf(-b, eu[j], ax[j]));
          acc[j] = wk[j] * (lim(ax[j] - b * e[j]) - x0u[j]);
        }
      }
      for (int k = 1; k < K; ++k) {
        const f32x4 e = *(const f32x4*)(eps + k * n + i), wk = *(const f32x4*)(w + k * n + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk[j], lim(ax[j] - b * e[j]) - x0u[j], acc[j]);
      }
      const f32x4 xp = use_prev ? *(const f32x4*)(x0_prev + i) : z;
      const f32x4 nz = use_noise ? *(const f32x4*)(noise + i) : z;
      const f32x4 kv = EDIT ? *(const f32x4*)(known + i) : z, mv = EDIT ? *(const f32x4*)(mask + i) : z;
      f32x4 xo, x0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float o;
        x0[j] = finish(xv[j], x0u[j], acc[j], xp[j], nz[j], kv[j], mv[j], o);
        xo[j] = o;
      }
      *(f32x4*)(x_out + i) = xo;
      if (x0_out) *(f32x4*)(x0_out + i) = x0;
    } else {
      for (int64_t j = i; j < i + 4 && j < n; ++j) {
        const float xv = x[j], ax = a * xv, x0u = lim(fmaf(-b, eps_u[j], ax));
        float acc = w[j] * (lim(ax - b * eps[j]) - x0u);
        for (int k = 1; k < K; ++k) acc = fmaf(w[k * n + j], lim(ax - b * eps[k * n + j]) - x0u, acc);
        float o;
        const float x0 = finish(xv, x0u, acc, use_prev ? x0_prev[j] : 0.f, use_noise ? noise[j] : 0.f,
                                EDIT ? known[j] : 0.f, EDIT ? mask[j] : 0.f, o);
        x_out[j] = o;
        if (x0_out) x0_out[j] = x0;
      }
    }
  }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

template <bool EDIT>
int launch_guided_update(const float* x, const float* eps_c, const float* eps_u, const float* x0_prev, const float* noise,
                         const float* known, const float* mask, int64_t n, const float* tab, const float* coef,
                         int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale, int32_t clip_denoised,
                         float* x_out, float* x0_out, void* stream) {
  if (!x || !eps_c || !tab || !coef || !x_out || n < 0 || steps <= 0) return MDM_ERR_ARG;
  if (EDIT && (!known || !mask)) return MDM_ERR_ARG;
  if (!t_dev && (t_imm < 0 || t_imm >= steps)) return MDM_ERR_ARG;
  if (n == 0) return MDM_OK;
  const bool vec = aligned16(x) && aligned16(eps_c) && aligned16(eps_u) && aligned16(x0_prev) && aligned16(noise) &&
                   aligned16(known) && aligned16(mask) && aligned16(x_out) && aligned16(x0_out);  // (NULL is aligned)
  const int64_t blocks = (((n + 3) >> 2) + 255) / 256;
  const dim3 grid((unsigned)(blocks > 2048 ? 2048 : blocks));
  if (vec)
    hipLaunchKernelGGL((guided_update_kernel<true, EDIT>), grid, dim3(256), 0, (hipStream_t)stream, x, eps_c, eps_u,
                       x0_prev, noise, known, mask, n, tab, coef, steps, t_dev, t_imm, cfg_scale, clip_denoised, x_out,
                       x0_out);
  else
    hipLaunchKernelGGL((guided_update_kernel<false, EDIT>), grid, dim3(256), 0, (hipStream_t)stream, x, eps_c, eps_u,
                       x0_prev, noise, known, mask, n, tab, coef, steps, t_dev, t_imm, cfg_scale, clip_denoised, x_out,
                       x0_out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

template <bool EDIT>
void launch_composed(dim3 grid, bool vec, const float* x, const float* eps, int32_t K, const float* w, const float* x0_prev,
                     const float* noise, const float* known, const float* mask, int64_t n, const float* tab,
                     const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale, int32_t clip,
                     float* x_out, float* x0_out, hipStream_t stream) {
  if (vec)
    hipLaunchKernelGGL((composed_update_kernel<true, EDIT>), grid, dim3(256), 0, stream, x, eps, K, w, x0_prev, noise,
                       known, mask, n, tab, coef, steps, t_dev, t_imm, cfg_scale, clip, x_out, x0_out);
  else
    hipLaunchKernelGGL((composed_update_kernel<false, EDIT>), grid, dim3(256), 0, stream, x, eps, K, w, x0_prev, noise,
                       known, mask, n, tab, coef, steps, t_dev, t_imm, cfg_scale, clip, x_out, x0_out);
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_fill_timesteps_mapped(int64_t* dst, int64_t n, const int32_t* t_dev, const int64_t* map, int32_t steps,
                              void* stream) {
  if (!dst || !t_dev || !map || n < 0 || steps <= 0) return MDM_ERR_ARG;
  if (n == 0) return MDM_OK;
  hipLaunchKernelGGL(mdm::fill_mapped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, n,
                     t_dev, map, steps);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int mdm_guided_update(const float* x, const float* eps_c, const float* eps_u, const float* x0_prev, const float* noise,
                      int64_t n, const float* tab, const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm,
                      float cfg_scale, int32_t clip_denoised, float* x_out, float* x0_out, void* stream) {
  return mdm::launch_guided_update<false>(x, eps_c, eps_u, x0_prev, noise, nullptr, nullptr, n, tab, coef, steps, t_dev,
                                          t_imm, cfg_scale, clip_denoised, x_out, x0_out, stream);
}

int mdm_guided_update_inpaint(const float* x, const float* eps_c, const float* eps_u, const float* x0_prev,
                              const float* noise, const float* known, const float* mask, int64_t n, const float* tab,
                              const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale,
                              int32_t clip_denoised, float* x_out, float* x0_out, void* stream) {
  return mdm::launch_guided_update<true>(x, eps_c, eps_u, x0_prev, noise, known, mask, n, tab, coef, steps, t_dev, t_imm,
                                         cfg_scale, clip_denoised, x_out, x0_out, stream);
}

int mdm_composed_update(const float* x, const float* eps, int32_t nconds, const float* weights, const float* x0_prev,
                        const float* noise, const float* known, const float* mask, int64_t n, const float* tab,
                        const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, float cfg_scale,
                        int32_t clip_denoised, float* x_out, float* x0_out, void* stream) {
  if (!x || !eps || !weights || !tab || !coef || !x_out || n < 0 || steps <= 0) return MDM_ERR_ARG;
  if (nconds < 1 || nconds > MDM_COMPOSE_MAX_K) return MDM_ERR_ARG;
  if (!known != !mask) return MDM_ERR_ARG;
  if (!t_dev && (t_imm < 0 || t_imm >= steps)) return MDM_ERR_ARG;
  if (n == 0) return MDM_OK;
  using mdm::aligned16;
  const bool vec = n % 4 == 0 && aligned16(x) && aligned16(eps) && aligned16(weights) && aligned16(x0_prev) &&
                   aligned16(noise) && aligned16(known) && aligned16(mask) && aligned16(x_out) && aligned16(x0_out);
  const int64_t blocks = (((n + 3) >> 2) + 255) / 256;
  const dim3 grid((unsigned)(blocks > 2048 ? 2048 : blocks));
  if (known)
    mdm::launch_composed<true>(grid, vec, x, eps, nconds, weights, x0_prev, noise, known, mask, n, tab, coef, steps, t_dev,
                               t_imm, cfg_scale, clip_denoised, x_out, x0_out, (hipStream_t)stream);
  else
    mdm::launch_composed<false>(grid, vec, x, eps, nconds, weights, x0_prev, noise, nullptr, nullptr, n, tab, coef, steps,
                                t_dev, t_imm, cfg_scale, clip_denoised, x_out, x0_out, (hipStream_t)stream);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
