// Counter-based gaussian noise for the sampler (Philox4x32-10 + Box-Muller), keyed on
//   (seed, GLOBAL sample index, stream id, element index)
// so that x_T and every step's noise are identical however the batch is sharded over GPUs, with O(1) host memory: the
// reference draws th.randn(*shape) / th.randn_like(x) from the process-global generator (gaussian_diffusion.py:1119,1094),
// which ties the sample to the batch composition; SURVEY.md section 8(e) asks for world-size-invariant noise instead.
// The stream id is the timestep t of the step that consumes the noise (read from device memory, so one captured hipGraph
// serves the whole loop) or MDM_NOISE_STREAM_XT for the initial x_T.
// oracle/philox_ref.py restates the generator in numpy; tests compare bit patterns of the uniforms and the normals to 1e-6.
// mdm_diffuse_start is the forward diffusion of a given motion to an intermediate level, out = a*x_start + s*n, in one launch:
// n is drawn in registers on the x_T stream (the values mdm_noise_normal would write) or read from a given buffer, so a
// sample's start is a function of (seed, global sample index) only, whatever the batch split.
#include "kernels.h"
#include "philox.h"

namespace mdm {
namespace {

__global__ void philox_normal_kernel(float* __restrict__ out, int64_t per_sample, int nsamples, int64_t sample0,
                                     const int64_t* __restrict__ sample_ids, uint64_t seed,
                                     const int* __restrict__ stream_dev, int stream_imm) {
  const uint32_t stream = (uint32_t)(stream_dev ? *stream_dev : stream_imm);
  const int64_t quads = (per_sample + 3) >> 2;  // 4 normals per Philox call
  const int64_t total = quads * nsamples;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = i / quads, qd = i - s * quads;
    const uint64_t gs = sample_ids ? (uint64_t)sample_ids[s] : (uint64_t)(sample0 + s);
    float z[4];
    philox_normal4(qd, gs, stream, seed, z);
    float* o = out + s * per_sample + 4 * qd;
    const int64_t left = per_sample - 4 * qd;
    if (left >= 4 && ((((uintptr_t)o) & 15) == 0)) {
      *(f32x4*)o = (f32x4){z[0], z[1], z[2], z[3]};
    } else {
      for (int k = 0; k < 4 && k < left; ++k) o[k] = z[k];
    }
  }
}

// One thread per quad of one sample, the quads of philox_normal_kernel.  out may be x_start (each element is read before it
// is written, by the same thread: no __restrict__ on the two).  VEC: every base pointer 16-byte aligned -> dwordx4 loads and
// stores on the whole quads of every row that starts on a 16-byte boundary; rows that do not (per_sample % 4 != 0) and each
// row's last partial quad go element by element.  a*x + s*n is written out as fma(a, x, s*n): one rounding per product and sum,
// the same in both forms.
template <bool VEC>
__global__ void __launch_bounds__(256) diffuse_start_kernel(const float* x_start, const float* __restrict__ noise, float* out,
                                                            int64_t per_sample, int nsamples, int64_t sample0,
                                                            const int64_t* __restrict__ sample_ids, uint64_t seed, float a,
                                                            float s) {
  const int64_t quads = (per_sample + 3) >> 2;
  const int64_t total = quads * nsamples;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / quads, qd = i - r * quads;
    const int64_t at = r * per_sample + 4 * qd, left = per_sample - 4 * qd;
    const bool whole = left >= 4;
    float z[4];
    if (!noise) {
      const uint64_t gs = sample_ids ? (uint64_t)sample_ids[r] : (uint64_t)(sample0 + r);
      philox_normal4(qd, gs, (uint32_t)MDM_NOISE_STREAM_XT, seed, z);
    }
    if (VEC && whole && (at & 3) == 0) {
      const f32x4 xv = *(const f32x4*)(x_start + at);
      f32x4 nz;
      if (noise) nz = *(const f32x4*)(noise + at);
      else nz = (f32x4){z[0], z[1], z[2], z[3]};
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = fmaf(a, xv[k], s * nz[k]);
      *(f32x4*)(out + at) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)  // unrolled: z stays in registers
        if (k < left) out[at + k] = fmaf(a, x_start[at + k], s * (noise ? noise[at + k] : z[k]));
    }
  }
}

}  // namespace

int philox_normal(float* out, int64_t per_sample, int nsamples, int64_t sample0, const int64_t* sample_ids, uint64_t seed,
                  const int* stream_dev, int stream_imm, hipStream_t s) {
  if (per_sample <= 0 || nsamples <= 0) return MDM_OK;
  if (!out || sample0 < 0) return MDM_ERR_ARG;
  const int64_t total = ((per_sample + 3) >> 2) * nsamples;
  int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, s, out, per_sample,
                     nsamples, sample0, sample_ids, seed, stream_dev, stream_imm);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // namespace mdm

extern "C" int mdm_noise_normal(float* out, int64_t per_sample, int32_t nsamples, int64_t sample0, uint64_t seed,
                                const int32_t* stream_dev, int32_t stream_imm, void* stream) {
  return mdm::philox_normal(out, per_sample, nsamples, sample0, nullptr, seed, stream_dev, stream_imm, (hipStream_t)stream);
}

// the same with an explicit GLOBAL sample index per row (device int64 [nsamples]): rows of a length-bucketed batch
extern "C" int mdm_noise_normal_ids(float* out, int64_t per_sample, int32_t nsamples, const int64_t* sample_ids, uint64_t seed,
                                    const int32_t* stream_dev, int32_t stream_imm, void* stream) {
  if (!sample_ids) return MDM_ERR_ARG;
  return mdm::philox_normal(out, per_sample, nsamples, 0, sample_ids, seed, stream_dev, stream_imm, (hipStream_t)stream);
}

// out[r, e] = a * x_start[r, e] + s * n[r, e]: n from `noise` when given, else the x_T-stream draw of global sample
// sample_ids[r] (when given) or sample0 + r
extern "C" int mdm_diffuse_start(const float* x_start, const float* noise, float* out, int64_t per_sample, int32_t nsamples,
                                 int64_t sample0, const int64_t* sample_ids, uint64_t seed, float a, float s, void* stream) {
  if (!x_start || !out || per_sample < 0 || nsamples < 0 || sample0 < 0) return MDM_ERR_ARG;
  if (!std::isfinite(a) || !std::isfinite(s)) return MDM_ERR_ARG;
  if (per_sample == 0 || nsamples == 0) return MDM_OK;
  const int64_t total = ((per_sample + 3) >> 2) * nsamples;
  const int64_t blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks > 2048 ? 2048 : blocks));
  const bool vec = ((((uintptr_t)x_start) | ((uintptr_t)noise) | ((uintptr_t)out)) & 15) == 0;  // (NULL is aligned)
  if (vec)
    hipLaunchKernelGGL(mdm::diffuse_start_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x_start, noise, out, per_sample,
                       nsamples, sample0, sample_ids, seed, a, s);
  else
    hipLaunchKernelGGL(mdm::diffuse_start_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x_start, noise, out,
                       per_sample, nsamples, sample0, sample_ids, seed, a, s);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}
