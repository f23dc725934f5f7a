// Stand weights of the terrain term from the foot-contact columns of a step's x0: which joints the
// guidance pulls down onto the ground.  The last four columns of a feature row are the contact labels of the skeleton's four
// foot joints; a label is de-normalised as the postprocess does (one fp32 multiply, one fp32 add, not fused) and compared
// with a threshold.  One thread per (frame, joint): out[frame, joint] = 1 at a foot joint whose label exceeds the threshold,
// 0 at every other joint.  Elementwise and allocation free: it runs inside graph capture in front of the guidance.
#include "kernels.h"

#include <cmath>

namespace mdm {
namespace {

constexpr int STAND_THREADS = 256;

struct Feet {
  int joint[4];
};

__global__ __launch_bounds__(STAND_THREADS) void terrain_stand_kernel(const float* __restrict__ x0, const int* __restrict__ frows,
                                                                      int64_t n, const float* __restrict__ mean,
                                                                      const float* __restrict__ sd, int F, int J, int group, Feet feet,
                                                                      float threshold, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * STAND_THREADS + threadIdx.x;
  if (i >= n * J) return;
  const int64_t f = i / J;
  const int j = (int)(i - f * J);
  const int64_t row = frows ? frows[f] : f;
  const int64_t st = group ? (f / group) * F : 0;  // the frame's row of mean / std
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (feet.joint[k] != j) continue;
    const int c = F - 4 + k;
    if (__fadd_rn(__fmul_rn(x0[row * F + c], sd[st + c]), mean[st + c]) > threshold) s = 1.f;
  }
  out[i] = s;
}

}  // namespace
}  // namespace mdm

extern "C" int mdm_terrain_stand_weights(const float* x0, const int32_t* frame_rows, int32_t n_frames, const float* mean,
                                         const float* std, int32_t F, int32_t stat_group, const int32_t* feet, float threshold,
                                         float* out, void* stream) {
  if (!x0 || !mean || !std || !feet || !out || n_frames < 0 || stat_group < 0 || !std::isfinite(threshold)) return MDM_ERR_ARG;
  const int J = (F + 1) % 12 == 0 && F >= 11 ? (F + 1) / 12 : 0;
  if (J == 0) return MDM_ERR_ARG;
  mdm::Feet ft;
  for (int k = 0; k < 4; ++k) {
    if (feet[k] < 0 || feet[k] >= J) return MDM_ERR_ARG;
    ft.joint[k] = feet[k];
  }
  if (n_frames == 0) return MDM_OK;
  const int64_t blocks = ((int64_t)n_frames * J + mdm::STAND_THREADS - 1) / mdm::STAND_THREADS;
  hipLaunchKernelGGL(mdm::terrain_stand_kernel, dim3((unsigned)blocks), dim3(mdm::STAND_THREADS), 0, (hipStream_t)stream, x0,
                     frame_rows, (int64_t)n_frames, mean, std, F, J, stat_group, ft, threshold, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}
