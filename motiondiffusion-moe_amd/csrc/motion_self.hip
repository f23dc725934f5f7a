// Self-collision avoidance: keep a character's joints out of the capsules of its own bones.  With the bones held
// fixed ("records are data"), the loss a Σ u_j Σ_i max(0, m + r_j + ρ_i − d_i)² has the gradient −2 a u_j Σ_i pen_i n_i at P[t, j],
// which is the gradient of §14's target term w |P − g|² at g = P + Σ_i pen_i n_i, w = a u_j.  So a producer in front of the
// unchanged guidance writes those targets and weights on every step, as §31's producer writes tracks:
//   1., 2. step_joints (motion_partners.hip): P = postprocess.recover_from_ric(x0 · std + mean), bit for bit;
//   3. self_push_kernel: one thread per (frame, joint), FRAMES frames per workgroup, a frame's joints in LDS, the bone loop
//      reading LDS in ascending bone order (a fixed order: the same bits run after run), and the merge with the user's static
//      targets fused into the store.
// mdm_self_push is launch 3 alone on given joints, with the push and the depth as outputs: the same kernel, hence the same bits.
// No atomics, no allocation, stream-ordered, graph-capturable.
#include "joint_control.h"
#include "kernels.h"

#include <cmath>

namespace mdm {
namespace {

constexpr int LANES = 32, FRAMES = 8, THREADS = LANES * FRAMES;  // a joint a lane: J <= 32
constexpr int MAX_BONES = 31;                                     // a bit of an int32 mask per bone

struct SelfBones {
  int32_t uv[MAX_BONES];  // u | v << 8
};

// merge == 0: out3 = push, out1 = depth (or NULL), (B, T, J, 3) / (B, T, J).  merge == 1: out3 = targets, outw = weights, both
// (B, T, J, 3), with the static pair (or NULL) winning wherever one of its three weights is not zero.
__global__ __launch_bounds__(THREADS) void self_push_kernel(const float* __restrict__ joints, const int* __restrict__ len,
                                                            SelfBones bones, int nb, const float* __restrict__ bone_radius,
                                                            const float* __restrict__ joint_params,
                                                            const int* __restrict__ pair_mask, float margin, float weight,
                                                            const float* __restrict__ static_targets,
                                                            const float* __restrict__ static_weights, int merge, int64_t frames,
                                                            int T, int J, float* __restrict__ out3, float* __restrict__ out1,
                                                            float* __restrict__ outw) {
#pragma clang fp contract(off)
  __shared__ float sh[FRAMES * LANES * 3];
  const int f = threadIdx.x / LANES, j = threadIdx.x - f * LANES;
  const int64_t fr = (int64_t)blockIdx.x * FRAMES + f;
  const bool own = fr < frames && j < J;
  bool valid = false;
  if (own) {
    const int64_t b = fr / T;
    const int t = (int)(fr - b * T);
    int n = len[b];
    n = n < 0 ? 0 : (n > T ? T : n);
    valid = t < n;
  }
  const int64_t at = (fr * J + j) * 3;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (valid) px = joints[at], py = joints[at + 1], pz = joints[at + 2];
  float* mine = sh + (f * LANES + j) * 3;
  mine[0] = px, mine[1] = py, mine[2] = pz;
  __syncthreads();
  float sx = 0.f, sy = 0.f, sz = 0.f, depth = 0.f;
  if (valid) {
    const int allowed = pair_mask[j];
    const float reach = margin + joint_params[2 * j];
    const float* fj = sh + f * LANES * 3;
    for (int i = 0; i < nb; ++i) {
      if (!((allowed >> i) & 1)) continue;
      const int uv = bones.uv[i];
      const float* a = fj + (uv & 255) * 3;
      const float* e = fj + (uv >> 8) * 3;
      const float ax = a[0], ay = a[1], az = a[2];
      const float ex = e[0] - ax, ey = e[1] - ay, ez = e[2] - az;
      const float vx = px - ax, vy = py - ay, vz = pz - az;
      const float ee = ex * ex + ey * ey + ez * ez;
      float h = ee > 0.f ? (vx * ex + vy * ey + vz * ez) / ee : 0.f;
      h = fminf(fmaxf(h, 0.f), 1.f);
      const float dx = vx - h * ex, dy = vy - h * ey, dz = vz - h * ez;
      const float d = sqrtf(dx * dx + dy * dy + dz * dz);
      const float pen = reach + bone_radius[i] - d;
      if (pen > 0.f) {
        depth += pen;
        if (d >= 1e-12f) {  // the jump set: no direction on the axis itself
          const float s = pen / d;
          sx += s * dx, sy += s * dy, sz += s * dz;
        }
      }
    }
  }
  if (!own) return;
  if (!merge) {
    out3[at] = sx, out3[at + 1] = sy, out3[at + 2] = sz;
    if (out1) out1[fr * J + j] = depth;
    return;
  }
  float gx = 0.f, gy = 0.f, gz = 0.f, wx = 0.f, wy = 0.f, wz = 0.f;
  bool user = false;
  if (static_weights) {
    wx = static_weights[at], wy = static_weights[at + 1], wz = static_weights[at + 2];
    user = !valid || wx != 0.f || wy != 0.f || wz != 0.f;
    if (user) gx = static_targets[at], gy = static_targets[at + 1], gz = static_targets[at + 2];
  }
  if (valid && !user) {
    const float w = depth > 0.f ? weight * joint_params[2 * j + 1] : 0.f;
    gx = px + sx, gy = py + sy, gz = pz + sz;
    wx = wy = wz = w;
  }
  out3[at] = gx, out3[at + 1] = gy, out3[at + 2] = gz;
  outw[at] = wx, outw[at + 1] = wy, outw[at + 2] = wz;
}

// the host checks both entries share; bones (nb, 2) in host memory
int self_args(const int32_t* bones, int nb, const float* bone_radius, const float* joint_params, const int32_t* pair_mask,
              float margin, int B, int T, int J, SelfBones& out) {
  if (!bones || !bone_radius || !joint_params || !pair_mask || B < 0 || T < 0) return MDM_ERR_ARG;
  if (J < 2 || J > LANES || nb < 1 || nb > MAX_BONES || !std::isfinite(margin)) return MDM_ERR_ARG;
  for (int i = 0; i < nb; ++i) {
    const int u = bones[2 * i], v = bones[2 * i + 1];
    if (u < 0 || u >= J || v < 0 || v >= J) return MDM_ERR_ARG;
    out.uv[i] = u | (v << 8);
  }
  return MDM_OK;
}

int self_launch(const float* joints, const int32_t* length, const SelfBones& bn, int nb, const float* bone_radius,
                const float* joint_params, const int32_t* pair_mask, float margin, float weight, const float* static_targets,
                const float* static_weights, int merge, int B, int T, int J, float* out3, float* out1, float* outw,
                hipStream_t s) {
  const int64_t frames = (int64_t)B * T;
  hipLaunchKernelGGL(self_push_kernel, dim3((unsigned)((frames + FRAMES - 1) / FRAMES)), dim3(THREADS), 0, s, joints, length, bn, nb,
                     bone_radius, joint_params, pair_mask, margin, weight, static_targets, static_weights, merge, frames, T, J, out3,
                     out1, outw);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // namespace
}  // namespace mdm

extern "C" int mdm_self_max_frames(void) { return mdm_partner_tracks_max_frames(); }

extern "C" int64_t mdm_self_targets_scratch_floats(int32_t B, int32_t T, int32_t F) {
  const int64_t J = mdm::control::control_joints(F);
  if (B < 0 || T < 0 || J == 0) return 0;
  return mdm::step_joints_scratch_floats(B, T, J);
}

extern "C" int mdm_self_push(const float* joints, const int32_t* length, const int32_t* bones, int32_t nb, const float* bone_radius,
                             const float* joint_params, const int32_t* pair_mask, float margin, int32_t B, int32_t T, int32_t J,
                             float* push_out, float* depth_out, void* stream) {
  if (!joints || !length || !push_out) return MDM_ERR_ARG;
  mdm::SelfBones bn = {};
  const int st = mdm::self_args(bones, nb, bone_radius, joint_params, pair_mask, margin, B, T, J, bn);
  if (st != MDM_OK) return st;
  if (B == 0 || T == 0) return MDM_OK;
  return mdm::self_launch(joints, length, bn, nb, bone_radius, joint_params, pair_mask, margin, 0.f, nullptr, nullptr, 0, B, T, J,
                          push_out, depth_out, nullptr, (hipStream_t)stream);
}

extern "C" int mdm_self_targets(const float* x0, const int32_t* length, const float* mean, const float* std, const int32_t* bones,
                                int32_t nb, const float* bone_radius, const float* joint_params, const int32_t* pair_mask,
                                float margin, float weight, const float* static_targets, const float* static_weights, int32_t B,
                                int32_t T, int32_t F, float* joints_out, float* scratch, float* targets_out, float* weights_out,
                                void* stream) {
  if (!x0 || !length || !mean || !std || !joints_out || !scratch || !targets_out || !weights_out) return MDM_ERR_ARG;
  if ((static_targets == nullptr) != (static_weights == nullptr)) return MDM_ERR_ARG;
  const int J = mdm::control::control_joints(F);
  if (J == 0) return MDM_ERR_ARG;
  if (!(std::isfinite(weight) && weight >= 0.f)) return MDM_ERR_ARG;
  mdm::SelfBones bn = {};
  int st = mdm::self_args(bones, nb, bone_radius, joint_params, pair_mask, margin, B, T, J, bn);
  if (st != MDM_OK) return st;
  if (B == 0 || T == 0) return MDM_OK;
  if (T > mdm_self_max_frames()) return MDM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  st = mdm::step_joints(x0, length, mean, std, B, T, F, J, scratch, joints_out, s);
  if (st != MDM_OK) return st;
  return mdm::self_launch(joints_out, length, bn, nb, bone_radius, joint_params, pair_mask, margin, weight, static_targets,
                          static_weights, 1, B, T, J, targets_out, nullptr, weights_out, s);
}
