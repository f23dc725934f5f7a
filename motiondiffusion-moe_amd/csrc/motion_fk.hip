// Joints from rotations on the device: forward kinematics of the rot6d columns of HumanML3D / KIT rows.
// (T, 12 J - 1) normalised rows -> (T, J, 3) joint positions on fixed bone offsets, and the (T, J, 3, 3) global rotations.
//   de-normalise, root Y rotation and XZ path as motion_post.hip (recover_root_rot_pos)   utils/motion_process.py:362-382
//   recover_from_rot: root quaternion -> cont6d, joined with the rot6d columns            utils/motion_process.py:384-398
//   forward_kinematics_cont6d down the kinematic chains                                   utils/skeleton.py:173-194
//   quaternion_to_matrix / quaternion_to_cont6d / cont6d_to_matrix                        utils/quaternion.py:274-336
// Kept as the reference has it: every chain starts its accumulated rotation from the ROOT matrix, also the chains that
// start at another joint (the two arm chains take spine3's position, not its rotation), and cont6d_to_matrix has no clamp
// and no epsilon: a zero x_raw or an x_raw parallel to y_raw gives non-finite joints down that frame's chain.
// One workgroup per sample.  The de-normalised rotation velocity is staged in LDS by all threads, one thread turns it into
// the heading (double accumulator rounded to fp32 per element: torch.cumsum on fp32 CPU tensors), all threads take cos / sin
// and the rotated root velocity, two threads (one per wave) prefix-sum X and Z.  Forward kinematics: one thread per (frame,
// chain), chains grouped in levels by the host: level 0 starts at the root, level k at a joint a chain of level k - 1 wrote;
// a workgroup barrier separates the levels, so a chain reads its start position only after it was stored.  Without offsets
// the sample's own are made first: per bone the mean over the valid frames of its length on the recover_from_ric joints
// (fp32 per frame, summed in double in frame order), times the bone's axis.  fp32 in the reference's operation order with
// contraction off.  HBM-bound and tiny (B x T x (12 J - 1) floats in, B x T x 12 J out).
#pragma clang fp contract(off)
#include "kernels.h"
#include "motion_root.h"

namespace mdm {
namespace {

constexpr int FK_THREADS = 256;
constexpr int FK_MAX_FRAMES = 3200;  // 5 floats of LDS per frame: 62.5 KiB beside the offsets, under 64 KiB

struct FkArg {
  MdmSkeleton s;
  int parent[MDM_SKEL_MAX_JOINTS];
  int order[MDM_SKEL_MAX_CHAINS];            // chains sorted by level
  int level_start[MDM_SKEL_MAX_CHAINS + 1];  // level l: order[level_start[l] .. level_start[l + 1])
  int nlevels;
};

struct M3 { float m[3][3]; };

// cont6d_to_matrix (quaternion.py:320-336): columns x = x_raw / |x_raw|, y = z x x, z = (x x y_raw) / |x x y_raw|
__device__ __forceinline__ M3 cont6d_matrix(float a0, float a1, float a2, float b0, float b1, float b2) {
  const float nx = __fsqrt_rn(a0 * a0 + a1 * a1 + a2 * a2);
  const float x0 = __fdiv_rn(a0, nx), x1 = __fdiv_rn(a1, nx), x2 = __fdiv_rn(a2, nx);
  float z0 = x1 * b2 - x2 * b1, z1 = x2 * b0 - x0 * b2, z2 = x0 * b1 - x1 * b0;
  const float nz = __fsqrt_rn(z0 * z0 + z1 * z1 + z2 * z2);
  z0 = __fdiv_rn(z0, nz), z1 = __fdiv_rn(z1, nz), z2 = __fdiv_rn(z2, nz);
  const float y0 = z1 * x2 - z2 * x1, y1 = z2 * x0 - z0 * x2, y2 = z0 * x1 - z1 * x0;
  return {{{x0, y0, z0}, {x1, y1, z1}, {x2, y2, z2}}};
}

// the root's matrix: quaternion (c, 0, s, 0) -> first two columns of quaternion_to_matrix (:283-296) -> cont6d_to_matrix
__device__ __forceinline__ M3 root_matrix(float c, float s) {
  const float r = c, i = 0.f, j = s, k = 0.f;
  const float two_s = __fdiv_rn(2.f, r * r + i * i + j * j + k * k);
  return cont6d_matrix(1.f - two_s * (j * j + k * k), two_s * (i * j + k * r), two_s * (i * k - j * r),
                       two_s * (i * j - k * r), 1.f - two_s * (i * i + k * k), two_s * (j * k + i * r));
}

__device__ __forceinline__ M3 matmul(const M3& a, const M3& b) {
  M3 o;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o.m[r][c] = a.m[r][0] * b.m[0][c] + a.m[r][1] * b.m[1][c] + a.m[r][2] * b.m[2][c];
  return o;
}

__device__ __forceinline__ void put_matrix(float* o, const M3& a) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[3 * r + c] = a.m[r][c];
}

__global__ __launch_bounds__(FK_THREADS) void motion_fk_kernel(
    const float* __restrict__ x, const int* __restrict__ len, const float* __restrict__ mean, const float* __restrict__ sd,
    const FkArg sk, const float* __restrict__ offs, int64_t off_stride, int T, int radius, const double* __restrict__ wts,
    float* raw, float* out, float* __restrict__ rot, float* __restrict__ offs_out) {
  extern __shared__ float sh[];  // cw[T], sw[T], px[T], pz[T], py[T]
  __shared__ float soff[MDM_SKEL_MAX_JOINTS * 3];
  float* cw = sh;
  float* sw = cw + T;
  float* px = sw + T;
  float* pz = px + T;
  float* py = pz + T;
  const MdmSkeleton& S = sk.s;
  const int J = S.joints, W = 3 * J, F = 12 * J - 1;
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = len ? len[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const float* xb = x + (int64_t)b * T * F;
  // de-normalised with two roundings, as the reference's numpy expression: the rows it is handed are fp32
  auto val = [&](int t, int c) { return xb[(int64_t)t * F + c] * sd[c] + mean[c]; };

  // heading: exclusive prefix sum of the rotation velocity (:364-367), in motion_post_kernel's order
  for (int t = tid; t < n; t += FK_THREADS) cw[t] = val(t, 0);
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int t = 0; t < n; ++t) {
      const float v = cw[t];
      cw[t] = (float)acc;
      acc += (double)v;
    }
  }
  __syncthreads();
  // cos / sin, and the previous frame's root velocity rotated by the inverse rotation (:373-376)
  for (int t = tid; t < n; t += FK_THREADS) {
    const float a = cw[t];
    const float c = cosf(a), s = sinf(a);
    float vx = 0.f, vz = 0.f;
    if (t > 0) vx = val(t - 1, 1), vz = val(t - 1, 2);
    float ox, oy, oz;
    rot_y(c, -s, vx, 0.f, vz, ox, oy, oz);
    cw[t] = c, sw[t] = s, px[t] = ox, pz[t] = oz, py[t] = val(t, 3);
  }
  __syncthreads();
  // root XZ: prefix sums (:378), X and Z in one thread each of two waves
  if (tid == 0 || tid == 64) {
    float* p = tid == 0 ? px : pz;
    double acc = 0.0;
    for (int t = 0; t < n; ++t) {
      acc += (double)p[t];
      p[t] = (float)acc;
    }
  }
  __syncthreads();

  float* rb = raw ? raw + (int64_t)b * T * W : nullptr;
  if (offs) {
    for (int i = tid; i < W; i += FK_THREADS) soff[i] = offs[(int64_t)b * off_stride + i];
  } else {
    // this sample's own offsets: bone lengths on the recover_from_ric joints (:403-416), fp32 per frame -> rb as [J][T]
    auto ric = [&](int t, int j, float& ox, float& oy, float& oz) {
      if (j == 0) {
        ox = px[t], oy = py[t], oz = pz[t];
      } else {
        const int c = 4 + 3 * (j - 1);
        rot_y(cw[t], -sw[t], val(t, c), val(t, c + 1), val(t, c + 2), ox, oy, oz);
        ox = add(ox, px[t]), oz = add(oz, pz[t]);
      }
    };
    for (int i = tid; i < n * (J - 1); i += FK_THREADS) {
      const int t = i / (J - 1), j = 1 + i - t * (J - 1);
      float ax, ay, az, bx, by, bz;
      ric(t, j, ax, ay, az);
      ric(t, sk.parent[j], bx, by, bz);
      const float dx = ax - bx, dy = ay - by, dz = az - bz;
      rb[(int64_t)j * T + t] = __fsqrt_rn(dx * dx + dy * dy + dz * dz);
    }
    __syncthreads();
    if (tid < J) {
      double acc = 0.0;
      for (int t = 0; t < n; ++t) acc += (double)rb[(int64_t)tid * T + t];
      const float m = (tid > 0 && n > 0) ? (float)(acc / (double)n) : 0.f;
      for (int k = 0; k < 3; ++k) soff[3 * tid + k] = m * S.raw_offsets[3 * tid + k];
    }
  }
  __syncthreads();  // the offsets are in LDS; the bone lengths in rb have been read
  if (offs_out)
    for (int i = tid; i < W; i += FK_THREADS) offs_out[(int64_t)b * W + i] = soff[i];

  // forward kinematics (skeleton.py:184-193); unfiltered joints go straight to the output
  float* dst = radius > 0 ? rb : out + (int64_t)b * T * W;
  float* rotb = rot ? rot + (int64_t)b * T * J * 9 : nullptr;
  const int c_rot = 4 + 3 * (J - 1);
  for (int lvl = 0; lvl < sk.nlevels; ++lvl) {
    const int first = sk.level_start[lvl], nc = sk.level_start[lvl + 1] - first;
    for (int i = tid; i < n * nc; i += FK_THREADS) {
      const int t = i / nc, ch = sk.order[first + i - t * nc];
      float* fr = dst + (int64_t)t * W;
      float* rf = rotb ? rotb + (int64_t)t * J * 9 : nullptr;
      M3 R = root_matrix(cw[t], sw[t]);  // also for the chains that do not start at the root
      int e = S.chain_offsets[ch];
      const int a = S.chain_joints[e];
      float p0, p1, p2;
      if (a == 0) {
        p0 = px[t], p1 = py[t], p2 = pz[t];
        if (ch == sk.order[0]) {
          fr[0] = p0, fr[1] = p1, fr[2] = p2;
          if (rf) put_matrix(rf, R);
        }
      } else {
        p0 = fr[3 * a], p1 = fr[3 * a + 1], p2 = fr[3 * a + 2];  // stored by a chain of the level before
      }
      for (++e; e < S.chain_offsets[ch + 1]; ++e) {
        const int c = S.chain_joints[e], col = c_rot + 6 * (c - 1);
        R = matmul(R, cont6d_matrix(val(t, col), val(t, col + 1), val(t, col + 2), val(t, col + 3), val(t, col + 4), val(t, col + 5)));
        const float o0 = soff[3 * c], o1 = soff[3 * c + 1], o2 = soff[3 * c + 2];
        p0 = (R.m[0][0] * o0 + R.m[0][1] * o1 + R.m[0][2] * o2) + p0;
        p1 = (R.m[1][0] * o0 + R.m[1][1] * o1 + R.m[1][2] * o2) + p1;
        p2 = (R.m[2][0] * o0 + R.m[2][1] * o1 + R.m[2][2] * o2) + p2;
        fr[3 * c] = p0, fr[3 * c + 1] = p1, fr[3 * c + 2] = p2;
        if (rf) put_matrix(rf + 9 * c, R);
      }
    }
    __syncthreads();
  }
  if (rotb)
    for (int i = n * J * 9 + tid; i < T * J * 9; i += FK_THREADS) rotb[i] = 0.f;

  // temporal gaussian filter of the joints over the valid frames, "nearest" edges; frames past the length are zeroed
  float* ob = out + (int64_t)b * T * W;
  if (radius <= 0) {
    for (int i = n * W + tid; i < T * W; i += FK_THREADS) ob[i] = 0.f;
    return;
  }
  for (int i = tid; i < T * W; i += FK_THREADS) {
    const int t = i / W, c = i - t * W;
    float r = 0.f;
    if (t < n) {
      double acc = (double)rb[(int64_t)t * W + c] * wts[0];
      for (int k = 1; k <= radius; ++k) {
        const int lo = t - k < 0 ? 0 : t - k, hi = t + k > n - 1 ? n - 1 : t + k;
        acc += ((double)rb[(int64_t)lo * W + c] + (double)rb[(int64_t)hi * W + c]) * wts[k];
      }
      r = (float)acc;
    }
    ob[i] = r;
  }
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_motion_fk_max_frames(void) { return mdm::FK_MAX_FRAMES; }

int mdm_motion_fk(const float* motion, const int32_t* length, const float* mean, const float* std,
                  const MdmSkeleton* skeleton, const float* offsets, int32_t offsets_per_sample, int32_t B, int32_t T,
                  int32_t F, int32_t radius, const double* weights, float* scratch, float* joints_out,
                  float* rotations_out, float* offsets_out, void* stream) {
  if (!motion || !mean || !std || !skeleton || !joints_out || B < 0 || T < 1 || radius < 0 || (radius > 0 && !weights))
    return MDM_ERR_ARG;
  if ((radius > 0 || !offsets) && !scratch) return MDM_ERR_ARG;
  mdm::FkArg sk;
  sk.s = *skeleton;
  if (!mdm::skeleton_ok(sk.s, sk.parent) || F != 12 * sk.s.joints - 1) return MDM_ERR_ARG;
  // a chain's level: 0 at the root, else one more than the level of the chain that reached its first joint
  int joint_level[MDM_SKEL_MAX_JOINTS] = {0}, level[MDM_SKEL_MAX_CHAINS];
  sk.nlevels = 0;
  for (int c = 0; c < sk.s.nchains; ++c) {
    const int lo = sk.s.chain_offsets[c], a = sk.s.chain_joints[lo];
    level[c] = a == 0 ? 0 : joint_level[a] + 1;
    for (int e = lo + 1; e < sk.s.chain_offsets[c + 1]; ++e) joint_level[sk.s.chain_joints[e]] = level[c];
    if (level[c] + 1 > sk.nlevels) sk.nlevels = level[c] + 1;
  }
  int k = 0;
  for (int l = 0; l < sk.nlevels; ++l) {
    sk.level_start[l] = k;
    for (int c = 0; c < sk.s.nchains; ++c)
      if (level[c] == l) sk.order[k++] = c;
  }
  sk.level_start[sk.nlevels] = k;
  if (T > mdm::FK_MAX_FRAMES) return MDM_ERR_UNSUPPORTED;
  if (B == 0) return MDM_OK;
  const size_t smem = (size_t)5 * T * sizeof(float);
  const int64_t off_stride = offsets_per_sample ? (int64_t)3 * sk.s.joints : 0;
  hipLaunchKernelGGL(mdm::motion_fk_kernel, dim3(B), dim3(mdm::FK_THREADS), smem, (hipStream_t)stream, motion, length, mean, std,
                     sk, offsets, off_stride, T, radius, weights, scratch, joints_out, rotations_out, offsets_out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
