// Joints -> feature rows on the device: the inverse of motion_post.hip.  (T, J, 3) joint positions ->
// (T - 1, 12 J - 1) HumanML3D / KIT rows  root 4 | ric (J-1) 3 | rot6d (J-1) 6 | local velocity J 3 | foot contacts 4.
//   uniform skeleton (optional): leg-length scale, inverse kinematics, forward kinematics on the target offsets
//                                                                          utils/motion_process.py:13-36, utils/skeleton.py:55-147
//   canonical pose: lowest joint on the floor, frame 0's root XZ at the origin, frame 0 facing Z+
//                                                                          utils/motion_process.py:169-218
//   features: foot contacts, facing direction filtered over time (sigma 20, "nearest" edges), root quaternion,
//   inverse kinematics down each chain -> rot6d, root-relative positions, velocities
//                                                                          utils/motion_process.py:39-166, utils/quaternion.py
// Two things are kept as the reference has them, because its training data was made with them:
//   * every kinematic chain starts its accumulated rotation from the ROOT quaternion, also the chains that start at
//     another joint (the two arm chains)                                   utils/skeleton.py:84-85
//   * the inverse kinematics reads the face joints as (l_hip, r_hip, sdr_r, sdr_l) from a list that is ordered
//     (r_hip, l_hip, sdr_r, sdr_l): its "across" vector is (p[face[1]] - p[face[0]]) + (p[face[2]] - p[face[3]]),
//     the canonical pose's is (p[face[0]] - p[face[1]]) + (p[face[2]] - p[face[3]])    utils/skeleton.py:58-60
// One workgroup per sample.  Frames are independent but for the floor minimum (a workgroup reduction), the filter of the
// facing direction (directions and root quaternions live in LDS: 16 bytes a frame) and the t / t + 1 differences; joint
// positions stay in global memory.  The quaternion helpers are fp32 in the reference's operation order with contraction
// off; what the reference does in fp64 before it casts (canonical shift, the uniform skeleton's bone directions and
// accumulation, the filter and the normalisation after it) is done in double.  HBM-bound and tiny.
#pragma clang fp contract(off)
#include "kernels.h"

#include <cmath>

namespace mdm {
namespace {

constexpr int MF_THREADS = 256;
constexpr int MF_MAX_FRAMES = 4000;  // 4 floats of LDS per frame: 62.5 KiB beside the reduction buffer, under 64 KiB

struct SkelArg {
  MdmSkeleton s;
  int leg_parent[2];
};

struct V3 { float x, y, z; };
struct Q4 { float w, x, y, z; };

__device__ __forceinline__ float root2(float v) { return __fsqrt_rn(v); }
__device__ __forceinline__ double root2(double v) { return sqrt(v); }
__device__ __forceinline__ float quot(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double quot(double a, double b) { return a / b; }

__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ Q4 qinv(Q4 q) { return {q.w, -q.x, -q.y, -q.z}; }
// quaternion.py:45-50: terms[i][j] = r_i q_j
__device__ __forceinline__ Q4 qmul(Q4 q, Q4 r) {
  return {r.w * q.w - r.x * q.x - r.y * q.y - r.z * q.z, r.w * q.x + r.x * q.w - r.y * q.z + r.z * q.y,
          r.w * q.y + r.x * q.z + r.y * q.w - r.z * q.x, r.w * q.z - r.x * q.y + r.y * q.x + r.z * q.w};
}
__device__ __forceinline__ V3 qrot(Q4 q, V3 v) {
  const V3 qv = {q.x, q.y, q.z};
  const V3 uv = cross(qv, v), uuv = cross(qv, uv);
  return {v.x + 2.f * (q.w * uv.x + uuv.x), v.y + 2.f * (q.w * uv.y + uuv.y), v.z + 2.f * (q.w * uv.z + uuv.z)};
}
__device__ __forceinline__ Q4 qbetween(V3 a, V3 b) {
  const V3 v = cross(a, b);
  const float w = root2((a.x * a.x + a.y * a.y + a.z * a.z) * (b.x * b.x + b.y * b.y + b.z * b.z)) + (a.x * b.x + a.y * b.y + a.z * b.z);
  const float n = root2(w * w + v.x * v.x + v.y * v.y + v.z * v.z);
  return {quot(w, n), quot(v.x, n), quot(v.y, n), quot(v.z, n)};
}
// first two columns of quaternion_to_matrix (quaternion.py:274-311)
__device__ __forceinline__ void cont6d(Q4 q, float* o) {
  const float r = q.w, i = q.x, j = q.y, k = q.z;
  const float s = quot(2.f, r * r + i * i + j * j + k * k);
  o[0] = 1.f - s * (j * j + k * k), o[1] = s * (i * j + k * r), o[2] = s * (i * k - j * r);
  o[3] = s * (i * j - k * r), o[4] = 1.f - s * (i * i + k * k), o[5] = s * (j * k + i * r);
}

// unit vector from joint a to joint b of one frame, differences and norm in S, handed to the fp32 helpers
template <typename S>
__device__ __forceinline__ V3 bone_dir(const float* fr, int a, int b) {
  const S x = (S)fr[3 * b] - (S)fr[3 * a], y = (S)fr[3 * b + 1] - (S)fr[3 * a + 1], z = (S)fr[3 * b + 2] - (S)fr[3 * a + 2];
  const S n = root2(x * x + y * y + z * z);
  return {(float)quot(x, n), (float)quot(y, n), (float)quot(z, n)};
}

// (a - b) + (c - d) of one frame, normalised, in S; y is the height, shifted by -floor (only the canonical pose has one)
template <typename S>
__device__ __forceinline__ void across_dir(const float* fr, int a, int b, int c, int d, S& ox, S& oz) {
  const S x = ((S)fr[3 * a] - (S)fr[3 * b]) + ((S)fr[3 * c] - (S)fr[3 * d]);
  const S y = ((S)fr[3 * a + 1] - (S)fr[3 * b + 1]) + ((S)fr[3 * c + 1] - (S)fr[3 * d + 1]);
  const S z = ((S)fr[3 * a + 2] - (S)fr[3 * b + 2]) + ((S)fr[3 * c + 2] - (S)fr[3 * d + 2]);
  const S n = root2(x * x + y * y + z * z);
  ox = quot(x, n), oz = quot(z, n);
}

// root quaternion of the facing direction (fx, 0, fz) given in double: normalised there, then qbetween(., Z+) in fp32
__device__ __forceinline__ Q4 facing_quat(double fx, double fz) {
  const double n = sqrt(fx * fx + fz * fz);
  const V3 f = {(float)(fx / n), 0.f, (float)(fz / n)};
  return qbetween(f, V3{0.f, 0.f, 1.f});
}

__global__ __launch_bounds__(MF_THREADS) void motion_features_kernel(
    const float* __restrict__ joints, const int* __restrict__ len, const float* __restrict__ mean, const float* __restrict__ sd,
    const SkelArg sk, const float* __restrict__ tgt, int T, double feet_thre, int canon, int radius,
    const double* __restrict__ wts, float* pos_out, float* __restrict__ out) {
  extern __shared__ float sh[];  // fx[T], fz[T], qw[T], qy[T]
  __shared__ float red[MF_THREADS];
  __shared__ double init[5];     // floor, frame 0's root x and z, the canonical rotation's w and y
  float* fxs = sh;
  float* fzs = fxs + T;
  float* qw = fzs + T;
  float* qy = qw + T;
  const MdmSkeleton& S = sk.s;
  const int J = S.joints, W = 3 * J, F = 12 * J - 1;
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = len ? len[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const float* src = joints + (int64_t)b * T * W;
  float* pos = pos_out ? pos_out + (int64_t)b * T * W : nullptr;

  if (canon) {
    if (tgt) {
      // uniform skeleton: scale by the leg-length ratio of frame 0, inverse kinematics (facing direction unfiltered) and
      // forward kinematics on the target offsets in one walk: both accumulate the same rotation down a chain
      float leg[2], tleg[2];
      for (int k = 0; k < 2; ++k) {
        const int c = S.legs[k], p = sk.leg_parent[k];
        const double x = (double)src[3 * c] - src[3 * p], y = (double)src[3 * c + 1] - src[3 * p + 1], z = (double)src[3 * c + 2] - src[3 * p + 2];
        leg[k] = n > 0 ? (float)sqrt(x * x + y * y + z * z) : 1.f;
        tleg[k] = fmaxf(fmaxf(fabsf(tgt[3 * c]), fabsf(tgt[3 * c + 1])), fabsf(tgt[3 * c + 2]));
      }
      const float scale = quot(tleg[0] + tleg[1], leg[0] + leg[1]);
      for (int t = tid; t < n; t += MF_THREADS) {
        const float* fr = src + (int64_t)t * W;
        float* o = pos + (int64_t)t * W;
        Q4 root = {1.f, 0.f, 0.f, 0.f};
        if (t > 0) {
          double ax, az;
          across_dir<double>(fr, S.face[1], S.face[0], S.face[2], S.face[3], ax, az);
          root = facing_quat(az, -ax);
        }
        for (int c = 0; c < 3; ++c) o[c] = (float)((double)fr[c] * (double)scale);
        for (int ch = 0; ch < S.nchains; ++ch) {
          Q4 R = root;
          int a = S.chain_joints[S.chain_offsets[ch]];
          // a chain starts from its first joint as stored (fp32: the root, or the joint an earlier chain reached); the
          // reference keeps that one in fp64 too.  One rounding of a position, 6e-8 relative; within a chain: double
          double cx = o[3 * a], cy = o[3 * a + 1], cz = o[3 * a + 2];
          for (int e = S.chain_offsets[ch] + 1; e < S.chain_offsets[ch + 1]; ++e) {
            const int c = S.chain_joints[e];
            const V3 u = {S.raw_offsets[3 * c], S.raw_offsets[3 * c + 1], S.raw_offsets[3 * c + 2]};
            const Q4 loc = qmul(qinv(R), qbetween(u, bone_dir<double>(fr, a, c)));
            R = qmul(R, loc);
            const V3 d = qrot(R, V3{tgt[3 * c], tgt[3 * c + 1], tgt[3 * c + 2]});
            cx += (double)d.x, cy += (double)d.y, cz += (double)d.z;
            o[3 * c] = (float)cx, o[3 * c + 1] = (float)cy, o[3 * c + 2] = (float)cz;
            a = c;
          }
        }
      }
      __syncthreads();
    }
    const float* cur = tgt ? pos : src;
    // put on the floor, frame 0's root XZ to the origin, frame 0's facing direction to Z+
    float m = INFINITY;
    for (int i = tid; i < n * J; i += MF_THREADS) m = fminf(m, cur[3 * i + 1]);
    red[tid] = m;
    __syncthreads();
    for (int s = MF_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] = fminf(red[tid], red[tid + s]);
      __syncthreads();
    }
    if (tid == 0 && n > 0) {
      double ax, az;
      across_dir<double>(cur, S.face[0], S.face[1], S.face[2], S.face[3], ax, az);  // heights differ: the floor cancels
      const Q4 q = facing_quat(az, -ax);
      init[0] = red[0], init[1] = cur[0], init[2] = cur[2], init[3] = q.w, init[4] = q.y;
    }
    __syncthreads();
    const Q4 q0 = {(float)init[3], 0.f, (float)init[4], 0.f};
    for (int i = tid; i < T * J; i += MF_THREADS) {
      V3 r = {0.f, 0.f, 0.f};
      if (i < n * J)
        r = qrot(q0, V3{(float)((double)cur[3 * i] - init[1]), (float)((double)cur[3 * i + 1] - init[0]),
                        (float)((double)cur[3 * i + 2] - init[2])});
      pos[3 * i] = r.x, pos[3 * i + 1] = r.y, pos[3 * i + 2] = r.z;
    }
    __syncthreads();
  }
  const float* P = canon ? pos : src;

  // facing direction per frame: cross((0, 1, 0), across) = (across.z, 0, -across.x)
  for (int t = tid; t < n; t += MF_THREADS) {
    float ax, az;
    across_dir<float>(P + (int64_t)t * W, S.face[1], S.face[0], S.face[2], S.face[3], ax, az);
    fxs[t] = az, fzs[t] = -ax;
  }
  __syncthreads();
  // gaussian filter over the valid frames ("nearest" edges, symmetric pairs in double), root quaternion; frame 0: identity
  for (int t = tid; t < n; t += MF_THREADS) {
    double fx = (double)fxs[t], fz = (double)fzs[t];
    if (radius > 0) {
      fx *= wts[0], fz *= wts[0];
      for (int k = radius; k >= 1; --k) {
        const int lo = t - k < 0 ? 0 : t - k, hi = t + k > n - 1 ? n - 1 : t + k;
        fx += ((double)fxs[lo] + (double)fxs[hi]) * wts[k];
        fz += ((double)fzs[lo] + (double)fzs[hi]) * wts[k];
      }
    }
    const Q4 q = facing_quat(fx, fz);
    qw[t] = t == 0 ? 1.f : q.w, qy[t] = t == 0 ? 0.f : q.y;
  }
  __syncthreads();

  const int rows = n > 0 ? n - 1 : 0;
  float* ob = out + (int64_t)b * (T - 1) * F;
  auto put = [&](int t, int c, float v) { ob[(int64_t)t * F + c] = mean ? quot(v - mean[c], sd[c]) : v; };
  const int c_rot = 4 + 3 * (J - 1), c_vel = 4 + 9 * (J - 1), c_feet = F - 4;
  // root, root-relative positions, velocities: one thread per (frame, joint)
  for (int i = tid; i < rows * J; i += MF_THREADS) {
    const int t = i / J, j = i - t * J;
    const float* f0 = P + (int64_t)t * W;
    const float* f1 = f0 + W;
    const Q4 r0 = {qw[t], 0.f, qy[t], 0.f};
    if (j == 0) {
      const Q4 r1 = {qw[t + 1], 0.f, qy[t + 1], 0.f};
      const V3 v = qrot(r1, V3{f1[0] - f0[0], f1[1] - f0[1], f1[2] - f0[2]});
      put(t, 0, asinf(qmul(r1, qinv(r0)).y));
      put(t, 1, v.x), put(t, 2, v.z), put(t, 3, f0[1]);
    } else {
      const V3 l = qrot(r0, V3{f0[3 * j] - f0[0], f0[3 * j + 1], f0[3 * j + 2] - f0[2]});
      const int c = 4 + 3 * (j - 1);
      put(t, c, l.x), put(t, c + 1, l.y), put(t, c + 2, l.z);
    }
    const V3 v = qrot(r0, V3{f1[3 * j] - f0[3 * j], f1[3 * j + 1] - f0[3 * j + 1], f1[3 * j + 2] - f0[3 * j + 2]});
    put(t, c_vel + 3 * j, v.x), put(t, c_vel + 3 * j + 1, v.y), put(t, c_vel + 3 * j + 2, v.z);
  }
  // inverse kinematics -> rot6d: one thread per (frame, chain)
  for (int i = tid; i < rows * S.nchains; i += MF_THREADS) {
    const int t = i / S.nchains, ch = i - t * S.nchains;
    const float* fr = P + (int64_t)t * W;
    Q4 R = {qw[t], 0.f, qy[t], 0.f};
    int a = S.chain_joints[S.chain_offsets[ch]];
    for (int e = S.chain_offsets[ch] + 1; e < S.chain_offsets[ch + 1]; ++e) {
      const int c = S.chain_joints[e];
      const V3 u = {S.raw_offsets[3 * c], S.raw_offsets[3 * c + 1], S.raw_offsets[3 * c + 2]};
      const Q4 loc = qmul(qinv(R), qbetween(u, bone_dir<float>(fr, a, c)));
      float r6[6];
      cont6d(loc, r6);
      for (int k = 0; k < 6; ++k) put(t, c_rot + 6 * (c - 1) + k, r6[k]);
      R = qmul(R, loc);
      a = c;
    }
  }
  // foot contacts: squared displacement to the next frame below the threshold (compared in double, as numpy does)
  for (int i = tid; i < rows * 4; i += MF_THREADS) {
    const int t = i >> 2, k = i & 3, j = S.feet[k];
    const float* f0 = P + (int64_t)t * W + 3 * j;
    const float* f1 = f0 + W;
    const float dx = f1[0] - f0[0], dy = f1[1] - f0[1], dz = f1[2] - f0[2];
    put(t, c_feet + k, (double)(dx * dx + dy * dy + dz * dz) < feet_thre ? 1.f : 0.f);
  }
  for (int i = rows * F + tid; i < (T - 1) * F; i += MF_THREADS) ob[i] = 0.f;
}

}  // namespace

// parent-ordered chains over J joints: every joint but the root is the child of exactly one link, a chain starts at the
// root or at a joint an earlier link reached; parent[] filled
bool skeleton_ok(const MdmSkeleton& s, int* parent) {
  if (s.joints < 2 || s.joints > MDM_SKEL_MAX_JOINTS || s.nchains < 1 || s.nchains > MDM_SKEL_MAX_CHAINS) return false;
  if (s.chain_offsets[0] != 0) return false;
  for (int j = 0; j < s.joints; ++j) parent[j] = -1;
  for (int c = 0; c < s.nchains; ++c) {
    const int lo = s.chain_offsets[c], hi = s.chain_offsets[c + 1];
    if (hi < lo + 2 || hi > MDM_SKEL_MAX_CHAIN_ENTRIES) return false;
    for (int e = lo; e < hi; ++e) {
      const int j = s.chain_joints[e];
      if (j < 0 || j >= s.joints) return false;
      if (e == lo) {
        if (j != 0 && parent[j] < 0) return false;
      } else {
        if (j == 0 || parent[j] >= 0) return false;
        parent[j] = s.chain_joints[e - 1];
        const float* u = s.raw_offsets + 3 * j;
        if (!(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] > 0.f)) return false;
      }
    }
  }
  for (int j = 1; j < s.joints; ++j)
    if (parent[j] < 0) return false;
  for (int k = 0; k < 4; ++k)
    if (s.face[k] < 0 || s.face[k] >= s.joints || s.feet[k] < 0 || s.feet[k] >= s.joints) return false;
  for (int k = 0; k < 2; ++k)
    if (s.legs[k] < 1 || s.legs[k] >= s.joints) return false;
  return true;
}

}  // namespace mdm

extern "C" {

int mdm_motion_features_max_frames(void) { return mdm::MF_MAX_FRAMES; }

int mdm_motion_features(const float* joints, const int32_t* length, const float* mean, const float* std,
                        const MdmSkeleton* skeleton, const float* target_offsets, int32_t B, int32_t T, double feet_thre,
                        int32_t canonicalize, int32_t radius, const double* weights, float* positions_out,
                        float* features_out, void* stream) {
  if (!joints || !skeleton || !features_out || B < 0 || T < 2 || radius < 0 || (radius > 0 && !weights)) return MDM_ERR_ARG;
  if ((mean == nullptr) != (std == nullptr) || !(feet_thre >= 0.0)) return MDM_ERR_ARG;
  if ((canonicalize && !positions_out) || (target_offsets && !canonicalize)) return MDM_ERR_ARG;
  mdm::SkelArg sk;
  sk.s = *skeleton;
  int parent[MDM_SKEL_MAX_JOINTS];
  if (!mdm::skeleton_ok(sk.s, parent)) return MDM_ERR_ARG;
  for (int k = 0; k < 2; ++k) sk.leg_parent[k] = parent[sk.s.legs[k]];
  if (T > mdm::MF_MAX_FRAMES) return MDM_ERR_UNSUPPORTED;
  if (B == 0) return MDM_OK;
  const size_t smem = (size_t)4 * T * sizeof(float);
  hipLaunchKernelGGL(mdm::motion_features_kernel, dim3(B), dim3(mdm::MF_THREADS), smem, (hipStream_t)stream, joints, length,
                     mean, std, sk, target_offsets, T, feet_thre, canonicalize ? 1 : 0, radius, weights,
                     canonicalize ? positions_out : nullptr, features_out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
