// Rig import on the device: the channel values of a BVH file -> joint positions at picked nodes, retimed to
// another frame rate.  The inverse direction of motion_rig.hip, for any hierarchy: the node tables are data.
//   A node's local rotation is L = R_a0(v0) R_a1(v1) R_a2(v2) over its rotation channels in the order the file lists them
//   (0 to 3 of them, any axes, degrees).  It is composed as a quaternion: one factor (cos v/2, sin v/2 e_axis) per channel,
//   multiplied on from the right with a branch per axis, w >= 0, normalised.  Retiming is §19's: output frame k lies at source
//   time k den / num in integers, t0 = (k den) / num, frac = ((k den) % num) / num; the local quaternions at t0 and t0 + 1 ->
//   the second flipped onto the first one's hemisphere -> slerp at frac (lerp where they nearly coincide) -> normalised; the
//   root position is lerped.  Where frac == 0 frame t0 + 1 is not read and nothing is interpolated.
//   Position of a picked node j: p = OFFSET[j]; for every ancestor a up to the root p = OFFSET[a] + L[a] p; the root's position
//   channels are added at the root; out = scale * basis * p.  The walk up needs no per-node matrices: 3 + 4 live floats.
// One thread per (sample, output frame, picked joint), and with quaternions_out one more per (sample, output frame, node), in a
// grid-stride loop; plain loads and stores, no LDS, nothing serial across threads, any T.  The tables travel in the kernel
// argument, packed to 16 and 8 bits (2.9 KB at 128 nodes); they are indexed there, never in registers.
#include "kernels.h"

namespace mdm {
namespace {

constexpr int IMP_THREADS = 256;
constexpr int IMP_MAX_NODES = 128;   // also the deepest chain: parents come first
constexpr int IMP_MAX_COLS = 32767;  // columns travel as int16

struct ImportArg {
  float offset[IMP_MAX_NODES * 3];
  int16_t rot_col[IMP_MAX_NODES * 3];  // -1: the node has no such channel
  int16_t parent[IMP_MAX_NODES];       // -1 at the root
  int16_t pick[IMP_MAX_NODES];
  uint8_t axes[IMP_MAX_NODES];         // axis of channel c in bits 2c, 2c + 1
  int pos_col[3];
  float basis[9];
};

struct Q4 { float w, x, y, z; };

__device__ __forceinline__ Q4 normalised(Q4 q) {
  const float s = 1.f / sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return {q.w * s, q.x * s, q.y * s, q.z * s};
}

// q (cos h, sin h e_axis): the axis is run-time data, so a branch picks the product; no register array is subscripted
__device__ __forceinline__ Q4 times_axis(const Q4& q, int axis, float degrees) {
  float s, c;
  sincospif(degrees * (1.f / 360.f), &s, &c);  // half the angle, in half turns: the reduction is exact at any angle
  if (axis == 0) return {q.w * c - q.x * s, q.x * c + q.w * s, q.y * c + q.z * s, q.z * c - q.y * s};
  if (axis == 1) return {q.w * c - q.y * s, q.x * c - q.z * s, q.y * c + q.w * s, q.z * c + q.x * s};
  return {q.w * c - q.z * s, q.x * c + q.y * s, q.y * c - q.x * s, q.z * c + q.w * s};
}

__device__ __forceinline__ Q4 local_quat(const ImportArg& rig, int node, const float* __restrict__ frame) {
  Q4 q = {1.f, 0.f, 0.f, 0.f};
  const int axes = rig.axes[node];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int col = rig.rot_col[3 * node + c];
    if (col >= 0) q = times_axis(q, (axes >> (2 * c)) & 3, frame[col]);
  }
  if (q.w < 0.f) q = {-q.w, -q.x, -q.y, -q.z};  // canonical: w >= 0
  return normalised(q);
}

// q0, q1 unit: as motion_rig.hip has it (the angle from the part of q1 across q0, atan2), and w >= 0 again afterwards
__device__ __forceinline__ Q4 slerp(const Q4& q0, Q4 q1, float f) {
  float d = q0.w * q1.w + q0.x * q1.x + q0.y * q1.y + q0.z * q1.z;
  if (d < 0.f) q1 = {-q1.w, -q1.x, -q1.y, -q1.z}, d = -d;
  const float pw = q1.w - d * q0.w, px = q1.x - d * q0.x, py = q1.y - d * q0.y, pz = q1.z - d * q0.z;
  const float s = sqrtf(pw * pw + px * px + py * py + pz * pz);
  float w0 = 1.f - f, w1 = f;
  if (s > 1e-6f) {
    const float th = atan2f(s, d) * 0.3183098861837907f;  // in half turns: sinpif needs no table for large arguments
    w0 = sinpif((1.f - f) * th) / s, w1 = sinpif(f * th) / s;
  }
  Q4 q = {w0 * q0.w + w1 * q1.w, w0 * q0.x + w1 * q1.x, w0 * q0.y + w1 * q1.y, w0 * q0.z + w1 * q1.z};
  if (q.w < 0.f) q = {-q.w, -q.x, -q.y, -q.z};
  return normalised(q);
}

// the node's retimed local rotation: frame1 is null where frac == 0 or the next frame lies past the length
__device__ __forceinline__ Q4 node_quat(const ImportArg& rig, int node, const float* __restrict__ frame0,
                                        const float* __restrict__ frame1, float f) {
  const Q4 q = local_quat(rig, node, frame0);
  return frame1 ? slerp(q, local_quat(rig, node, frame1), f) : q;
}

// v turned by the unit quaternion q: v + 2 w (u x v) + 2 u x (u x v)
__device__ __forceinline__ void rotate(const Q4& q, float& x, float& y, float& z) {
  const float cx = q.y * z - q.z * y, cy = q.z * x - q.x * z, cz = q.x * y - q.y * x;
  const float dx = q.y * cz - q.z * cy, dy = q.z * cx - q.x * cz, dz = q.x * cy - q.y * cx;
  x += 2.f * (q.w * cx + dx), y += 2.f * (q.w * cy + dy), z += 2.f * (q.w * cz + dz);
}

__global__ __launch_bounds__(IMP_THREADS) void rig_joints_kernel(
    const float* __restrict__ values, const int* __restrict__ len, const ImportArg rig, int B, int T, int C, int N, int n_pick,
    float scale, int num, int den, int T_out, const int* __restrict__ len_out, float* __restrict__ joints,
    float* __restrict__ quat) {
  const int per = n_pick + (quat ? N : 0);  // work items of one output frame: the picked joints, then the nodes' quaternions
  const uint32_t total = (uint32_t)B * T_out * per;  // < 2^31: the host has checked it, so the index arithmetic is 32-bit
  for (uint32_t i = blockIdx.x * IMP_THREADS + threadIdx.x; i < total; i += gridDim.x * IMP_THREADS) {
    const uint32_t bk = i / per;
    const int item = (int)(i - bk * per);
    const int b = (int)(bk / T_out), k = (int)(bk - b * T_out);
    int n = len ? len[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    const int n_out = len_out ? len_out[b] : T_out;
    const uint32_t kd = (uint32_t)k * den;  // < 2^31: checked on the host
    const int t0 = (int)(kd / num), rem = (int)(kd - t0 * num);
    float* out = item < n_pick ? joints + ((int64_t)bk * n_pick + item) * 3 : nullptr;
    float* qo = item < n_pick ? nullptr : quat + ((int64_t)bk * N + (item - n_pick)) * 4;
    if (k >= n_out || t0 >= n) {  // past the length: zeros, and no source frame is read
      if (out) out[0] = 0.f, out[1] = 0.f, out[2] = 0.f;
      if (qo) qo[0] = 0.f, qo[1] = 0.f, qo[2] = 0.f, qo[3] = 0.f;
      continue;
    }
    const bool two = rem != 0 && t0 + 1 < n;  // frame t0 + 1 is read only where it is needed and valid
    const float f = two ? (float)rem / (float)num : 0.f;
    const float* frame0 = values + ((int64_t)b * T + t0) * C;
    const float* frame1 = two ? frame0 + C : nullptr;
    // a quaternion item is the first step of a walk that starts at its node; a joint item walks from the pick's parent
    int a = qo ? item - n_pick : rig.pick[item];
    float x = 0.f, y = 0.f, z = 0.f;
    if (!qo) {
      x = rig.offset[3 * a], y = rig.offset[3 * a + 1], z = rig.offset[3 * a + 2];
      a = rig.parent[a];
    }
    for (; a >= 0; a = rig.parent[a]) {  // parents come first: the walk ends at the root
      const Q4 q = node_quat(rig, a, frame0, frame1, f);
      if (qo) {
        *reinterpret_cast<float4*>(qo) = make_float4(q.w, q.x, q.y, q.z);  // 16-byte aligned: the host has checked the base
        break;
      }
      rotate(q, x, y, z);
      x += rig.offset[3 * a], y += rig.offset[3 * a + 1], z += rig.offset[3 * a + 2];
    }
    if (qo) continue;
    float root[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {  // the root's position channels are added to its OFFSET
      const int col = rig.pos_col[e];
      float v = 0.f;
      if (col >= 0) {
        v = frame0[col];
        if (two) v = v + f * (frame1[col] - v);
      }
      root[e] = v;
    }
    x += root[0], y += root[1], z += root[2];
    const float* m = rig.basis;
    out[0] = scale * (m[0] * x + m[1] * y + m[2] * z);
    out[1] = scale * (m[3] * x + m[4] * y + m[5] * z);
    out[2] = scale * (m[6] * x + m[7] * y + m[8] * z);
  }
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_rig_joints(const float* values, const int32_t* length, int32_t B, int32_t T, int32_t C, int32_t n_nodes,
                   const int32_t* parent, const float* offsets, const int32_t* rot_col, const int32_t* rot_axis,
                   const int32_t* pos_col, const int32_t* pick, int32_t n_pick, const float* basis, float scale, int32_t num,
                   int32_t den, int32_t T_out, const int32_t* length_out, float* joints_out, float* quaternions_out,
                   void* stream) {
  if ((uintptr_t)quaternions_out % 16) return MDM_ERR_ARG;  // written as float4
  if (!values || !parent || !offsets || !rot_col || !rot_axis || !pos_col || !pick || !basis || !joints_out) return MDM_ERR_ARG;
  if (B < 0 || T < 1 || T_out < 1 || C < 1 || C > mdm::IMP_MAX_COLS || num < 1 || den < 1) return MDM_ERR_ARG;
  if (n_nodes < 1 || n_nodes > mdm::IMP_MAX_NODES || n_pick < 1 || n_pick > mdm::IMP_MAX_NODES) return MDM_ERR_ARG;
  if ((int64_t)(T_out - 1) * den > (int64_t)(T - 1) * num) return MDM_ERR_ARG;  // the last output frame lies past the source
  mdm::ImportArg rig = {};
  int depth[mdm::IMP_MAX_NODES];
  for (int n = 0; n < n_nodes; ++n) {
    const int p = parent[n];
    if (n == 0 ? p != -1 : (p < 0 || p >= n)) return MDM_ERR_ARG;
    depth[n] = p < 0 ? 1 : depth[p] + 1;
    if (depth[n] > mdm::IMP_MAX_NODES) return MDM_ERR_ARG;
    rig.parent[n] = (int16_t)p;
    int axes = 0;
    for (int c = 0; c < 3; ++c) {
      const int col = rot_col[3 * n + c], ax = rot_axis[3 * n + c];
      if (col < -1 || col >= C || ax < 0 || ax > 2) return MDM_ERR_ARG;
      rig.rot_col[3 * n + c] = (int16_t)col;
      axes |= ax << (2 * c);
      rig.offset[3 * n + c] = offsets[3 * n + c];
    }
    rig.axes[n] = (uint8_t)axes;
  }
  for (int n = n_nodes; n < mdm::IMP_MAX_NODES; ++n) rig.parent[n] = -1;
  for (int i = 0; i < 3 * mdm::IMP_MAX_NODES; ++i)
    if (i >= 3 * n_nodes) rig.rot_col[i] = -1;
  for (int e = 0; e < 3; ++e) {
    if (pos_col[e] < -1 || pos_col[e] >= C) return MDM_ERR_ARG;
    rig.pos_col[e] = pos_col[e];
  }
  for (int i = 0; i < n_pick; ++i) {
    if (pick[i] < 0 || pick[i] >= n_nodes) return MDM_ERR_ARG;
    rig.pick[i] = (int16_t)pick[i];
  }
  for (int e = 0; e < 9; ++e) rig.basis[e] = basis[e];
  if (B == 0) return MDM_OK;
  const int64_t total = (int64_t)B * T_out * (n_pick + (quaternions_out ? n_nodes : 0));
  // the kernel counts its work items and the source time k den in 32 bits
  if (total >= ((int64_t)1 << 31) || (int64_t)(T_out - 1) * den >= ((int64_t)1 << 31)) return MDM_ERR_UNSUPPORTED;
  const int64_t blocks = (total + mdm::IMP_THREADS - 1) / mdm::IMP_THREADS;
  const int grid = (int)(blocks < 4096 ? blocks : 4096);
  hipLaunchKernelGGL(mdm::rig_joints_kernel, dim3(grid), dim3(mdm::IMP_THREADS), 0, (hipStream_t)stream, values, length, rig, B,
                     T, C, n_nodes, n_pick, scale, num, den, T_out, length_out, joints_out, quaternions_out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
