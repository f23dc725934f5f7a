// Rotation arithmetic shared by the rig kernels (motion_rig.hip, motion_retarget.hip): 3 x 3 matrices and unit
// quaternions held in registers, matrix -> quaternion -> slerp -> matrix -> Euler angles.  Everything is __forceinline__ and
// indexed at compile time, so a matrix never leaves the registers.
#pragma once
#include "kernels.h"

namespace mdm {
namespace rigmath {

struct R3 { float m[3][3]; };
struct Q4 { float w, x, y, z; };

__device__ __forceinline__ R3 load_rot(const float* __restrict__ rot_frame, int joint) {
  R3 a;
  if (joint < 0) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) a.m[r][c] = r == c ? 1.f : 0.f;
    return a;
  }
  const float* p = rot_frame + 9 * joint;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) a.m[r][c] = p[3 * r + c];
  return a;
}

// a^T b
__device__ __forceinline__ R3 tmatmul(const R3& a, const R3& b) {
  R3 o;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o.m[r][c] = a.m[0][r] * b.m[0][c] + a.m[1][r] * b.m[1][c] + a.m[2][r] * b.m[2][c];
  return o;
}

__device__ __forceinline__ Q4 normalised(Q4 q) {
  const float s = 1.f / sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return {q.w * s, q.x * s, q.y * s, q.z * s};
}

// the largest of 1 + trace, 1 + 2 m_ii - trace is >= 1, so no branch divides by a small number
__device__ __forceinline__ Q4 matrix_quat(const R3& a) {
  const float m00 = a.m[0][0], m11 = a.m[1][1], m22 = a.m[2][2], tr = m00 + m11 + m22;
  Q4 q;
  if (tr >= m00 && tr >= m11 && tr >= m22) {
    q = {1.f + tr, a.m[2][1] - a.m[1][2], a.m[0][2] - a.m[2][0], a.m[1][0] - a.m[0][1]};
  } else if (m00 >= m11 && m00 >= m22) {
    q = {a.m[2][1] - a.m[1][2], 1.f + m00 - m11 - m22, a.m[0][1] + a.m[1][0], a.m[0][2] + a.m[2][0]};
  } else if (m11 >= m22) {
    q = {a.m[0][2] - a.m[2][0], a.m[0][1] + a.m[1][0], 1.f - m00 + m11 - m22, a.m[1][2] + a.m[2][1]};
  } else {
    q = {a.m[1][0] - a.m[0][1], a.m[0][2] + a.m[2][0], a.m[1][2] + a.m[2][1], 1.f - m00 - m11 + m22};
  }
  if (q.w < 0.f) q = {-q.w, -q.x, -q.y, -q.z};  // canonical: w >= 0
  return normalised(q);
}

__device__ __forceinline__ R3 quat_matrix(const Q4& q) {
  const float xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z;
  const float wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
  return {{{1.f - 2.f * (yy + zz), 2.f * (xy - wz), 2.f * (xz + wy)},
           {2.f * (xy + wz), 1.f - 2.f * (xx + zz), 2.f * (yz - wx)},
           {2.f * (xz - wy), 2.f * (yz + wx), 1.f - 2.f * (xx + yy)}}};
}

// q0, q1 unit.  The angle between them from the part of q1 across q0 (atan2: exact at small angles, where acos is not)
__device__ __forceinline__ Q4 slerp(const Q4& q0, Q4 q1, float f) {
  float d = q0.w * q1.w + q0.x * q1.x + q0.y * q1.y + q0.z * q1.z;
  if (d < 0.f) q1 = {-q1.w, -q1.x, -q1.y, -q1.z}, d = -d;
  const float pw = q1.w - d * q0.w, px = q1.x - d * q0.x, py = q1.y - d * q0.y, pz = q1.z - d * q0.z;
  const float s = sqrtf(pw * pw + px * px + py * py + pz * pz);
  float w0 = 1.f - f, w1 = f;
  if (s > 1e-6f) {
    const float th = atan2f(s, d);
    w0 = sinf((1.f - f) * th) / s, w1 = sinf(f * th) / s;
  }
  return normalised({w0 * q0.w + w1 * q1.w, w0 * q0.x + w1 * q1.x, w0 * q0.y + w1 * q1.y, w0 * q0.z + w1 * q1.z});
}

// L = R_i(a) R_j(b) R_k(c), sg = +1 for a cyclic (i, j, k), -1 otherwise: L[i][k] = sg sin b, L[i][i] = cos b cos c,
// L[i][j] = -sg cos b sin c.  With c taken, column j of L R_k(c)^T is R_i(a)'s, of full length whatever b: a is taken from it,
// so that at the gimbal (cos b within rounding of 0, c := 0) the matrix is still rebuilt.
// The axes are template arguments: the matrix stays in registers (indexed at run time it would be put in memory).
template <int i, int j, int k>
__device__ __forceinline__ void euler_angles(const R3& L, float& a, float& b, float& c) {
  constexpr float sg = (j == (i + 1) % 3) ? 1.f : -1.f;
  const float cb = sqrtf(L.m[i][i] * L.m[i][i] + L.m[i][j] * L.m[i][j]);
  b = atan2f(sg * L.m[i][k], cb);
  c = cb > 1e-6f ? atan2f(-sg * L.m[i][j], L.m[i][i]) : 0.f;
  float sc, cc;
  sincosf(c, &sc, &cc);
  const float mkj = sg * sc * L.m[k][i] + cc * L.m[k][j], mjj = sg * sc * L.m[j][i] + cc * L.m[j][j];
  a = atan2f(sg * mkj, mjj);
}

}  // namespace rigmath
}  // namespace mdm
