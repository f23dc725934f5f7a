// Scene constraints: signed distances of a joint to the primitives of a scene, their gradients, and the
// penalty both control kernels (motion_control.hip, motion_control_canvas.hip) add to dL/dP of a joint.
//   record of primitive k, SCENE_REC floats:  kind, sigma (+1 keep out, -1 keep in), weight a >= 0, margin m, 8 parameters
//     sphere      c[3], r                      d = |p - c| - r                                grad d undefined at the centre
//     capsule     a[3], b[3], r                d = distance to the segment a b - r            ... on the axis
//     box         c[3], h[3], cos yaw, sin yaw d = |max(q, 0)| + min(max(q_x, q_y, q_z), 0),  ... inside, where the two largest q tie
//                                              q = |R_y(-yaw) (p - c)| - h
//     half-space  n[3] (unit), o               d = n . p - o
//   penalty of joint j (radius r, weight u) at p:  u sum_k a_k max(0, m_k + r - sigma_k d_k(p))^2
// Where grad d is undefined (the exact centre or axis) it is taken as 0.  Distances and gradients in fp32; the caller sums
// the loss in fp64.
#pragma once
#include <hip/hip_runtime.h>

namespace mdm {
namespace scene {

constexpr int SCENE_REC = 12;
enum { PAD = 0, SPHERE = 1, CAPSULE = 2, BOX = 3, HALF_SPACE = 4 };

// unit vector of v and its length; the zero vector stays zero
__device__ __forceinline__ float unit(float vx, float vy, float vz, float& nx, float& ny, float& nz) {
  const float len = sqrtf(vx * vx + vy * vy + vz * vz);
  const float inv = len > 0.f ? 1.f / len : 0.f;
  nx = vx * inv, ny = vy * inv, nz = vz * inv;
  return len;
}

// signed distance of p to the primitive of record q (its parameters start at q[4]) and its gradient n
__device__ __forceinline__ float distance(const float* q, int kind, float px, float py, float pz, float& nx, float& ny,
                                          float& nz) {
  if (kind == SPHERE) return unit(px - q[4], py - q[5], pz - q[6], nx, ny, nz) - q[7];
  if (kind == CAPSULE) {
    const float ax = q[4], ay = q[5], az = q[6];
    const float ex = q[7] - ax, ey = q[8] - ay, ez = q[9] - az;
    const float vx = px - ax, vy = py - ay, vz = pz - az;
    const float den = ex * ex + ey * ey + ez * ez;
    float h = den > 0.f ? (vx * ex + vy * ey + vz * ez) / den : 0.f;
    h = fminf(fmaxf(h, 0.f), 1.f);
    return unit(vx - h * ex, vy - h * ey, vz - h * ez, nx, ny, nz) - q[10];
  }
  if (kind == BOX) {
    const float c = q[10], s = q[11];
    const float dx = px - q[4], dz = pz - q[6];
    const float lx = c * dx - s * dz, ly = py - q[5], lz = s * dx + c * dz;  // the box's frame
    const float qx = fabsf(lx) - q[7], qy = fabsf(ly) - q[8], qz = fabsf(lz) - q[9];
    const float sgx = lx > 0.f ? 1.f : (lx < 0.f ? -1.f : 0.f), sgy = ly > 0.f ? 1.f : (ly < 0.f ? -1.f : 0.f),
                sgz = lz > 0.f ? 1.f : (lz < 0.f ? -1.f : 0.f);
    float gx, gy, gz, d;
    const float big = fmaxf(qx, fmaxf(qy, qz));
    if (big > 0.f) {  // outside: the distance to the nearest face, edge or corner
      d = unit(fmaxf(qx, 0.f), fmaxf(qy, 0.f), fmaxf(qz, 0.f), gx, gy, gz);
      gx *= sgx, gy *= sgy, gz *= sgz;
    } else {  // inside: minus the distance to the nearest face
      d = big;
      gx = qx == big ? sgx : 0.f;
      gy = qx != big && qy == big ? sgy : 0.f;
      gz = qx != big && qy != big ? sgz : 0.f;
    }
    nx = c * gx + s * gz, ny = gy, nz = c * gz - s * gx;  // back to the scene's frame
    return d;
  }
  if (kind == HALF_SPACE) {
    nx = q[4], ny = q[5], nz = q[6];
    return nx * px + ny * py + nz * pz - q[7];
  }
  nx = ny = nz = 0.f;
  return 0.f;
}

// The scene's penalty of one joint at p: adds its dL/dP to g and returns its loss.  prims: K records; u == 0 exempts the joint.
__device__ __forceinline__ double penalty(const float* prims, int K, float r, float u, float px, float py, float pz,
                                          float g[3]) {
  double loss = 0.0;
  if (u == 0.f) return loss;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const float* q = prims + k * SCENE_REC;
    const int kind = (int)q[0];
    if (kind < SPHERE || kind > HALF_SPACE) continue;
    float nx, ny, nz;
    const float d = distance(q, kind, px, py, pz, nx, ny, nz);
    const float sg = q[1], ua = u * q[2];
    const float v = q[3] + r - sg * d;
    if (!(v > 0.f) || ua == 0.f) continue;
    loss += (double)ua * (double)v * (double)v;
    const float f = -2.f * ua * v * sg;
    g[0] += f * nx, g[1] += f * ny, g[2] += f * nz;
  }
  return loss;
}

}  // namespace scene
}  // namespace mdm
