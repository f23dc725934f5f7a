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

// A workgroup-uniform pointer as a value of the thread's own, bit for bit (every lane reads its own lane): the compiler then
// keeps it in vector registers.  The instantiations with tracks hold the pointers their loops use this way: they have vector
// registers to spare and not one scalar register.  ON = false: the pointer itself.
template <bool ON, typename T>
__device__ __forceinline__ T* own(T* p) {
  if (!ON) return p;
  return reinterpret_cast<T*>(__shfl((unsigned long long)p, (int)(threadIdx.x & 63), 64));
}

// The scene's penalty of one joint with tracks: the K records of `prims` and then the Km records of the
// joint's frame at `recs` in global memory (16-byte aligned, three 4-float loads a record), in one walk.  bound: the frame's
// ball (centre, radius) around every live keep-out track inflated by its margin; a joint whose own sphere lies outside it
// leaves the frame's records out of its walk.  A radius of +inf never does, one of -inf (no live track) always.
// One loop with one trip count per joint, not a second loop behind nested conditions: each level costs a pair of the
// scalar registers the control kernels have none to spare of.
__device__ __forceinline__ double penalty_tracks(const float* prims, int K, const float* recs, int Km, const float bound[4],
                                                 float r, float u, float px, float py, float pz, float g[3]) {
  double loss = 0.0;
  const float dx = px - bound[0], dy = py - bound[1], dz = pz - bound[2];
  const int trips = K + (sqrtf(dx * dx + dy * dy + dz * dz) > bound[3] + r ? 0 : Km);
#pragma unroll 1
  for (int k = 0; k < trips; ++k) {
    float q[SCENE_REC];
    if (k < K) {
#pragma unroll
      for (int i = 0; i < SCENE_REC; ++i) q[i] = prims[k * SCENE_REC + i];
    } else {
      const float4* src = reinterpret_cast<const float4*>(recs + (k - K) * SCENE_REC);
      const float4 h = src[0], a = src[1], b = src[2];
      q[0] = h.x, q[1] = h.y, q[2] = h.z, q[3] = h.w, q[4] = a.x, q[5] = a.y, q[6] = a.z, q[7] = a.w;
      q[8] = b.x, q[9] = b.y, q[10] = b.z, q[11] = b.w;
    }
    loss += penalty(q, 1, r, u, px, py, pz, g);  // skips padding and a joint of weight 0
  }
  return loss;
}

// the track arguments of the mdm_*_tracks_* calls: 0 to MAX_TRACKS records a frame; records and bounds are read 16 bytes at a time
constexpr int MAX_TRACKS = 24;
inline bool tracks_ok(const float* tracks, int Km, const float* bounds) {
  if (Km < 0 || Km > MAX_TRACKS || (Km > 0 && !tracks)) return false;
  return (uintptr_t)tracks % 16 == 0 && (uintptr_t)bounds % 16 == 0;
}

}  // namespace scene
}  // namespace mdm
