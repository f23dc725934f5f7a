// fp32 arithmetic of the root recovery shared by motion_post.hip and motion_fk.hip: single roundings in the reference's
// operation order (no contraction), and the rotation by a Y-axis quaternion.
#pragma once
#include "mdm_common.h"

namespace mdm {

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// v rotated by the quaternion (w, 0, qy, 0): qrot with cross products written out (utils/quaternion.py:70-73)
__device__ __forceinline__ void rot_y(float w, float qy, float vx, float vy, float vz, float& ox, float& oy, float& oz) {
  const float uvx = mul(qy, vz), uvz = -mul(qy, vx);        // uv = cross(qvec, v), qvec = (0, qy, 0)
  const float uuvx = mul(qy, uvz), uuvz = -mul(qy, uvx);    // uuv = cross(qvec, uv)
  ox = add(vx, mul(2.f, add(mul(w, uvx), uuvx)));
  oy = vy;                                                  // + 2 * (w * 0 + 0)
  oz = add(vz, mul(2.f, add(mul(w, uvz), uuvz)));
}

}  // namespace mdm
