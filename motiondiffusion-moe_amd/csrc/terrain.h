// Terrain: a height-map ground under the joints, the one more loss term both control kernels
// (motion_control.hip, motion_control_canvas.hip) add to dL/dP of a joint next to the scene's (scene_sdf.h).
//   grid H (Gz, Gx) of heights in metres, row major (H[k][i] at k Gx + i), in global memory: it does not fit in LDS
//   record, TERRAIN_REC floats:  ox, oz, cos yaw, sin yaw, 1 / cell_x, 1 / cell_z, weight a >= 0, margin m
//   (lx, lz) = R_y(-yaw) (p_xz - (ox, oz));  u = clamp(lx / cell_x, 0, Gx - 1), v = clamp(lz / cell_z, 0, Gz - 1)
//   i = min(floor(u), Gx - 2), k = min(floor(v), Gz - 2);  h(p) bilinear in the four samples around (i, k)
//   outside the grid the nearest edge's height holds, with zero slope in the clamped direction
//   clearance e = p_y - h(p) (vertical, not the true distance), grad e = (-dh/dx, 1, -dh/dz) turned back by the yaw
//   penalty of joint j (radius r, weight u, stand weight S >= 0) at p, with d = m + r - e:
//     u a d^2 where d > 0 (the joint is under the ground), S u a d^2 where d < 0 (a planted joint is above it)
// Where grad h jumps (the grid lines) the cell floor() gives is taken.  Heights and gradients in fp32, four dword gathers a
// joint; the caller sums the loss in fp64.  The grid and S are data: no gradient reaches them.
#pragma once
#include <hip/hip_runtime.h>

namespace mdm {
namespace terrain {

constexpr int TERRAIN_REC = 8;
constexpr int MAX_GRID = 512;
enum { OX, OZ, CY, SY, ICX, ICZ, WEIGHT, MARGIN };

// the record of one sample: two 16-byte loads (the record pointer is 16-byte aligned: terrain_ok)
__device__ __forceinline__ void load_record(const float* src, float rec[TERRAIN_REC]) {
  const float4 a = reinterpret_cast<const float4*>(src)[0], b = reinterpret_cast<const float4*>(src)[1];
  rec[0] = a.x, rec[1] = a.y, rec[2] = a.z, rec[3] = a.w, rec[4] = b.x, rec[5] = b.y, rec[6] = b.z, rec[7] = b.w;
}

// Vertical clearance e of p over the terrain and its gradient n.  A NaN coordinate clamps to cell 0: every index stays
// inside the grid whatever p holds.
__device__ __forceinline__ float clearance(const float* grid, int Gx, int Gz, const float rec[TERRAIN_REC], float px, float py,
                                           float pz, float n[3]) {
  const float c = rec[CY], s = rec[SY];
  const float dx = px - rec[OX], dz = pz - rec[OZ];
  const float ru = (c * dx - s * dz) * rec[ICX], rv = (s * dx + c * dz) * rec[ICZ];  // the grid's frame, in cells
  const float u = fminf(fmaxf(ru, 0.f), (float)(Gx - 1)), v = fminf(fmaxf(rv, 0.f), (float)(Gz - 1));
  const int i = min((int)floorf(u), Gx - 2), k = min((int)floorf(v), Gz - 2);
  const float fu = u - (float)i, fv = v - (float)k;
  const float* q = grid + (k * Gx + i);
  const float h00 = q[0], h10 = q[1], h01 = q[Gx], h11 = q[Gx + 1];
  const float lo = h00 + fu * (h10 - h00), hi = h01 + fu * (h11 - h01);
  const float h = lo + fv * (hi - lo);
  // slopes per metre in the grid's frame; zero in a clamped direction
  const float hu = ru < 0.f || ru > (float)(Gx - 1) ? 0.f : ((h10 - h00) + fv * ((h11 - h01) - (h10 - h00))) * rec[ICX];
  const float hv = rv < 0.f || rv > (float)(Gz - 1) ? 0.f : (hi - lo) * rec[ICZ];
  n[0] = -(c * hu + s * hv), n[1] = 1.f, n[2] = -(c * hv - s * hu);  // back to the scene's frame
  return py - h;
}

// The terrain's penalty of one joint at p: adds its dL/dP to g and returns its loss.  u == 0 exempts the joint, a == 0
// switches the terrain off, S == 0 leaves a joint above the ground alone: the term's weight w is then 0 and g keeps its
// value.  Without a branch: every level of divergent control flow costs a pair of the scalar registers the control kernels
// have none to spare of, and the four gathers always stay inside the grid.
__device__ __forceinline__ double penalty(const float* grid, int Gx, int Gz, const float rec[TERRAIN_REC], float r, float u,
                                          float S, float px, float py, float pz, float g[3]) {
  const float ua = u * rec[WEIGHT];
  float n[3];
  const float e = clearance(grid, Gx, Gz, rec, px, py, pz, n);
  const float d = rec[MARGIN] + r - e;
  const float w = d > 0.f ? ua : S * ua;
  const float f = -2.f * w * d;  // dL/de
  g[0] += f * n[0], g[1] += f * n[1], g[2] += f * n[2];
  return (double)w * (double)d * (double)d;
}

// A workgroup-uniform integer as a value of the thread's own (scene::own for a kernel argument): in a vector register.
__device__ __forceinline__ int own(int v) { return __shfl(v, (int)(threadIdx.x & 63), 64); }

// a if on == 1, b if on == 0, by masking bits.  `on` is a value of the thread's own: a select on it would be hoisted out of
// the iteration loop as a lane mask in a pair of scalar registers.
__device__ __forceinline__ float pick(float a, float b, int on) {
  return __int_as_float((__float_as_int(a) & -on) | (__float_as_int(b) & (on - 1)));
}

// The stand weight of joint j of a frame.  on = 1: row[j]; on = 0 (no stand weights given): 0, whatever row[0] holds.
__device__ __forceinline__ float stand_weight(const float* row, int j, int on) { return pick(row[j * on], 0.f, on); }

// the terrain arguments of the mdm_*_terrain_* calls, a grid given: 2 to MAX_GRID samples a side, a record, read 16 bytes at
// a time; grid and stand weights are fp32
inline bool terrain_ok(const float* grid, const float* rec, int Gx, int Gz, const float* stand) {
  if (Gx < 2 || Gx > MAX_GRID || Gz < 2 || Gz > MAX_GRID || !rec) return false;
  return (uintptr_t)grid % 4 == 0 && (uintptr_t)rec % 16 == 0 && (uintptr_t)stand % 4 == 0;
}

}  // namespace terrain
}  // namespace mdm
