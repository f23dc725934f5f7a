// Motion preview on the device: joints (B, T, J, 3) -> image frames, the scene of the reference's
// plot_3d_motion (utils/plot_script.py: floor, root trajectory, five coloured kinematic chains) under a rasteriser that is
// defined here and not by matplotlib.
//   Scene of a sample with n valid frames: MINS / MAXS per axis over valid frames and joints; y -= MINS.y; frame t's x, z are
//   relative to its root; floor = [MINS.x - root.x, MAXS.x - root.x] x [MINS.z - root.z, MAXS.z - root.z] at y = 0; trajectory
//   (t > 1 only) = the polyline through root_xz[0 .. t - 1] - root_xz[t] at y = 0; bones = the links of the skeleton's chains.
//   Camera: look-at pinhole, the basis worked out on the host in double.  A point with view depth z lands at
//   (W/2 + F x / z, H/2 - F y / z); pixel centres at (i + 0.5, j + 0.5); segments and the floor are clipped at z = near.
//   Coverage of a capsule of half-width w: clamp(0.5 + w - d, 0, 1), d the distance to the segment (parameter clamped to
//   [0, 1], squared length floored: a zero-length bone is a disc); of the floor: clamp(0.5 + s, 0, 1), s the smallest signed
//   distance to the polygon's edge lines.  A group's coverage is the maximum over its segments; groups are composited once
//   each, in fp32, floor -> trajectory -> chain 0 .. : c <- c (1 - a cov) + colour a cov.  uint8 = floor(255 c + 0.5).
// Two kernels.  render_scene_kernel: one workgroup per sample reduces MINS / MAXS over the valid frames and copies the root
// path to a dense (T, 2) row, so that the raster kernel reads it with unit stride.  render_raster_kernel: one workgroup per
// (64 x 16 pixel tile, frame, sample): threads project, clip and cull the frame's bones into LDS (compacted per chain with an
// LDS counter: a group's maximum does not depend on the order), one thread builds the floor's edge lines, the trajectory goes
// through LDS in chunks of 256 segments whose maximum is kept in registers, so T is unbounded.  A thread owns 4 horizontally
// adjacent pixels and stores them as three dwords (one in palette mode).  What bounds the kernel is its stores.
// Precision: a segment is held as (anchor, direction, 1 / length^2) with the anchor at the endpoint nearer to the image
// centre, so that an endpoint the near plane has thrown 10^5 pixels off the image costs nothing on it; a floor edge is held
// as the homogeneous line through its two view-space corners, which never forms such coordinates.
#include <cmath>

#include "kernels.h"

namespace mdm {
namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_TILE_W = 64, RD_TILE_H = 16;  // 16 x 16 threads of 4 pixels
constexpr int RD_MAX_BONES = MDM_SKEL_MAX_CHAIN_ENTRIES;
constexpr int RD_MAX_GROUPS = 2 + MDM_SKEL_MAX_CHAINS;
constexpr int RD_SCENE = 8;           // floats of a scene record before the root path: MINS xyz, MAXS xyz, 2 unused
constexpr float RD_CULL_SLACK = 0.01f;  // pixels: a culled segment's coverage is 0 with this much to spare
constexpr float RD_TINY_LEN2 = 1e-12f;  // floor of a projected segment's squared length, pixels^2

struct RenderArg {
  float eye[3], r[3], u[3], f[3];  // camera basis
  float F, near, cx, cy;           // focal length in pixels, near plane, image centre
  float bg[3];
  float colour[RD_MAX_GROUPS][3], alpha[RD_MAX_GROUPS], halfw[RD_MAX_GROUPS];  // groups: floor, trajectory, chains
  int nchains;
  int16_t bone_a[RD_MAX_BONES], bone_b[RD_MAX_BONES];  // joints of link i
  int16_t bone_off[MDM_SKEL_MAX_CHAINS + 1];           // links of chain c: bone_off[c] .. bone_off[c + 1]
};

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 to_view(const RenderArg& a, float x, float y, float z) {
  const float dx = x - a.eye[0], dy = y - a.eye[1], dz = z - a.eye[2];
  return {a.r[0] * dx + a.r[1] * dy + a.r[2] * dz, a.u[0] * dx + a.u[1] * dy + a.u[2] * dz,
          a.f[0] * dx + a.f[1] * dy + a.f[2] * dz};
}

__device__ __forceinline__ V3 at_near(const V3& p, const V3& q, float near) {  // on p q where z = near; p.z < near <= q.z
  const float s = (near - p.z) / (q.z - p.z);
  return {p.x + s * (q.x - p.x), p.y + s * (q.y - p.y), near};
}

// One segment of half-width w (pixels) between two view-space points -> the five floats the shading reads, or false where the
// near plane or the tile's bounds leave nothing of it.  tile: x0, y0, x1, y1 of the tile's outermost pixel centres.
__device__ __forceinline__ bool make_segment(const RenderArg& a, V3 p, V3 q, float w, const float* tile, float* out) {
  if (p.z < a.near && q.z < a.near) return false;
  if (p.z < a.near) p = at_near(p, q, a.near);
  else if (q.z < a.near) q = at_near(q, p, a.near);
  float ax = a.cx + a.F * p.x / p.z, ay = a.cy - a.F * p.y / p.z;
  float bx = a.cx + a.F * q.x / q.z, by = a.cy - a.F * q.y / q.z;
  const float reach = w + 0.5f + RD_CULL_SLACK;  // beyond it the coverage is 0
  if (fmaxf(ax, bx) + reach < tile[0] || fminf(ax, bx) - reach > tile[2] || fmaxf(ay, by) + reach < tile[1] ||
      fminf(ay, by) - reach > tile[3])
    return false;
  const float da = (ax - a.cx) * (ax - a.cx) + (ay - a.cy) * (ay - a.cy);
  const float db = (bx - a.cx) * (bx - a.cx) + (by - a.cy) * (by - a.cy);
  if (db < da) {  // the anchor is the endpoint nearer to the image centre
    float t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
  }
  const float ex = bx - ax, ey = by - ay;
  out[0] = ax, out[1] = ay, out[2] = ex, out[3] = ey, out[4] = 1.f / fmaxf(ex * ex + ey * ey, RD_TINY_LEN2);
  return true;
}

__global__ __launch_bounds__(RD_THREADS) void render_scene_kernel(const float* __restrict__ joints,
                                                                  const int* __restrict__ len, int T, int J,
                                                                  float* __restrict__ scene) {
  __shared__ float red[6][RD_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = len ? len[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const float* src = joints + (int64_t)b * T * J * 3;
  float* rec = scene + (int64_t)b * (RD_SCENE + 2 * T);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = tid; i < n * J; i += RD_THREADS) {  // valid frames only: padding is never read
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float v = src[(int64_t)i * 3 + e];
      lo[e] = fminf(lo[e], v), hi[e] = fmaxf(hi[e], v);
    }
  }
  for (int t = tid; t < T; t += RD_THREADS) {
    const bool ok = t < n;
    rec[RD_SCENE + 2 * t] = ok ? src[(int64_t)t * J * 3] : 0.f;
    rec[RD_SCENE + 2 * t + 1] = ok ? src[(int64_t)t * J * 3 + 2] : 0.f;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) red[e][tid] = lo[e], red[3 + e][tid] = hi[e];
  __syncthreads();
  for (int s = RD_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        red[e][tid] = fminf(red[e][tid], red[e][tid + s]);
        red[3 + e][tid] = fmaxf(red[3 + e][tid], red[3 + e][tid + s]);
      }
    }
    __syncthreads();
  }
  if (tid < RD_SCENE) rec[tid] = tid < 6 ? red[tid][0] : 0.f;
}

__device__ __forceinline__ void blend(float (&c)[4][3], const float (&cov)[4], const float* colour, float alpha) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float k = alpha * cov[i];
#pragma unroll
    for (int e = 0; e < 3; ++e) c[i][e] = c[i][e] * (1.f - k) + colour[e] * k;
  }
}

// max over `count` segments of (base + 5 s) of the capsule coverage at the thread's four pixel centres (px + i, py)
__device__ __forceinline__ void cover(const float* base, int count, float w, float px, float py, float (&cov)[4]) {
  for (int s = 0; s < count; ++s) {
    const float* g = base + 5 * s;  // the same address in every lane: an LDS broadcast
    const float ax = g[0], ay = g[1], ex = g[2], ey = g[3], inv = g[4];
    const float dy = py - ay;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dx = (px + (float)i) - ax;
      const float t = fminf(fmaxf((dx * ex + dy * ey) * inv, 0.f), 1.f);
      const float qx = dx - t * ex, qy = dy - t * ey;
      const float d = sqrtf(qx * qx + qy * qy);
      cov[i] = fmaxf(cov[i], fminf(fmaxf(0.5f + w - d, 0.f), 1.f));
    }
  }
}

__device__ __forceinline__ uint32_t to_u8(float c) {
  return (uint32_t)floorf(fminf(fmaxf(255.f * c + 0.5f, 0.f), 255.f));
}

__global__ __launch_bounds__(RD_THREADS) void render_raster_kernel(
    const float* __restrict__ joints, const int* __restrict__ len, const RenderArg arg, int T, int J, int H, int W, int tiles_x,
    const int* __restrict__ frames, int NF, int palette, const float* __restrict__ scene, uint8_t* __restrict__ out) {
  __shared__ float bone[RD_MAX_BONES * 5];
  __shared__ float traj[RD_THREADS * 5];
  __shared__ float floor_line[6][3], corner[6][3];  // a quadrilateral cut by one plane has 5 corners; 6 whatever the rounding
  __shared__ int count[MDM_SKEL_MAX_CHAINS + 2];  // links kept per chain, trajectory segments kept, floor edges
  const int tid = threadIdx.x, b = blockIdx.z, k = blockIdx.y;
  const int tile_x0 = (blockIdx.x % tiles_x) * RD_TILE_W, tile_y0 = (blockIdx.x / tiles_x) * RD_TILE_H;
  const int x = tile_x0 + 4 * (tid & 15), y = tile_y0 + (tid >> 4);
  const bool inside = x < W && y < H;  // W % 4 == 0: a thread's four pixels are inside together
  const int64_t pixel = (((int64_t)b * NF + k) * H + y) * W + x;
  int n = len ? len[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const int t = frames ? frames[k] : k;
  if (t < 0 || t >= n) {  // block-uniform: a frame past the length is zeros and reads nothing
    if (inside) {
      if (palette) {
        *reinterpret_cast<uint32_t*>(out + pixel) = 0u;
      } else {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + pixel * 3);
        o[0] = 0u, o[1] = 0u, o[2] = 0u;
      }
    }
    return;
  }
  const float* rec = scene + (int64_t)b * (RD_SCENE + 2 * T);
  const float* path = rec + RD_SCENE;
  const float min_x = rec[0], min_y = rec[1], min_z = rec[2], max_x = rec[3], max_z = rec[5];
  const float root_x = path[2 * t], root_z = path[2 * t + 1];
  const float tile[4] = {tile_x0 + 0.5f, tile_y0 + 0.5f, tile_x0 + RD_TILE_W - 0.5f, tile_y0 + RD_TILE_H - 0.5f};
  const int nbones = arg.bone_off[arg.nchains];
  if (tid < MDM_SKEL_MAX_CHAINS + 2) count[tid] = 0;
  __syncthreads();
  if (tid < nbones) {
    int c = 0;
    while (tid >= arg.bone_off[c + 1]) ++c;
    const float* fr = joints + ((int64_t)b * T + t) * J * 3;
    const float* ja = fr + 3 * arg.bone_a[tid];
    const float* jb = fr + 3 * arg.bone_b[tid];
    const V3 p = to_view(arg, ja[0] - root_x, ja[1] - min_y, ja[2] - root_z);
    const V3 q = to_view(arg, jb[0] - root_x, jb[1] - min_y, jb[2] - root_z);
    float seg[5];
    if (make_segment(arg, p, q, arg.halfw[2 + c], tile, seg)) {
      const int slot = arg.bone_off[c] + atomicAdd(&count[c], 1);  // slot < bone_off[c + 1]: at most one per link
#pragma unroll
      for (int e = 0; e < 5; ++e) bone[5 * slot + e] = seg[e];
    }
  } else if (tid == RD_THREADS - 1) {
    // the floor rectangle, clipped at the near plane: a convex polygon of up to 5 corners, each edge as a homogeneous line
    const float fx[4] = {min_x - root_x, max_x - root_x, max_x - root_x, min_x - root_x};
    const float fz[4] = {min_z - root_z, min_z - root_z, max_z - root_z, max_z - root_z};
    V3 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = to_view(arg, fx[i], 0.f, fz[i]);
    int m = 0;  // corners kept, as image-plane homogeneous points (F x, -F y, z): the pixel (cx + X / Z, cy + Y / Z)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const V3 p = v[i], q = v[(i + 1) & 3];
      const bool pin = p.z >= arg.near, qin = q.z >= arg.near;
      if (pin) {
        corner[m][0] = arg.F * p.x, corner[m][1] = -arg.F * p.y, corner[m][2] = p.z;
        ++m;
      }
      if (pin != qin) {
        const V3 s = pin ? at_near(q, p, arg.near) : at_near(p, q, arg.near);
        corner[m][0] = arg.F * s.x, corner[m][1] = -arg.F * s.y, corner[m][2] = s.z;
        ++m;
      }
    }  // m <= 5: one plane cuts a quadrilateral at two edges at most (6 if rounding made the depths alternate)
    int edges = 0;
    for (int i = 0; i < m && m >= 3; ++i) {
      const float* hi = corner[i];
      const float* hj = corner[i + 1 == m ? 0 : i + 1];
      const float l0 = hi[1] * hj[2] - hi[2] * hj[1], l1 = hi[2] * hj[0] - hi[0] * hj[2], l2 = hi[0] * hj[1] - hi[1] * hj[0];
      const float norm2 = l0 * l0 + l1 * l1;
      if (!(norm2 > 0.f)) continue;  // an edge without length
      float side = 0.f, scale = 0.f;  // every other corner lies on the inner side; scale: what the sum's terms are made of
      for (int q = 0; q < m; ++q) {
        const float* h = corner[q];
        side += (l0 * h[0] + l1 * h[1] + l2 * h[2]) / h[2];
        scale = fmaxf(scale, (fabsf(l0 * h[0]) + fabsf(l1 * h[1]) + fabsf(l2 * h[2])) / h[2]);
      }
      if (!(fabsf(side) > 4e-6f * scale)) {  // no area to speak of (the eye in the floor's plane): no floor
        edges = 0;
        break;
      }
      const float inv = (side > 0.f ? 1.f : -1.f) / sqrtf(norm2);
      floor_line[edges][0] = l0 * inv, floor_line[edges][1] = l1 * inv, floor_line[edges][2] = l2 * inv;
      ++edges;
    }
    count[MDM_SKEL_MAX_CHAINS + 1] = edges;
  }
  __syncthreads();
  const float px = x + 0.5f, py = y + 0.5f;
  float c[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 3; ++e) c[i][e] = arg.bg[e];
  const int edges = count[MDM_SKEL_MAX_CHAINS + 1];
  if (edges >= 3) {
    float cov[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = INFINITY;
      for (int e = 0; e < edges; ++e)
        s = fminf(s, floor_line[e][0] * (px + (float)i - arg.cx) + floor_line[e][1] * (py - arg.cy) + floor_line[e][2]);
      cov[i] = fminf(fmaxf(0.5f + s, 0.f), 1.f);
    }
    blend(c, cov, arg.colour[0], arg.alpha[0]);
  }
  if (t > 1) {  // the reference's trajec[:index] rule: t points, t - 1 segments, nothing at t = 1
    float cov[4] = {0.f, 0.f, 0.f, 0.f};
    const float w = arg.halfw[1];
    for (int s0 = 0; s0 < t - 1; s0 += RD_THREADS) {
      const int s = s0 + tid;
      if (s < t - 1) {
        const V3 p = to_view(arg, path[2 * s] - root_x, 0.f, path[2 * s + 1] - root_z);
        const V3 q = to_view(arg, path[2 * s + 2] - root_x, 0.f, path[2 * s + 3] - root_z);
        float seg[5];
        if (make_segment(arg, p, q, w, tile, seg)) {
          const int slot = atomicAdd(&count[MDM_SKEL_MAX_CHAINS], 1);
#pragma unroll
          for (int e = 0; e < 5; ++e) traj[5 * slot + e] = seg[e];
        }
      }
      __syncthreads();
      cover(traj, count[MDM_SKEL_MAX_CHAINS], w, px, py, cov);
      __syncthreads();
      if (tid == 0) count[MDM_SKEL_MAX_CHAINS] = 0;
      __syncthreads();
    }
    blend(c, cov, arg.colour[1], arg.alpha[1]);
  }
  for (int g = 0; g < arg.nchains; ++g) {
    if (count[g] == 0) continue;  // block-uniform
    float cov[4] = {0.f, 0.f, 0.f, 0.f};
    cover(bone + 5 * arg.bone_off[g], count[g], arg.halfw[2 + g], px, py, cov);
    blend(c, cov, arg.colour[2 + g], arg.alpha[2 + g]);
  }
  if (!inside) return;
  uint32_t v[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 3; ++e) v[i][e] = to_u8(c[i][e]);
  if (palette) {  // the 6 x 7 x 6 cube, in integers on the 8-bit colour
    uint32_t word = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t idx = ((v[i][0] * 5u + 127u) / 255u) * 42u + ((v[i][1] * 6u + 127u) / 255u) * 6u + (v[i][2] * 5u + 127u) / 255u;
      word |= idx << (8 * i);
    }
    *reinterpret_cast<uint32_t*>(out + pixel) = word;  // x % 4 == 0 and W % 4 == 0: dword aligned
  } else {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + pixel * 3);  // 12 bytes at a multiple of 12
    o[0] = v[0][0] | v[0][1] << 8 | v[0][2] << 16 | v[1][0] << 24;
    o[1] = v[1][1] | v[1][2] << 8 | v[2][0] << 16 | v[2][1] << 24;
    o[2] = v[2][2] | v[3][0] << 8 | v[3][1] << 16 | v[3][2] << 24;
  }
}

}  // namespace
}  // namespace mdm

extern "C" {

int64_t mdm_motion_render_scratch_floats(int32_t B, int32_t T) {
  if (B < 0 || T < 1) return -1;
  return (int64_t)B * (mdm::RD_SCENE + 2 * (int64_t)T);
}

int mdm_motion_render(const float* joints, const int32_t* length, const MdmSkeleton* skeleton, int32_t B, int32_t T, int32_t J,
                      int32_t H, int32_t W, const float* camera, const float* style, int32_t mode, const int32_t* frames,
                      int32_t n_frames, uint8_t* out, float* scratch, void* stream) {
  if (!joints || !skeleton || !camera || !style || !out || !scratch) return MDM_ERR_ARG;
  if (B < 0 || T < 1 || H < 4 || W < 4 || W % 4 || (mode != 0 && mode != 1)) return MDM_ERR_ARG;
  if (frames && n_frames < 1) return MDM_ERR_ARG;
  if ((uintptr_t)out % 4) return MDM_ERR_ARG;  // written as dwords
  int parent[MDM_SKEL_MAX_JOINTS];
  if (!mdm::skeleton_ok(*skeleton, parent) || J != skeleton->joints) return MDM_ERR_ARG;
  const double elev = camera[0], azim = camera[1], dist = camera[2], fov = camera[3], near = camera[7];
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(camera[i])) return MDM_ERR_ARG;
  if (!(std::fabs(elev) < 89.9) || !(dist > 0) || !(near > 0) || !(near < dist) || !(fov > 0) || !(fov < 180)) return MDM_ERR_ARG;
  const int groups = 2 + skeleton->nchains;
  for (int i = 0; i < 3 + 5 * groups; ++i)
    if (!std::isfinite(style[i])) return MDM_ERR_ARG;
  for (int g = 0; g < groups; ++g)
    if (style[3 + 5 * g + 4] < 0.f) return MDM_ERR_ARG;  // a width
  mdm::RenderArg arg = {};
  const double rad = 3.14159265358979323846 / 180.0;
  const double ce = std::cos(elev * rad), se = std::sin(elev * rad), ca = std::cos(azim * rad), sa = std::sin(azim * rad);
  const double back[3] = {ce * sa, se, ce * ca};  // from the target to the eye
  const double f[3] = {-back[0], -back[1], -back[2]};
  double r[3] = {f[1] * 0 - f[2] * 1, f[2] * 0 - f[0] * 0, f[0] * 1 - f[1] * 0};  // f x (0, 1, 0)
  const double rn = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int e = 0; e < 3; ++e) r[e] /= rn;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};  // r x f
  for (int e = 0; e < 3; ++e) {
    arg.eye[e] = (float)(camera[4 + e] + dist * back[e]);
    arg.r[e] = (float)r[e], arg.u[e] = (float)u[e], arg.f[e] = (float)f[e];
    arg.bg[e] = style[e];
  }
  arg.F = (float)(0.5 * H / std::tan(0.5 * fov * rad));
  arg.near = (float)near, arg.cx = 0.5f * W, arg.cy = 0.5f * H;
  for (int g = 0; g < groups; ++g) {
    const float* s = style + 3 + 5 * g;
    for (int e = 0; e < 3; ++e) arg.colour[g][e] = s[e];
    arg.alpha[g] = s[3];
    arg.halfw[g] = (float)((double)s[4] * H / 1440.0);  // points of a figure 720 points high, half of the full width
  }
  arg.nchains = skeleton->nchains;
  int nb = 0;
  for (int c = 0; c < skeleton->nchains; ++c) {
    arg.bone_off[c] = (int16_t)nb;
    for (int e = skeleton->chain_offsets[c]; e + 1 < skeleton->chain_offsets[c + 1]; ++e, ++nb) {
      arg.bone_a[nb] = (int16_t)skeleton->chain_joints[e];
      arg.bone_b[nb] = (int16_t)skeleton->chain_joints[e + 1];
    }
  }
  for (int c = skeleton->nchains; c <= MDM_SKEL_MAX_CHAINS; ++c) arg.bone_off[c] = (int16_t)nb;
  const int NF = frames ? n_frames : T;
  const int tiles_x = (W + mdm::RD_TILE_W - 1) / mdm::RD_TILE_W, tiles_y = (H + mdm::RD_TILE_H - 1) / mdm::RD_TILE_H;
  if (B > 65535 || NF > 65535 || (int64_t)tiles_x * tiles_y >= ((int64_t)1 << 31)) return MDM_ERR_UNSUPPORTED;  // grid limits
  if (B == 0) return MDM_OK;
  hipLaunchKernelGGL(mdm::render_scene_kernel, dim3(B), dim3(mdm::RD_THREADS), 0, (hipStream_t)stream, joints, length, T, J,
                     scratch);
  MDM_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(mdm::render_raster_kernel, dim3(tiles_x * tiles_y, NF, B), dim3(mdm::RD_THREADS), 0, (hipStream_t)stream,
                     joints, length, arg, T, J, H, W, tiles_x, frames, NF, mode, (const float*)scratch, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
