// World view of the motion preview: up to four characters and the primitives of a scene (static records and
// per-frame track records, motion_scene's) in one picture per frame, in world coordinates.  Camera, pixel centres, capsule and
// polygon coverage, near-plane clipping, "a group is a maximum, composited once", the rounding and the palette are §21's
// (motion_render.hip); the few device functions both files need are restated here, that file is not touched.
//   Extent: per-axis min / max over the valid frames of every character, the boxes around static spheres, capsules and boxes
//   and around the same kinds among live track records in frames below the world's length (the longest character's).
//   Ground: the extent's XZ rectangle grown by 0.5 m at height ground[b], §21's floor style.  Then one trajectory group per
//   character (root path through frames 0 .. t - 1 at the ground's height, 1 < t < the character's length).  Then the items,
//   far to near by the view depth of a reference point, ties to the lower index: static primitives, tracks, (character, chain).
//     sphere      a disc of radius F r / z_c at the projected centre, dropped where z_c - r < near
//     capsule     the axis clipped at the near plane, stroked with half-width F r / z_m, z_m the clipped axis's mid depth
//     box         the faces the eye sees in the box's own frame (e_x > h_x: +x, ...), each a clipped quad filled once with
//                 shade[axis] * solid colour, then the edges of those faces as one maximum group; keep-in: all 12 edges only
//     half-space  a square on the plane around the projection of the extent's centre, half-side the extent's half-diagonal,
//                 t1 = normalize(n x Y) (X where n is parallel to Y), t2 = n x t1, filled with shade[dominant axis of n]
//     keep-in spheres, capsules and half-spaces, kind 0: nothing
//   A painter's order per item, not a depth test per pixel.
// Three kernels.  world_extent_kernel: one workgroup per world reduces the extent and copies every character's root path to a
// dense row.  world_list_kernel: one workgroup per (drawn frame, world); thread i builds item i in screen space (projects,
// clips, decides the faces, builds edge lines and stroke widths), the keys are ranked by counting in LDS, and every item is
// written to scratch at its rank: the per-frame work is done once, not once per tile.  world_raster_kernel: one workgroup per
// (64 x 16 tile, frame, world); it culls the items' boxes against the tile and compacts them in drawing order with a prefix
// sum over the waves' ballots, stages each kept item in LDS and composites in registers; trajectories go through LDS in
// chunks of 256 segments (any T).  A thread owns 4 pixels and stores three dwords (one in palette mode).
#include <cmath>

#include "kernels.h"
#include "scene_sdf.h"

namespace mdm {
namespace {

constexpr int WR_THREADS = 256;
constexpr int WR_TILE_W = 64, WR_TILE_H = 16;
constexpr int WR_MAX_CHARS = 4;
constexpr int WR_MAX_ITEMS = MDM_SCENE_MAX_PRIMS + MDM_SCENE_MAX_TRACKS + WR_MAX_CHARS * MDM_SKEL_MAX_CHAINS;  // 72
constexpr int WR_MAX_BONES = MDM_SKEL_MAX_CHAIN_ENTRIES;
constexpr int WR_EXT = 8;    // floats of a world's extent record: MINS xyz, MAXS xyz, 2 unused
constexpr int WR_POLY = 24;  // a polygon: edges, r, g, b, alpha, unused, 6 homogeneous edge lines
constexpr int WR_HDR = 12;   // an item: polygons, segments, half-width, r, g, b, alpha of the stroke, unused, box x0 y0 x1 y1
constexpr int WR_SEGS = WR_HDR + 3 * WR_POLY;  // then up to 47 segments of 5 floats
constexpr int WR_ITEM = 320;
constexpr int WR_FRAME = 32;  // a frame's list starts with the ground: its polygon at float 8
constexpr float WR_CULL_SLACK = 0.01f;
constexpr float WR_TINY_LEN2 = 1e-12f;
static_assert(WR_SEGS + 5 * (WR_MAX_BONES - 1) <= WR_ITEM, "an item holds a chain of every link");
static_assert(WR_MAX_ITEMS <= 128, "the raster kernel compacts the items with two waves");

struct WorldArg {
  float eye[3], r[3], u[3], f[3];
  float F, near, cx, cy;
  float bg[3], floor[4], solid[4], edge[3], edge_halfw, shade[3];
  float traj[WR_MAX_CHARS][4], traj_halfw[WR_MAX_CHARS];
  float chain[WR_MAX_CHARS][MDM_SKEL_MAX_CHAINS][4], chain_halfw[WR_MAX_CHARS][MDM_SKEL_MAX_CHAINS];
  int nchains;
  int16_t bone_a[WR_MAX_BONES], bone_b[WR_MAX_BONES];
  int16_t bone_off[MDM_SKEL_MAX_CHAINS + 1];
};

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 to_view(const WorldArg& a, float x, float y, float z) {
  const float dx = x - a.eye[0], dy = y - a.eye[1], dz = z - a.eye[2];
  return {a.r[0] * dx + a.r[1] * dy + a.r[2] * dz, a.u[0] * dx + a.u[1] * dy + a.u[2] * dz,
          a.f[0] * dx + a.f[1] * dy + a.f[2] * dz};
}

__device__ __forceinline__ V3 at_near(const V3& p, const V3& q, float near) {  // on p q where z = near; p.z < near <= q.z
  const float s = (near - p.z) / (q.z - p.z);
  return {p.x + s * (q.x - p.x), p.y + s * (q.y - p.y), near};
}

__device__ __forceinline__ bool clip_segment(V3& p, V3& q, float near) {
  if (p.z < near && q.z < near) return false;
  if (p.z < near) p = at_near(p, q, near);
  else if (q.z < near) q = at_near(q, p, near);
  return true;
}

__device__ __forceinline__ void grow(float* box, float x, float y, float reach) {
  box[0] = fminf(box[0], x - reach), box[1] = fminf(box[1], y - reach);
  box[2] = fmaxf(box[2], x + reach), box[3] = fmaxf(box[3], y + reach);
}

// A clipped view-space segment -> the five floats of §21 (anchor at the end nearer to the image centre, direction,
// 1 / length^2); ends[4]: its pixel ends.
__device__ __forceinline__ void project_segment(const WorldArg& a, const V3& p, const V3& q, float* out, float* ends) {
  float ax = a.cx + a.F * p.x / p.z, ay = a.cy - a.F * p.y / p.z;
  float bx = a.cx + a.F * q.x / q.z, by = a.cy - a.F * q.y / q.z;
  ends[0] = ax, ends[1] = ay, ends[2] = bx, ends[3] = by;
  const float da = (ax - a.cx) * (ax - a.cx) + (ay - a.cy) * (ay - a.cy);
  const float db = (bx - a.cx) * (bx - a.cx) + (by - a.cy) * (by - a.cy);
  if (db < da) {
    float t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
  }
  const float ex = bx - ax, ey = by - ay;
  out[0] = ax, out[1] = ay, out[2] = ex, out[3] = ey, out[4] = 1.f / fmaxf(ex * ex + ey * ey, WR_TINY_LEN2);
}

// Segment s of an item: clipped, projected, written behind the ones before it; the item's box grows by its reach.
__device__ __forceinline__ void emit_segment(const WorldArg& a, V3 p, V3 q, float w, float* item, int& nseg, float* box) {
  if (!clip_segment(p, q, a.near)) return;
  float ends[4];
  project_segment(a, p, q, item + WR_SEGS + 5 * nseg, ends);
  ++nseg;
  const float reach = w + 0.5f + WR_CULL_SLACK;
  grow(box, ends[0], ends[1], reach);
  grow(box, ends[2], ends[3], reach);
}

// A view-space quadrilateral, clipped at the near plane -> its edges as homogeneous lines at poly[6 ..] and their count at
// poly[0] (§21's floor); false where nothing with an area is left.  corner: 18 floats of the thread's own in LDS.
__device__ __forceinline__ bool emit_polygon(const WorldArg& a, const V3 (&v)[4], float* corner, float* poly, float* box) {
  int m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const V3 p = v[i], q = v[(i + 1) & 3];
    const bool pin = p.z >= a.near, qin = q.z >= a.near;
    if (pin) {
      corner[3 * m] = a.F * p.x, corner[3 * m + 1] = -a.F * p.y, corner[3 * m + 2] = p.z;
      ++m;
    }
    if (pin != qin) {
      const V3 s = pin ? at_near(q, p, a.near) : at_near(p, q, a.near);
      corner[3 * m] = a.F * s.x, corner[3 * m + 1] = -a.F * s.y, corner[3 * m + 2] = s.z;
      ++m;
    }
  }  // m <= 6
  int edges = 0;
  for (int i = 0; i < m && m >= 3; ++i) {
    const float* hi = corner + 3 * i;
    const float* hj = corner + 3 * (i + 1 == m ? 0 : i + 1);
    const float l0 = hi[1] * hj[2] - hi[2] * hj[1], l1 = hi[2] * hj[0] - hi[0] * hj[2], l2 = hi[0] * hj[1] - hi[1] * hj[0];
    const float norm2 = l0 * l0 + l1 * l1;
    if (!(norm2 > 0.f)) continue;
    float side = 0.f, scale = 0.f;
    for (int q = 0; q < m; ++q) {
      const float* h = corner + 3 * q;
      side += (l0 * h[0] + l1 * h[1] + l2 * h[2]) / h[2];
      scale = fmaxf(scale, (fabsf(l0 * h[0]) + fabsf(l1 * h[1]) + fabsf(l2 * h[2])) / h[2]);
    }
    if (!(fabsf(side) > 4e-6f * scale)) {  // seen edge-on: no area
      edges = 0;
      break;
    }
    const float inv = (side > 0.f ? 1.f : -1.f) / sqrtf(norm2);
    poly[6 + 3 * edges] = l0 * inv, poly[7 + 3 * edges] = l1 * inv, poly[8 + 3 * edges] = l2 * inv;
    ++edges;
  }
  if (edges < 3) return false;
  poly[0] = (float)edges;
  for (int i = 0; i < m; ++i)
    grow(box, a.cx + corner[3 * i] / corner[3 * i + 2], a.cy + corner[3 * i + 1] / corner[3 * i + 2], 0.5f + WR_CULL_SLACK);
  return true;
}

__device__ __forceinline__ void set_fill(float* poly, const float* colour, float shade, float alpha) {
  poly[1] = colour[0] * shade, poly[2] = colour[1] * shade, poly[3] = colour[2] * shade, poly[4] = alpha, poly[5] = 0.f;
}

__device__ __forceinline__ int clamp_len(const int* len, int i, int T) {
  const int n = len ? len[i] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}

// the box around the primitive of record q: false for a kind without one (padding, a half-space)
__device__ __forceinline__ bool prim_box(const float* q, float* lo, float* hi) {
  const int kind = (int)q[0];
  if (kind == scene::SPHERE) {
#pragma unroll
    for (int e = 0; e < 3; ++e) lo[e] = q[4 + e] - q[7], hi[e] = q[4 + e] + q[7];
    return true;
  }
  if (kind == scene::CAPSULE) {
#pragma unroll
    for (int e = 0; e < 3; ++e) lo[e] = fminf(q[4 + e], q[7 + e]) - q[10], hi[e] = fmaxf(q[4 + e], q[7 + e]) + q[10];
    return true;
  }
  if (kind == scene::BOX) {
    const float c = fabsf(q[10]), s = fabsf(q[11]);
    const float half[3] = {c * q[7] + s * q[9], q[8], s * q[7] + c * q[9]};
#pragma unroll
    for (int e = 0; e < 3; ++e) lo[e] = q[4 + e] - half[e], hi[e] = q[4 + e] + half[e];
    return true;
  }
  return false;
}

// ext: this world's 6 floats at ext + b ext_stride; paths: null, or (B, C, T, 2) root paths
__global__ __launch_bounds__(WR_THREADS) void world_extent_kernel(const float* __restrict__ joints, const int* __restrict__ len,
                                                                  const float* __restrict__ prims, int K,
                                                                  const float* __restrict__ tracks, int Km, int C, int T, int J,
                                                                  float* __restrict__ ext, int ext_stride,
                                                                  float* __restrict__ paths) {
  __shared__ float red[6][WR_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int longest = 0;
  for (int c = 0; c < C; ++c) {
    const int n = clamp_len(len, b * C + c, T);
    longest = n > longest ? n : longest;
    const float* src = joints + ((int64_t)b * C + c) * T * J * 3;
    for (int i = tid; i < n * J; i += WR_THREADS) {  // valid frames only
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float v = src[(int64_t)i * 3 + e];
        lo[e] = fminf(lo[e], v), hi[e] = fmaxf(hi[e], v);
      }
    }
    if (paths) {
      float* row = paths + ((int64_t)b * C + c) * T * 2;
      for (int t = tid; t < T; t += WR_THREADS) {
        const bool ok = t < n;
        row[2 * t] = ok ? src[(int64_t)t * J * 3] : 0.f;
        row[2 * t + 1] = ok ? src[(int64_t)t * J * 3 + 2] : 0.f;
      }
    }
  }
  for (int i = tid; i < K + longest * Km; i += WR_THREADS) {
    const float* q = i < K ? prims + ((int64_t)b * K + i) * scene::SCENE_REC
                           : tracks + ((int64_t)b * T * Km + (i - K)) * scene::SCENE_REC;  // frames below the world's length
    float l[3], h[3];
    if (prim_box(q, l, h)) {
#pragma unroll
      for (int e = 0; e < 3; ++e) lo[e] = fminf(lo[e], l[e]), hi[e] = fmaxf(hi[e], h[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) red[e][tid] = lo[e], red[3 + e][tid] = hi[e];
  __syncthreads();
  for (int s = WR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        red[e][tid] = fminf(red[e][tid], red[e][tid + s]);
        red[3 + e][tid] = fmaxf(red[3 + e][tid], red[3 + e][tid + s]);
      }
    }
    __syncthreads();
  }
  if (tid < 6) ext[(int64_t)b * ext_stride + tid] = red[tid][0];
}

// One workgroup per (output frame k, world b): the frame's ground and items, in drawing order, at list + ((b NF + k) stride).
__global__ __launch_bounds__(WR_THREADS) void world_list_kernel(
    const float* __restrict__ joints, const int* __restrict__ len, const WorldArg arg, const float* __restrict__ prims, int K,
    const float* __restrict__ tracks, int Km, int C, int T, int J, const int* __restrict__ frames, int NF,
    const float* __restrict__ ext, int ext_stride, const float* __restrict__ ground, float* __restrict__ list, int64_t stride) {
  __shared__ float key[WR_MAX_ITEMS];
  __shared__ float work[WR_MAX_ITEMS + 1][18];
  const int tid = threadIdx.x, k = blockIdx.x, b = blockIdx.y;
  const int t = frames ? frames[k] : k;
  int longest = 0;
  for (int c = 0; c < C; ++c) longest = max(longest, clamp_len(len, b * C + c, T));
  if (t < 0 || t >= longest) return;  // the raster kernel writes zeros and reads no list
  const int nslots = K + Km + C * arg.nchains;
  float* out = list + ((int64_t)b * NF + k) * stride;
  const float* e6 = ext + (int64_t)b * ext_stride;
  const float mid[3] = {0.5f * (e6[0] + e6[3]), 0.5f * (e6[1] + e6[4]), 0.5f * (e6[2] + e6[5])};
  const float dgx = e6[3] - e6[0], dgy = e6[4] - e6[1], dgz = e6[5] - e6[2];
  const float half_diag = 0.5f * sqrtf(dgx * dgx + dgy * dgy + dgz * dgz);

  // what the slot is, and its key: the view depth of its reference point (-inf: draws nothing)
  const float* q = nullptr;  // a primitive's record
  const float* fr = nullptr;  // a chain's frame of joints
  int kind = scene::PAD, ch = 0, g = 0;
  float depth = -INFINITY;
  if (tid < K + Km) {
    q = tid < K ? prims + ((int64_t)b * K + tid) * scene::SCENE_REC
                : tracks + (((int64_t)b * T + t) * Km + (tid - K)) * scene::SCENE_REC;
    kind = (int)q[0];
    const bool keep_in = q[1] < 0.f;
    if (kind < scene::SPHERE || kind > scene::HALF_SPACE || (keep_in && kind != scene::BOX)) kind = scene::PAD;
    if (kind == scene::SPHERE || kind == scene::BOX) depth = to_view(arg, q[4], q[5], q[6]).z;
    if (kind == scene::CAPSULE) depth = to_view(arg, 0.5f * (q[4] + q[7]), 0.5f * (q[5] + q[8]), 0.5f * (q[6] + q[9])).z;
    if (kind == scene::HALF_SPACE) {
      if (half_diag < INFINITY) {
        const float d = q[4] * mid[0] + q[5] * mid[1] + q[6] * mid[2] - q[7];
        depth = to_view(arg, mid[0] - d * q[4], mid[1] - d * q[5], mid[2] - d * q[6]).z;
      } else {
        kind = scene::PAD;  // a world without an extent has no square
      }
    }
  } else if (tid < nslots) {
    ch = (tid - K - Km) / arg.nchains, g = (tid - K - Km) % arg.nchains;
    const int first = arg.bone_off[g], last = arg.bone_off[g + 1];
    if (t < clamp_len(len, b * C + ch, T) && last > first) {
      fr = joints + ((((int64_t)b * C + ch) * T + t) * J) * 3;
      const float* j0 = fr + 3 * arg.bone_b[last - 1];
      float sum = to_view(arg, j0[0], j0[1], j0[2]).z;
      for (int i = first; i < last; ++i) {
        const float* ja = fr + 3 * arg.bone_a[i];
        sum += to_view(arg, ja[0], ja[1], ja[2]).z;
      }
      depth = sum / (float)(last - first + 1);
    }
  }
  if (!(depth == depth)) depth = -INFINITY;  // a NaN would tie with nothing, itself included: every slot needs its own rank
  if (tid < nslots) key[tid] = depth;
  __syncthreads();

  if (tid == WR_THREADS - 1) {  // the ground
    float* poly = out + 8;
    float box[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
    const float x0 = e6[0] - 0.5f, x1 = e6[3] + 0.5f, z0 = e6[2] - 0.5f, z1 = e6[5] + 0.5f, y = ground[b];
    const V3 v[4] = {to_view(arg, x0, y, z0), to_view(arg, x1, y, z0), to_view(arg, x1, y, z1), to_view(arg, x0, y, z1)};
    if (!(x1 >= x0 && z1 >= z0) || !emit_polygon(arg, v, work[WR_MAX_ITEMS], poly, box)) poly[0] = 0.f;
    set_fill(poly, arg.floor, 1.f, arg.floor[3]);
    out[0] = (float)nslots;
  }
  if (tid >= nslots) return;

  int rank = 0;  // items drawn before this one: farther, or as far with a lower index
  for (int i = 0; i < nslots; ++i) rank += (key[i] > depth || (key[i] == depth && i < tid)) ? 1 : 0;
  float* item = out + WR_FRAME + (int64_t)rank * WR_ITEM;
  float* corner = work[tid];
  float box[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
  int npoly = 0, nseg = 0;
  float w = 0.f;
  float stroke[4] = {arg.solid[0], arg.solid[1], arg.solid[2], arg.solid[3]};  // r, g, b, alpha of the segments

  if (kind == scene::SPHERE) {
    const V3 c = to_view(arg, q[4], q[5], q[6]);
    if (!(c.z - q[7] < arg.near)) {
      w = arg.F * q[7] / c.z;
      emit_segment(arg, c, c, w, item, nseg, box);
    }
  } else if (kind == scene::CAPSULE) {
    V3 p = to_view(arg, q[4], q[5], q[6]), s = to_view(arg, q[7], q[8], q[9]);
    if (clip_segment(p, s, arg.near)) {
      w = arg.F * q[10] / (0.5f * (p.z + s.z));
      emit_segment(arg, p, s, w, item, nseg, box);
    }
  } else if (kind == scene::BOX) {
    const float c = q[10], s = q[11];
    const float h[3] = {q[7], q[8], q[9]};
    const float dx = arg.eye[0] - q[4], dz = arg.eye[2] - q[6];
    const float el[3] = {c * dx - s * dz, arg.eye[1] - q[5], s * dx + c * dz};  // the eye in the box's frame
    const bool keep_in = q[1] < 0.f;
    int vis[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) vis[a] = keep_in ? 0 : (el[a] > h[a] ? 1 : (el[a] < -h[a] ? -1 : 0));
    const float bx = q[4], by = q[5], bz = q[6];
#define WR_BOX_POINT(l) to_view(arg, bx + c * (l)[0] + s * (l)[2], by + (l)[1], bz - s * (l)[0] + c * (l)[2])
    const int sb[4] = {-1, 1, 1, -1}, sc[4] = {-1, -1, 1, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (vis[a] == 0) continue;
      V3 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float l[3];
        l[a] = vis[a] * h[a], l[(a + 1) % 3] = sb[i] * h[(a + 1) % 3], l[(a + 2) % 3] = sc[i] * h[(a + 2) % 3];
        v[i] = WR_BOX_POINT(l);
      }
      float* poly = item + WR_HDR + WR_POLY * npoly;
      if (emit_polygon(arg, v, corner, poly, box)) {
        set_fill(poly, arg.solid, arg.shade[a == 1 ? 0 : (a == 0 ? 1 : 2)], arg.solid[3]);
        ++npoly;
      }
    }
    w = arg.edge_halfw;
    stroke[0] = arg.edge[0], stroke[1] = arg.edge[1], stroke[2] = arg.edge[2], stroke[3] = 1.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {  // the four edges along axis a
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!(keep_in || vis[(a + 1) % 3] == sb[i] || vis[(a + 2) % 3] == sc[i])) continue;
        float l[3];
        l[(a + 1) % 3] = sb[i] * h[(a + 1) % 3], l[(a + 2) % 3] = sc[i] * h[(a + 2) % 3];
        l[a] = -h[a];
        const V3 p = WR_BOX_POINT(l);
        l[a] = h[a];
        emit_segment(arg, p, WR_BOX_POINT(l), w, item, nseg, box);
      }
    }
#undef WR_BOX_POINT
  } else if (kind == scene::HALF_SPACE) {
    const float nx = q[4], ny = q[5], nz = q[6];
    const float d = nx * mid[0] + ny * mid[1] + nz * mid[2] - q[7];
    const float cx = mid[0] - d * nx, cy = mid[1] - d * ny, cz = mid[2] - d * nz;
    float t1x = 1.f, t1y = 0.f, t1z = 0.f;
    if (nx != 0.f || nz != 0.f) {
      const float inv = 1.f / sqrtf(nz * nz + nx * nx);
      t1x = -nz * inv, t1z = nx * inv;  // n x Y
    }
    const float t2x = ny * t1z - nz * t1y, t2y = nz * t1x - nx * t1z, t2z = nx * t1y - ny * t1x;  // n x t1
    const float s1[4] = {1.f, -1.f, -1.f, 1.f}, s2[4] = {1.f, 1.f, -1.f, -1.f};
    V3 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a1 = s1[i] * half_diag, a2 = s2[i] * half_diag;
      v[i] = to_view(arg, cx + a1 * t1x + a2 * t2x, cy + a1 * t1y + a2 * t2y, cz + a1 * t1z + a2 * t2z);
    }
    float* poly = item + WR_HDR;
    if (emit_polygon(arg, v, corner, poly, box)) {
      const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
      set_fill(poly, arg.solid, arg.shade[(ay >= ax && ay >= az) ? 0 : (ax >= az ? 1 : 2)], arg.solid[3]);
      npoly = 1;
    }
  } else if (fr) {
    w = arg.chain_halfw[ch][g];
#pragma unroll
    for (int e = 0; e < 4; ++e) stroke[e] = arg.chain[ch][g][e];
    for (int i = arg.bone_off[g]; i < arg.bone_off[g + 1]; ++i) {
      const float* ja = fr + 3 * arg.bone_a[i];
      const float* jb = fr + 3 * arg.bone_b[i];
      emit_segment(arg, to_view(arg, ja[0], ja[1], ja[2]), to_view(arg, jb[0], jb[1], jb[2]), w, item, nseg, box);
    }
  }
  item[0] = (float)npoly, item[1] = (float)nseg, item[2] = w;
  item[3] = stroke[0], item[4] = stroke[1], item[5] = stroke[2], item[6] = stroke[3], item[7] = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) item[8 + e] = box[e];  // nothing drawn: an empty box, culled by every tile
}

__device__ __forceinline__ void blend(float (&c)[4][3], const float (&cov)[4], const float* colour, float alpha) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float k = alpha * cov[i];
#pragma unroll
    for (int e = 0; e < 3; ++e) c[i][e] = c[i][e] * (1.f - k) + colour[e] * k;
  }
}

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

// the polygon at poly (LDS), composited over c
__device__ __forceinline__ void fill(const WorldArg& a, const float* poly, float px, float py, float (&c)[4][3]) {
  const int edges = min((int)poly[0], 6);
  if (edges < 3) return;
  float cov[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float s = INFINITY;
    for (int e = 0; e < edges; ++e)
      s = fminf(s, poly[6 + 3 * e] * (px + (float)i - a.cx) + poly[7 + 3 * e] * (py - a.cy) + poly[8 + 3 * e]);
    cov[i] = fminf(fmaxf(0.5f + s, 0.f), 1.f);
  }
  blend(c, cov, poly + 1, poly[4]);
}

__device__ __forceinline__ uint32_t to_u8(float c) {
  return (uint32_t)floorf(fminf(fmaxf(255.f * c + 0.5f, 0.f), 255.f));
}

__global__ __launch_bounds__(WR_THREADS) void world_raster_kernel(
    const int* __restrict__ len, const WorldArg arg, int C, int T, int H, int W, int tiles_x, const int* __restrict__ frames, int NF,
    int palette, const float* __restrict__ paths, const float* __restrict__ ground, const float* __restrict__ list, int64_t stride,
    uint8_t* __restrict__ out) {
  __shared__ float item[WR_ITEM];
  __shared__ float traj[WR_THREADS * 5];
  __shared__ int kept[WR_MAX_ITEMS];
  __shared__ int count[3];  // items kept by wave 0 and by wave 1; trajectory segments kept
  const int tid = threadIdx.x, b = blockIdx.z, k = blockIdx.y;
  const int tile_x0 = (blockIdx.x % tiles_x) * WR_TILE_W, tile_y0 = (blockIdx.x / tiles_x) * WR_TILE_H;
  const int x = tile_x0 + 4 * (tid & 15), y = tile_y0 + (tid >> 4);
  const bool inside = x < W && y < H;
  const int64_t pixel = (((int64_t)b * NF + k) * H + y) * W + x;
  const int t = frames ? frames[k] : k;
  int longest = 0;
  for (int c = 0; c < C; ++c) longest = max(longest, clamp_len(len, b * C + c, T));
  if (t < 0 || t >= longest) {  // block-uniform
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
  const float* src = list + ((int64_t)b * NF + k) * stride;
  const float tile[4] = {tile_x0 + 0.5f, tile_y0 + 0.5f, tile_x0 + WR_TILE_W - 0.5f, tile_y0 + WR_TILE_H - 0.5f};
  const int nslots = min(max((int)src[0], 0), WR_MAX_ITEMS);  // the list kernel's K + Km + C nchains
  if (tid < WR_FRAME) item[tid] = src[tid];
  if (tid < 3) count[tid] = 0;
  bool keep = false;
  if (tid < nslots) {
    const float* box = src + WR_FRAME + (int64_t)tid * WR_ITEM + 8;
    keep = !(box[2] < tile[0] || box[0] > tile[2] || box[3] < tile[1] || box[1] > tile[3]);  // false for an empty box
  }
  const unsigned long long votes = __ballot(keep);  // every wave, outside any branch
  __syncthreads();
  if (tid < 128 && (tid & 63) == 0) count[tid >> 6] = __popcll(votes);
  __syncthreads();
  if (keep) kept[(tid >= 64 ? count[0] : 0) + __popcll(votes & ((1ull << (tid & 63)) - 1ull))] = tid;  // the drawing order stays
  const int nkept = count[0] + count[1];

  const float px = x + 0.5f, py = y + 0.5f;
  float c[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 3; ++e) c[i][e] = arg.bg[e];
  fill(arg, item + 8, px, py, c);  // the ground
  __syncthreads();
  const float gy = ground[b];
  for (int ch = 0; ch < C; ++ch) {
    if (!(t > 1 && t < clamp_len(len, b * C + ch, T))) continue;  // block-uniform
    const float* path = paths + ((int64_t)b * C + ch) * T * 2;
    const float w = arg.traj_halfw[ch];
    const float reach = w + 0.5f + WR_CULL_SLACK;
    float cov[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < t - 1; s0 += WR_THREADS) {
      const int s = s0 + tid;
      if (s < t - 1) {
        V3 p = to_view(arg, path[2 * s], gy, path[2 * s + 1]), q = to_view(arg, path[2 * s + 2], gy, path[2 * s + 3]);
        if (clip_segment(p, q, arg.near)) {
          float seg[5], ends[4];
          project_segment(arg, p, q, seg, ends);
          if (!(fmaxf(ends[0], ends[2]) + reach < tile[0] || fminf(ends[0], ends[2]) - reach > tile[2] ||
                fmaxf(ends[1], ends[3]) + reach < tile[1] || fminf(ends[1], ends[3]) - reach > tile[3])) {
            const int slot = atomicAdd(&count[2], 1);  // a maximum does not depend on the order
#pragma unroll
            for (int e = 0; e < 5; ++e) traj[5 * slot + e] = seg[e];
          }
        }
      }
      __syncthreads();
      cover(traj, count[2], w, px, py, cov);
      __syncthreads();
      if (tid == 0) count[2] = 0;
      __syncthreads();
    }
    blend(c, cov, arg.traj[ch], arg.traj[ch][3]);
  }
  for (int i = 0; i < nkept; ++i) {
    const float* it = src + WR_FRAME + (int64_t)kept[i] * WR_ITEM;
    const int nseg = min(max((int)it[1], 0), WR_MAX_BONES - 1);  // as the list kernel wrote it: inside the item
    for (int j = tid; j < WR_SEGS + 5 * nseg; j += WR_THREADS) item[j] = it[j];
    __syncthreads();
    const int npoly = min(max((int)item[0], 0), 3);
    for (int p = 0; p < npoly; ++p) fill(arg, item + WR_HDR + WR_POLY * p, px, py, c);
    if (nseg > 0) {
      float cov[4] = {0.f, 0.f, 0.f, 0.f};
      cover(item + WR_SEGS, nseg, item[2], px, py, cov);
      blend(c, cov, item + 3, item[6]);
    }
    __syncthreads();
  }
  if (!inside) return;
  uint32_t v[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 3; ++e) v[i][e] = to_u8(c[i][e]);
  if (palette) {
    uint32_t word = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t idx = ((v[i][0] * 5u + 127u) / 255u) * 42u + ((v[i][1] * 6u + 127u) / 255u) * 6u + (v[i][2] * 5u + 127u) / 255u;
      word |= idx << (8 * i);
    }
    *reinterpret_cast<uint32_t*>(out + pixel) = word;
  } else {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + pixel * 3);
    o[0] = v[0][0] | v[0][1] << 8 | v[0][2] << 16 | v[1][0] << 24;
    o[1] = v[1][1] | v[1][2] << 8 | v[2][0] << 16 | v[2][1] << 24;
    o[2] = v[2][2] | v[3][0] << 8 | v[3][1] << 16 | v[3][2] << 24;
  }
}

bool world_shape_ok(const float* joints, const float* prims, int K, const float* tracks, int Km, int B, int C, int T, int J) {
  if (!joints || B < 0 || C < 1 || C > WR_MAX_CHARS || T < 1 || J < 1 || J > MDM_SKEL_MAX_JOINTS) return false;
  if (K < 0 || K > MDM_SCENE_MAX_PRIMS || (K > 0 && !prims)) return false;
  if (Km < 0 || Km > MDM_SCENE_MAX_TRACKS || (Km > 0 && !tracks)) return false;
  return true;
}

int64_t world_list_stride(int C, int K, int Km) { return WR_FRAME + (int64_t)(K + Km + C * MDM_SKEL_MAX_CHAINS) * WR_ITEM; }

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_world_extent(const float* joints, const int32_t* lengths, const float* scene, int32_t K, const float* tracks, int32_t Km,
                     int32_t B, int32_t C, int32_t T, int32_t J, float* extent_out, void* stream) {
  if (!mdm::world_shape_ok(joints, scene, K, tracks, Km, B, C, T, J) || !extent_out) return MDM_ERR_ARG;
  if (B > 65535) return MDM_ERR_UNSUPPORTED;
  if (B == 0) return MDM_OK;
  hipLaunchKernelGGL(mdm::world_extent_kernel, dim3(B), dim3(mdm::WR_THREADS), 0, (hipStream_t)stream, joints, lengths, scene, K,
                     tracks, Km, C, T, J, extent_out, 6, (float*)nullptr);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int64_t mdm_world_render_scratch_floats(int32_t B, int32_t C, int32_t T, int32_t n_frames, int32_t K, int32_t Km) {
  if (B < 0 || C < 1 || C > mdm::WR_MAX_CHARS || T < 1 || n_frames < 1 || K < 0 || K > MDM_SCENE_MAX_PRIMS || Km < 0 ||
      Km > MDM_SCENE_MAX_TRACKS)
    return -1;
  return (int64_t)B * (mdm::WR_EXT + 2 * (int64_t)C * T + (int64_t)n_frames * mdm::world_list_stride(C, K, Km));
}

int mdm_world_render(const float* joints, const int32_t* lengths, const MdmSkeleton* skeleton, const float* scene, int32_t K,
                     const float* tracks, int32_t Km, int32_t B, int32_t C, int32_t T, int32_t J, int32_t H, int32_t W,
                     const float* camera, const float* style, const float* ground, int32_t mode, const int32_t* frames,
                     int32_t n_frames, uint8_t* out, float* scratch, void* stream) {
  if (!skeleton || !camera || !style || !ground || !out || !scratch) return MDM_ERR_ARG;
  if (!mdm::world_shape_ok(joints, scene, K, tracks, Km, B, C, T, J)) return MDM_ERR_ARG;
  if (H < 4 || W < 4 || W % 4 || (mode != 0 && mode != 1)) return MDM_ERR_ARG;
  if (frames && n_frames < 1) return MDM_ERR_ARG;
  if ((uintptr_t)out % 4) return MDM_ERR_ARG;  // written as dwords
  int parent[MDM_SKEL_MAX_JOINTS];
  if (!mdm::skeleton_ok(*skeleton, parent) || J != skeleton->joints) return MDM_ERR_ARG;
  const double elev = camera[0], azim = camera[1], dist = camera[2], fov = camera[3], near = camera[7];
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(camera[i])) return MDM_ERR_ARG;
  if (!(std::fabs(elev) < 89.9) || !(dist > 0) || !(near > 0) || !(near < dist) || !(fov > 0) || !(fov < 180)) return MDM_ERR_ARG;
  const int nchains = skeleton->nchains, per_char = 5 * (1 + nchains);
  for (int i = 0; i < 18 + C * per_char; ++i)
    if (!std::isfinite(style[i])) return MDM_ERR_ARG;
  if (style[14] < 0.f) return MDM_ERR_ARG;  // widths
  for (int i = 0; i < C * (1 + nchains); ++i)
    if (style[18 + 5 * i + 4] < 0.f) return MDM_ERR_ARG;
  mdm::WorldArg arg = {};
  const double rad = 3.14159265358979323846 / 180.0;
  const double ce = std::cos(elev * rad), se = std::sin(elev * rad), ca = std::cos(azim * rad), sa = std::sin(azim * rad);
  const double back[3] = {ce * sa, se, ce * ca};  // from the target to the eye
  const double f[3] = {-back[0], -back[1], -back[2]};
  double r[3] = {f[1] * 0 - f[2] * 1, f[2] * 0 - f[0] * 0, f[0] * 1 - f[1] * 0};  // f x (0, 1, 0)
  const double rn = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int e = 0; e < 3; ++e) r[e] /= rn;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};  // r x f
  const double points = H / 1440.0;  // points of a figure 720 points high, half of the full width
  for (int e = 0; e < 3; ++e) {
    arg.eye[e] = (float)(camera[4 + e] + dist * back[e]);
    arg.r[e] = (float)r[e], arg.u[e] = (float)u[e], arg.f[e] = (float)f[e];
    arg.bg[e] = style[e], arg.edge[e] = style[11 + e], arg.shade[e] = style[15 + e];
  }
  for (int e = 0; e < 4; ++e) arg.floor[e] = style[3 + e], arg.solid[e] = style[7 + e];
  arg.edge_halfw = (float)((double)style[14] * points);
  arg.F = (float)(0.5 * H / std::tan(0.5 * fov * rad));
  arg.near = (float)near, arg.cx = 0.5f * W, arg.cy = 0.5f * H;
  for (int c = 0; c < C; ++c) {
    const float* s = style + 18 + c * per_char;
    for (int e = 0; e < 4; ++e) arg.traj[c][e] = s[e];
    arg.traj_halfw[c] = (float)((double)s[4] * points);
    for (int g = 0; g < nchains; ++g) {
      for (int e = 0; e < 4; ++e) arg.chain[c][g][e] = s[5 + 5 * g + e];
      arg.chain_halfw[c][g] = (float)((double)s[5 + 5 * g + 4] * points);
    }
  }
  arg.nchains = nchains;
  int nb = 0;
  for (int c = 0; c < nchains; ++c) {
    arg.bone_off[c] = (int16_t)nb;
    for (int e = skeleton->chain_offsets[c]; e + 1 < skeleton->chain_offsets[c + 1]; ++e, ++nb) {
      arg.bone_a[nb] = (int16_t)skeleton->chain_joints[e];
      arg.bone_b[nb] = (int16_t)skeleton->chain_joints[e + 1];
    }
  }
  for (int c = nchains; c <= MDM_SKEL_MAX_CHAINS; ++c) arg.bone_off[c] = (int16_t)nb;
  const int NF = frames ? n_frames : T;
  const int tiles_x = (W + mdm::WR_TILE_W - 1) / mdm::WR_TILE_W, tiles_y = (H + mdm::WR_TILE_H - 1) / mdm::WR_TILE_H;
  if (B > 65535 || NF > 65535 || (int64_t)tiles_x * tiles_y >= ((int64_t)1 << 31)) return MDM_ERR_UNSUPPORTED;  // grid limits
  if (B == 0) return MDM_OK;
  float* ext = scratch;  // (B, 8), then the root paths (B, C, T, 2), then the lists (B, NF, stride)
  float* paths = ext + (int64_t)B * mdm::WR_EXT;
  float* list = paths + (int64_t)B * C * T * 2;
  const int64_t stride = mdm::world_list_stride(C, K, Km);
  hipLaunchKernelGGL(mdm::world_extent_kernel, dim3(B), dim3(mdm::WR_THREADS), 0, (hipStream_t)stream, joints, lengths, scene, K,
                     tracks, Km, C, T, J, ext, mdm::WR_EXT, paths);
  MDM_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(mdm::world_list_kernel, dim3(NF, B), dim3(mdm::WR_THREADS), 0, (hipStream_t)stream, joints, lengths, arg, scene,
                     K, tracks, Km, C, T, J, frames, NF, (const float*)ext, mdm::WR_EXT, ground, list, stride);
  MDM_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(mdm::world_raster_kernel, dim3(tiles_x * tiles_y, NF, B), dim3(mdm::WR_THREADS), 0, (hipStream_t)stream,
                     lengths, arg, C, T, H, W, tiles_x, frames, NF, mode, (const float*)paths, ground, (const float*)list, stride, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
