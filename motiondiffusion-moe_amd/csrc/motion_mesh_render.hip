// Body view of the motion preview: the vertices of a skinned mesh (B, T, V, 3) -> image frames, a triangle
// rasteriser with a depth test per pixel and shading from normals over §21's floor and trajectory.
//   Scene of a sample with n valid frames: MINS / MAXS per axis over the valid frames' finite vertex coordinates; y -= MINS.y;
//   frame t's x, z are relative to root[t]; floor and trajectory as §21, traj[t] = root[t]'s (x, z); camera as §21.
//   Body: vertex i -> view space v_i, depth z_i, screen s_i = (W/2 + F x/z, H/2 - F y/z), w_i = 1/z_i.  A face with a non-finite
//   vertex (or projection), an index outside [0, V) or a z_i < near is dropped.  Edge function of (a, b) at p: with o the
//   lexicographically smaller of s_a, s_b and q the other, C = (q.x - o.x)(p.y - o.y) - (q.y - o.y)(p.x - o.x), no product
//   contracted, E_ab = C if o is s_a else -C: two faces that share an edge compute the same bits C with opposite signs.
//   A = E_01(s_2); A = 0: not drawn; covered iff sign(A) E_k(p) >= 0 for the three edges (two-sided).  E_k the function of the
//   edge opposite vertex k, S = (E_0 + E_1) + E_2 (S = 0: not covered), lambda_k = E_k / S, depth key d = sum lambda_k w_k; the
//   largest d wins, ties to the lower face index.  Shading: g_k = lambda_k w_k / d, P = sum g_k v_k, e = -normalise(P),
//   n = normalise((v_1 - v_0) x (v_2 - v_0)) or normalise(sum g_k n_k), turned towards e, I = ambient + (1 - ambient) max(0, n.l),
//   c <- c (1 - alpha) + alpha colour I.
// Three launches.  mesh_extent_kernel: MR_SLICES workgroups per sample reduce MINS / MAXS over a slice of the valid vertices
// each.  mesh_frame_kernel: one workgroup per (drawn frame, sample) folds the slices, projects every vertex once (8 floats:
// s.x, s.y, w, v.x, v.y, v.z; w = 0 marks a vertex that drops its faces), turns the normals into view space, and writes each
// face's pixel box (two dwords, with the sign of A) and the body's box.  mesh_raster_kernel: one workgroup per (64 x 16 tile,
// frame, sample), a thread owning 4 pixels; floor and trajectory as §21; a tile that the body's box misses stores and leaves;
// else the faces go by in chunks of 256: a thread culls one face's box against the tile, the survivors are compacted in face
// order with wave ballots and a prefix over the four waves (no counter, so the tie rule holds), staged in LDS as three
// ordered edges, and every wave runs the staged faces whose box reaches its 16 x 16 block over its pixels, keeping (d, face,
// lambda) in registers; the winner is shaded once at the end.  F and T are unbounded by LDS.
#include <cmath>

#include "kernels.h"

#pragma clang fp contract(off)  // the edge function's products must not be fused: shared edges rely on equal bits

namespace mdm {
namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_TILE_W = 64, MR_TILE_H = 16;  // four waves, each a block of 16 x 16 pixels: 4 x 16 threads of 4 pixels
constexpr int MR_BLOCK = 16;
constexpr int MR_SLICES = 8;                   // workgroups per sample of the extent reduction
constexpr int MR_PART = 8;                     // floats of a slice's record: MINS xyz, MAXS xyz, 2 unused
constexpr int MR_FRAME = 8;                    // dwords of a frame's record: body box x0, x1, y0, y1 (int), MINS.y, 3 unused
constexpr int MR_VERT = 8;                     // floats of a projected vertex
constexpr int MR_STAGE = 20;                   // floats of a staged face: 3 edges x (o, q - o), 3 signs, 3 w, the face, its columns
constexpr int MR_MAX_SIDE = 8192;              // H, W: a box coordinate (0 .. 8192) sits in a 16-bit field, bit 31 is the sign of A
constexpr uint32_t MR_NO_FACE = 0x0000FFFFu;   // x0 = 65535 > x1 = 0: a face that is not drawn
constexpr float MR_CULL_SLACK = 0.01f;         // as §21
constexpr float MR_TINY_LEN2 = 1e-12f;

struct MeshArg {
  float eye[3], r[3], u[3], f[3];
  float F, near, cx, cy;
  float bg[3];
  float floor_colour[3], floor_alpha;
  float traj_colour[3], traj_alpha, traj_halfw;
  float body_colour[3], body_alpha, ambient;
  float light[3];  // unit, in view space (right, up, away from the eye)
};

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 to_view(const MeshArg& a, float x, float y, float z) {
  const float dx = x - a.eye[0], dy = y - a.eye[1], dz = z - a.eye[2];
  return {a.r[0] * dx + a.r[1] * dy + a.r[2] * dz, a.u[0] * dx + a.u[1] * dy + a.u[2] * dz,
          a.f[0] * dx + a.f[1] * dy + a.f[2] * dz};
}

__device__ __forceinline__ V3 at_near(const V3& p, const V3& q, float near) {  // on p q where z = near; p.z < near <= q.z
  const float s = (near - p.z) / (q.z - p.z);
  return {p.x + s * (q.x - p.x), p.y + s * (q.y - p.y), near};
}

// §21's segment: (anchor, direction, 1 / length^2) of a capsule of half-width w, or false where nothing of it reaches the tile
__device__ __forceinline__ bool make_segment(const MeshArg& a, V3 p, V3 q, float w, const float* tile, float* out) {
  if (p.z < a.near && q.z < a.near) return false;
  if (p.z < a.near) p = at_near(p, q, a.near);
  else if (q.z < a.near) q = at_near(q, p, a.near);
  float ax = a.cx + a.F * p.x / p.z, ay = a.cy - a.F * p.y / p.z;
  float bx = a.cx + a.F * q.x / q.z, by = a.cy - a.F * q.y / q.z;
  const float reach = w + 0.5f + MR_CULL_SLACK;
  if (fmaxf(ax, bx) + reach < tile[0] || fminf(ax, bx) - reach > tile[2] || fmaxf(ay, by) + reach < tile[1] ||
      fminf(ay, by) - reach > tile[3])
    return false;
  const float da = (ax - a.cx) * (ax - a.cx) + (ay - a.cy) * (ay - a.cy);
  const float db = (bx - a.cx) * (bx - a.cx) + (by - a.cy) * (by - a.cy);
  if (db < da) {
    float t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
  }
  const float ex = bx - ax, ey = by - ay;
  out[0] = ax, out[1] = ay, out[2] = ex, out[3] = ey, out[4] = 1.f / fmaxf(ex * ex + ey * ey, MR_TINY_LEN2);
  return true;
}

__device__ __forceinline__ int clamp_len(const int* len, int b, int T) {
  const int n = len ? len[b] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}

__global__ __launch_bounds__(MR_THREADS) void mesh_extent_kernel(const float* __restrict__ vertices,
                                                                 const int* __restrict__ len, int T, int V,
                                                                 float* __restrict__ parts) {
  __shared__ float red[6][MR_THREADS];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = clamp_len(len, b, T);
  const int64_t total = (int64_t)n * V;  // valid frames only: padding is never read
  const int64_t per = (total + MR_SLICES - 1) / MR_SLICES;
  const int64_t lo_i = per * s, hi_i = lo_i + per < total ? lo_i + per : total;
  const float* src = vertices + (int64_t)b * T * V * 3;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = lo_i + tid; i < hi_i; i += MR_THREADS) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float v = src[i * 3 + e];
      if (fabsf(v) < INFINITY) lo[e] = fminf(lo[e], v), hi[e] = fmaxf(hi[e], v);  // a coordinate that is not finite is no extent
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) red[e][tid] = lo[e], red[3 + e][tid] = hi[e];
  __syncthreads();
  for (int h = MR_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        red[e][tid] = fminf(red[e][tid], red[e][tid + h]);
        red[3 + e][tid] = fmaxf(red[3 + e][tid], red[3 + e][tid + h]);
      }
    }
    __syncthreads();
  }
  if (tid < MR_PART) parts[((int64_t)b * MR_SLICES + s) * MR_PART + tid] = tid < 6 ? red[tid][0] : 0.f;
}

// the extent of sample b, element e of (MINS xyz, MAXS xyz), from the slices
__device__ __forceinline__ float extent_of(const float* parts, int b, int e) {
  const float* p = parts + (int64_t)b * MR_SLICES * MR_PART + e;
  float v = p[0];
#pragma unroll
  for (int s = 1; s < MR_SLICES; ++s) v = e < 3 ? fminf(v, p[s * MR_PART]) : fmaxf(v, p[s * MR_PART]);
  return v;
}

__device__ __forceinline__ bool lex_less(float ax, float ay, float bx, float by) { return ax < bx || (ax == bx && ay < by); }

// E_ab at p (see the head of the file)
__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
  const bool swap = lex_less(bx, by, ax, ay);
  const float ox = swap ? bx : ax, oy = swap ? by : ay, qx = swap ? ax : bx, qy = swap ? ay : by;
  const float c = (qx - ox) * (py - oy) - (qy - oy) * (px - ox);
  return swap ? -c : c;
}

__global__ __launch_bounds__(MR_THREADS) void mesh_frame_kernel(
    const float* __restrict__ vertices, const float* __restrict__ normals, const int* __restrict__ faces,
    const float* __restrict__ root, const int* __restrict__ len, const MeshArg arg, int T, int V, int F, int H, int W,
    const int* __restrict__ frames, int NF, const float* __restrict__ parts, float* __restrict__ frame_rec,
    float* __restrict__ pv, float* __restrict__ pn, uint32_t* __restrict__ face_rec) {
  __shared__ float red[4][MR_THREADS];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = clamp_len(len, b, T);
  const int t = frames ? frames[k] : k;
  if (t < 0 || t >= n) return;  // the raster kernel reads nothing of such a frame
  const int64_t fk = (int64_t)b * NF + k;
  const float min_y = extent_of(parts, b, 1);
  const float* rt = root + ((int64_t)b * T + t) * 3;
  const float root_x = rt[0], root_z = rt[2];
  const float* src = vertices + ((int64_t)b * T + t) * V * 3;
  const float* nsrc = normals ? normals + ((int64_t)b * T + t) * V * 3 : nullptr;
  float* dst = pv + fk * V * MR_VERT;
  float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  for (int i = tid; i < V; i += MR_THREADS) {
    const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    const V3 v = to_view(arg, x - root_x, y - min_y, z - root_z);
    float sx = 0.f, sy = 0.f, w = 0.f;
    if (v.z >= arg.near) {  // false for a NaN depth
      sx = arg.cx + arg.F * v.x / v.z, sy = arg.cy - arg.F * v.y / v.z;
      w = 1.f / v.z;
      if (!(fabsf(sx) < INFINITY && fabsf(sy) < INFINITY && fabsf(v.x) < INFINITY && fabsf(v.y) < INFINITY && w > 0.f))
        sx = 0.f, sy = 0.f, w = 0.f;
    }
    if (w > 0.f) lo_x = fminf(lo_x, sx), hi_x = fmaxf(hi_x, sx), lo_y = fminf(lo_y, sy), hi_y = fmaxf(hi_y, sy);
    float4* o = reinterpret_cast<float4*>(dst + (int64_t)i * MR_VERT);
    o[0] = make_float4(sx, sy, w, 0.f);
    o[1] = make_float4(v.x, v.y, v.z, 0.f);
    if (nsrc) {
      const float nx = nsrc[3 * i], ny = nsrc[3 * i + 1], nz = nsrc[3 * i + 2];
      reinterpret_cast<float4*>(pn + fk * V * 4)[i] =
          make_float4(arg.r[0] * nx + arg.r[1] * ny + arg.r[2] * nz, arg.u[0] * nx + arg.u[1] * ny + arg.u[2] * nz,
                      arg.f[0] * nx + arg.f[1] * ny + arg.f[2] * nz, 0.f);
    }
  }
  red[0][tid] = lo_x, red[1][tid] = lo_y, red[2][tid] = hi_x, red[3][tid] = hi_y;
  __syncthreads();  // also makes this workgroup's projected vertices visible to all of its threads
  for (int h = MR_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] = fminf(red[0][tid], red[0][tid + h]), red[1][tid] = fminf(red[1][tid], red[1][tid + h]);
      red[2][tid] = fmaxf(red[2][tid], red[2][tid + h]), red[3][tid] = fmaxf(red[3][tid], red[3][tid + h]);
    }
    __syncthreads();
  }
  // a pixel box: the pixels whose centres lie inside [lo, hi], grown by one pixel so that no rounding of an edge function can
  // claim a pixel outside it; clamped to the image as floats first, so that no huge coordinate is converted
  auto first = [](float lo, int size) { return (int)fminf(fmaxf(floorf(lo - 0.5f) - 1.f, 0.f), (float)size); };
  auto last = [](float hi, int size) { return (int)fminf(fmaxf(floorf(hi - 0.5f) + 1.f, -1.f), (float)(size - 1)); };
  if (tid == 0) {
    int* rec = reinterpret_cast<int*>(frame_rec + fk * MR_FRAME);
    const bool any = red[0][0] <= red[2][0];
    rec[0] = any ? first(red[0][0], W) : 1, rec[1] = any ? last(red[2][0], W) : 0;
    rec[2] = any ? first(red[1][0], H) : 1, rec[3] = any ? last(red[3][0], H) : 0;
    frame_rec[fk * MR_FRAME + 4] = min_y;
  }
  uint32_t* frec = face_rec + fk * F * 2;
  for (int f = tid; f < F; f += MR_THREADS) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    uint32_t r0 = MR_NO_FACE, r1 = 0u;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
      const float4 a = *reinterpret_cast<const float4*>(dst + (int64_t)i0 * MR_VERT);
      const float4 c = *reinterpret_cast<const float4*>(dst + (int64_t)i1 * MR_VERT);
      const float4 d = *reinterpret_cast<const float4*>(dst + (int64_t)i2 * MR_VERT);
      if (a.z > 0.f && c.z > 0.f && d.z > 0.f) {
        const float A = edge_fn(a.x, a.y, c.x, c.y, d.x, d.y);
        if (A > 0.f || A < 0.f) {
          const int x0 = first(fminf(a.x, fminf(c.x, d.x)), W), x1 = last(fmaxf(a.x, fmaxf(c.x, d.x)), W);
          const int y0 = first(fminf(a.y, fminf(c.y, d.y)), H), y1 = last(fmaxf(a.y, fmaxf(c.y, d.y)), H);
          if (x0 <= x1 && y0 <= y1) {
            r0 = (uint32_t)x0 | (uint32_t)x1 << 16;
            r1 = (uint32_t)y0 | (uint32_t)y1 << 16 | (A < 0.f ? 0x80000000u : 0u);
          }
        }
      }
    }
    frec[2 * f] = r0, frec[2 * f + 1] = r1;
  }
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
    const float* g = base + 5 * s;
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

__device__ __forceinline__ V3 normalise(V3 a) {
  const float l = sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
  if (!(l > 0.f)) return {0.f, 0.f, 0.f};
  return {a.x / l, a.y / l, a.z / l};
}

// one ordered edge of a staged face: o, q - o and the sign that makes the function positive inside the face
__device__ __forceinline__ void stage_edge(float* e, float* sign, float ax, float ay, float bx, float by, float face_sign) {
  const bool swap = lex_less(bx, by, ax, ay);
  const float ox = swap ? bx : ax, oy = swap ? by : ay, qx = swap ? ax : bx, qy = swap ? ay : by;
  e[0] = ox, e[1] = oy, e[2] = qx - ox, e[3] = qy - oy;
  *sign = swap ? -face_sign : face_sign;
}

__global__ __launch_bounds__(MR_THREADS) void mesh_raster_kernel(
    const int* __restrict__ faces, const float* __restrict__ root, const int* __restrict__ len, const MeshArg arg, int T, int V,
    int F, int H, int W, int tiles_x, const int* __restrict__ frames, int NF, int palette, int smooth,
    const float* __restrict__ parts, const float* __restrict__ frame_rec, const float* __restrict__ pv,
    const float* __restrict__ pn, const uint32_t* __restrict__ face_rec, uint8_t* __restrict__ out) {
  __shared__ float stage[MR_THREADS * MR_STAGE];  // the trajectory's segments (5 floats), then the faces (20 floats)
  __shared__ float floor_line[6][3], corner[6][3];
  __shared__ int count[2];       // trajectory segments kept, floor edges
  __shared__ int wave_count[4];  // faces kept by each wave of a chunk
  const int tid = threadIdx.x, b = blockIdx.z, k = blockIdx.y;
  const int tile_x0 = (blockIdx.x % tiles_x) * MR_TILE_W, tile_y0 = (blockIdx.x / tiles_x) * MR_TILE_H;
  // a wave owns a 16 x 16 block of the tile (4 threads of 4 pixels across, 16 rows), so that it can pass over a face whose
  // box misses the block with one scalar branch: a body's faces are a few pixels each
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int x = tile_x0 + MR_BLOCK * wave + 4 * (lane & 3), y = tile_y0 + (lane >> 2);
  const bool inside = x < W && y < H;
  const int64_t pixel = (((int64_t)b * NF + k) * H + y) * W + x;
  const int n = clamp_len(len, b, T);
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
  const int64_t fk = (int64_t)b * NF + k;
  const float* path = root + (int64_t)b * T * 3;
  const float min_x = extent_of(parts, b, 0), min_z = extent_of(parts, b, 2);
  const float max_x = extent_of(parts, b, 3), max_z = extent_of(parts, b, 5);
  const float root_x = path[3 * t], root_z = path[3 * t + 2];
  const float tile[4] = {tile_x0 + 0.5f, tile_y0 + 0.5f, tile_x0 + MR_TILE_W - 0.5f, tile_y0 + MR_TILE_H - 0.5f};
  if (tid < 2) count[tid] = 0;
  __syncthreads();
  if (tid == MR_THREADS - 1) {
    // §21's floor: the rectangle clipped at the near plane, each edge of the polygon as a homogeneous line
    const float fx[4] = {min_x - root_x, max_x - root_x, max_x - root_x, min_x - root_x};
    const float fz[4] = {min_z - root_z, min_z - root_z, max_z - root_z, max_z - root_z};
    V3 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = to_view(arg, fx[i], 0.f, fz[i]);
    int m = 0;
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
    }
    int edges = 0;
    for (int i = 0; i < m && m >= 3; ++i) {
      const float* hi = corner[i];
      const float* hj = corner[i + 1 == m ? 0 : i + 1];
      const float l0 = hi[1] * hj[2] - hi[2] * hj[1], l1 = hi[2] * hj[0] - hi[0] * hj[2], l2 = hi[0] * hj[1] - hi[1] * hj[0];
      const float norm2 = l0 * l0 + l1 * l1;
      if (!(norm2 > 0.f)) continue;
      float side = 0.f, scale = 0.f;
      for (int q = 0; q < m; ++q) {
        const float* h = corner[q];
        side += (l0 * h[0] + l1 * h[1] + l2 * h[2]) / h[2];
        scale = fmaxf(scale, (fabsf(l0 * h[0]) + fabsf(l1 * h[1]) + fabsf(l2 * h[2])) / h[2]);
      }
      if (!(fabsf(side) > 4e-6f * scale)) {
        edges = 0;
        break;
      }
      const float inv = (side > 0.f ? 1.f : -1.f) / sqrtf(norm2);
      floor_line[edges][0] = l0 * inv, floor_line[edges][1] = l1 * inv, floor_line[edges][2] = l2 * inv;
      ++edges;
    }
    count[1] = edges;
  }
  __syncthreads();
  const float px = x + 0.5f, py = y + 0.5f;
  float c[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 3; ++e) c[i][e] = arg.bg[e];
  const int edges = count[1];
  if (edges >= 3) {
    float cov[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = INFINITY;
      for (int e = 0; e < edges; ++e)
        s = fminf(s, floor_line[e][0] * (px + (float)i - arg.cx) + floor_line[e][1] * (py - arg.cy) + floor_line[e][2]);
      cov[i] = fminf(fmaxf(0.5f + s, 0.f), 1.f);
    }
    blend(c, cov, arg.floor_colour, arg.floor_alpha);
  }
  if (t > 1) {
    float cov[4] = {0.f, 0.f, 0.f, 0.f};
    const float w = arg.traj_halfw;
    for (int s0 = 0; s0 < t - 1; s0 += MR_THREADS) {
      const int s = s0 + tid;
      if (s < t - 1) {
        const V3 p = to_view(arg, path[3 * s] - root_x, 0.f, path[3 * s + 2] - root_z);
        const V3 q = to_view(arg, path[3 * s + 3] - root_x, 0.f, path[3 * s + 5] - root_z);
        float seg[5];
        if (make_segment(arg, p, q, w, tile, seg)) {
          const int slot = atomicAdd(&count[0], 1);  // in LDS; a maximum does not depend on the order
#pragma unroll
          for (int e = 0; e < 5; ++e) stage[5 * slot + e] = seg[e];
        }
      }
      __syncthreads();
      cover(stage, count[0], w, px, py, cov);
      __syncthreads();
      if (tid == 0) count[0] = 0;
      __syncthreads();
    }
    blend(c, cov, arg.traj_colour, arg.traj_alpha);
  }
  // ---- the body ----
  const int* box = reinterpret_cast<const int*>(frame_rec + fk * MR_FRAME);
  const int tx1 = tile_x0 + MR_TILE_W - 1, ty1 = tile_y0 + MR_TILE_H - 1;
  const bool body = arg.body_alpha > 0.f && box[0] <= tx1 && box[1] >= tile_x0 && box[2] <= ty1 && box[3] >= tile_y0;  // uniform
  float best_d[4] = {0.f, 0.f, 0.f, 0.f}, best_l0[4] = {}, best_l1[4] = {}, best_l2[4] = {};
  int best_f[4] = {-1, -1, -1, -1};
  if (body) {
    const uint32_t* frec = face_rec + fk * F * 2;
    const float* verts = pv + fk * V * MR_VERT;
    const int block_x0 = MR_BLOCK * wave, block_x1 = MR_BLOCK * wave + MR_BLOCK - 1;  // the wave's columns of the tile
    for (int f0 = 0; f0 < F; f0 += MR_THREADS) {
      const int f = f0 + tid;
      bool keep = false;
      uint32_t r1 = 0u, columns = 0u;
      if (f < F) {
        const uint32_t r0 = frec[2 * f];
        r1 = frec[2 * f + 1];
        const int x0 = r0 & 0xFFFFu, x1 = r0 >> 16, y0 = r1 & 0xFFFFu, y1 = (r1 >> 16) & 0x7FFFu;
        keep = x0 <= tx1 && x1 >= tile_x0 && y0 <= ty1 && y1 >= tile_y0;
        columns = (uint32_t)max(x0 - tile_x0, 0) | (uint32_t)min(x1 - tile_x0, MR_TILE_W - 1) << 8;  // of the tile, where kept
      }
      const unsigned long long mask = __ballot(keep);
      if (lane == 0) wave_count[wave] = __popcll(mask);
      __syncthreads();
      int slot = __popcll(mask & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int cnt = wave_count[v];
        slot += v < wave ? cnt : 0;
        kept += cnt;
      }
      if (keep) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];  // in range: the frame kernel checked
        const float4 a = *reinterpret_cast<const float4*>(verts + (int64_t)i0 * MR_VERT);
        const float4 c1 = *reinterpret_cast<const float4*>(verts + (int64_t)i1 * MR_VERT);
        const float4 d = *reinterpret_cast<const float4*>(verts + (int64_t)i2 * MR_VERT);
        const float sg = (r1 & 0x80000000u) ? -1.f : 1.f;
        float* s = stage + slot * MR_STAGE;
        stage_edge(s, s + 12, c1.x, c1.y, d.x, d.y, sg);     // edge 12, opposite vertex 0
        stage_edge(s + 4, s + 13, d.x, d.y, a.x, a.y, sg);   // edge 20, opposite vertex 1
        stage_edge(s + 8, s + 14, a.x, a.y, c1.x, c1.y, sg);  // edge 01, opposite vertex 2
        s[15] = a.z, s[16] = c1.z, s[17] = d.z;
        s[18] = __int_as_float(f);
        s[19] = __uint_as_float(columns);
      }
      __syncthreads();
      for (int j = 0; j < kept; ++j) {
        const float* s = stage + j * MR_STAGE;  // the same address in every lane: an LDS broadcast
        const uint32_t columns = __builtin_amdgcn_readfirstlane(__float_as_uint(s[19]));
        if ((int)(columns & 0xFFu) > block_x1 || (int)(columns >> 8) < block_x0) continue;  // scalar: the box misses the block
        float e[3][4];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float ox = s[4 * q], oy = s[4 * q + 1], dx = s[4 * q + 2], dy = s[4 * q + 3], sg = s[12 + q];
          const float ty = dx * (py - oy);
#pragma unroll
          for (int i = 0; i < 4; ++i) e[q][i] = sg * (ty - dy * ((px + (float)i) - ox));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (e[0][i] >= 0.f && e[1][i] >= 0.f && e[2][i] >= 0.f) {
            const float S = (e[0][i] + e[1][i]) + e[2][i];
            if (S > 0.f) {
              const float l0 = e[0][i] / S, l1 = e[1][i] / S, l2 = e[2][i] / S;
              const float d = (l0 * s[15] + l1 * s[16]) + l2 * s[17];
              if (d > best_d[i]) best_d[i] = d, best_l0[i] = l0, best_l1[i] = l1, best_l2[i] = l2, best_f[i] = __float_as_int(s[18]);
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (!inside) return;
  if (body) {
    const float* verts = pv + fk * V * MR_VERT;
    const float4* vn = reinterpret_cast<const float4*>(pn + fk * V * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = best_f[i];
      if (f < 0) continue;
      const int id[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
      float w[3];
      V3 v[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float4* rec = reinterpret_cast<const float4*>(verts + (int64_t)id[q] * MR_VERT);
        w[q] = rec[0].z;
        const float4 p = rec[1];
        v[q] = {p.x, p.y, p.z};
      }
      const float d = best_d[i];
      const float g0 = best_l0[i] * w[0] / d, g1 = best_l1[i] * w[1] / d, g2 = best_l2[i] * w[2] / d;
      const V3 P = {g0 * v[0].x + g1 * v[1].x + g2 * v[2].x, g0 * v[0].y + g1 * v[1].y + g2 * v[2].y,
                    g0 * v[0].z + g1 * v[1].z + g2 * v[2].z};
      const V3 eu = normalise(P);
      V3 nn;
      if (smooth) {
        const float4 n0 = vn[id[0]], n1 = vn[id[1]], n2 = vn[id[2]];
        nn = normalise({g0 * n0.x + g1 * n1.x + g2 * n2.x, g0 * n0.y + g1 * n1.y + g2 * n2.y, g0 * n0.z + g1 * n1.z + g2 * n2.z});
      } else {
        const V3 a = {v[1].x - v[0].x, v[1].y - v[0].y, v[1].z - v[0].z}, bb = {v[2].x - v[0].x, v[2].y - v[0].y, v[2].z - v[0].z};
        nn = normalise({a.y * bb.z - a.z * bb.y, a.z * bb.x - a.x * bb.z, a.x * bb.y - a.y * bb.x});
      }
      const float ne = -(nn.x * eu.x + nn.y * eu.y + nn.z * eu.z);  // n . e, e = -normalise(P)
      if (ne < 0.f) nn = {-nn.x, -nn.y, -nn.z};
      const float I = arg.ambient + (1.f - arg.ambient) * fmaxf(0.f, nn.x * arg.light[0] + nn.y * arg.light[1] + nn.z * arg.light[2]);
#pragma unroll
      for (int e = 0; e < 3; ++e) c[i][e] = c[i][e] * (1.f - arg.body_alpha) + arg.body_alpha * arg.body_colour[e] * I;
    }
  }
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

// the scratch: slices | frame records | projected vertices | view-space normals | face records, each a multiple of 4 floats
struct MeshScratch { int64_t parts, frame, pv, pn, face, total; };

inline MeshScratch mesh_scratch(int64_t B, int64_t NF, int64_t V, int64_t F, bool with_normals) {
  MeshScratch s;
  s.parts = 0;
  s.frame = s.parts + B * MR_SLICES * MR_PART;
  s.pv = s.frame + B * NF * MR_FRAME;
  s.pn = s.pv + B * NF * V * MR_VERT;
  s.face = s.pn + (with_normals ? B * NF * V * 4 : 0);
  s.total = s.face + ((B * NF * F * 2 + 3) / 4) * 4;
  return s;
}

inline bool sizes_ok(int32_t B, int32_t T, int32_t V, int32_t F, int32_t NF) {
  return B >= 0 && T >= 1 && V >= 1 && V <= (1 << 24) && F >= 1 && F <= (1 << 24) && NF >= 0;
}

}  // namespace
}  // namespace mdm

extern "C" {

int64_t mdm_mesh_render_scratch_floats(int32_t B, int32_t T, int32_t n_frames, int32_t V, int32_t F, int32_t with_normals) {
  if (!mdm::sizes_ok(B, T, V, F, n_frames)) return -1;
  return mdm::mesh_scratch(B, n_frames, V, F, with_normals != 0).total;
}

int mdm_mesh_render(const float* vertices, const float* normals, const int32_t* faces, const float* root, const int32_t* length,
                    int32_t B, int32_t T, int32_t V, int32_t F, int32_t H, int32_t W, const float* camera, const float* style,
                    int32_t mode, const int32_t* frames, int32_t n_frames, uint8_t* out, float* scratch, void* stream) {
  if (!vertices || !faces || !root || !camera || !style || !out || !scratch) return MDM_ERR_ARG;
  if (!mdm::sizes_ok(B, T, V, F, 0) || H < 4 || W < 4 || H > mdm::MR_MAX_SIDE || W > mdm::MR_MAX_SIDE || W % 4) return MDM_ERR_ARG;
  if (mode < 0 || mode > 3) return MDM_ERR_ARG;  // bit 0: palette; bit 1: shade from the normals
  if ((mode & 2) && !normals) return MDM_ERR_ARG;
  if (frames && n_frames < 1) return MDM_ERR_ARG;
  if ((uintptr_t)out % 4 || (uintptr_t)scratch % 16) return MDM_ERR_ARG;  // written as dwords; read as float4
  const double elev = camera[0], azim = camera[1], dist = camera[2], fov = camera[3], near = camera[7];
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(camera[i])) return MDM_ERR_ARG;
  if (!(std::fabs(elev) < 89.9) || !(dist > 0) || !(near > 0) || !(near < dist) || !(fov > 0) || !(fov < 180)) return MDM_ERR_ARG;
  for (int i = 0; i < 20; ++i)
    if (!std::isfinite(style[i])) return MDM_ERR_ARG;
  const double lx = style[17], ly = style[18], lz = style[19], ll = std::sqrt(lx * lx + ly * ly + lz * lz);
  if (style[11] < 0.f || !(ll > 0)) return MDM_ERR_ARG;  // the trajectory's width, a light without direction
  mdm::MeshArg arg = {};
  const double rad = 3.14159265358979323846 / 180.0;
  const double ce = std::cos(elev * rad), se = std::sin(elev * rad), ca = std::cos(azim * rad), sa = std::sin(azim * rad);
  const double back[3] = {ce * sa, se, ce * ca};
  const double f[3] = {-back[0], -back[1], -back[2]};
  double r[3] = {f[1] * 0 - f[2] * 1, f[2] * 0 - f[0] * 0, f[0] * 1 - f[1] * 0};
  const double rn = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int e = 0; e < 3; ++e) r[e] /= rn;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  for (int e = 0; e < 3; ++e) {
    arg.eye[e] = (float)(camera[4 + e] + dist * back[e]);
    arg.r[e] = (float)r[e], arg.u[e] = (float)u[e], arg.f[e] = (float)f[e];
    arg.bg[e] = style[e], arg.floor_colour[e] = style[3 + e], arg.traj_colour[e] = style[7 + e], arg.body_colour[e] = style[12 + e];
  }
  arg.F = (float)(0.5 * H / std::tan(0.5 * fov * rad));
  arg.near = (float)near, arg.cx = 0.5f * W, arg.cy = 0.5f * H;
  arg.floor_alpha = style[6], arg.traj_alpha = style[10], arg.traj_halfw = (float)((double)style[11] * H / 1440.0);
  arg.body_alpha = style[15], arg.ambient = style[16];
  arg.light[0] = (float)(lx / ll), arg.light[1] = (float)(ly / ll), arg.light[2] = (float)(-lz / ll);  // towards the eye is -f
  const int NF = frames ? n_frames : T;
  const int tiles_x = (W + mdm::MR_TILE_W - 1) / mdm::MR_TILE_W, tiles_y = (H + mdm::MR_TILE_H - 1) / mdm::MR_TILE_H;
  if (B > 65535 || NF > 65535) return MDM_ERR_UNSUPPORTED;  // grid limits
  if (B == 0 || NF == 0) return MDM_OK;
  const mdm::MeshScratch s = mdm::mesh_scratch(B, NF, V, F, (mode & 2) != 0);
  float* parts = scratch + s.parts;
  float* frame_rec = scratch + s.frame;
  float* pv = scratch + s.pv;
  float* pn = scratch + s.pn;
  uint32_t* face_rec = reinterpret_cast<uint32_t*>(scratch + s.face);
  hipLaunchKernelGGL(mdm::mesh_extent_kernel, dim3(mdm::MR_SLICES, B), dim3(mdm::MR_THREADS), 0, (hipStream_t)stream, vertices,
                     length, T, V, parts);
  MDM_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(mdm::mesh_frame_kernel, dim3(NF, B), dim3(mdm::MR_THREADS), 0, (hipStream_t)stream, vertices,
                     (mode & 2) ? normals : (const float*)nullptr, faces, root, length, arg, T, V, F, H, W, frames, NF,
                     (const float*)parts, frame_rec, pv, pn, face_rec);
  MDM_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(mdm::mesh_raster_kernel, dim3(tiles_x * tiles_y, NF, B), dim3(mdm::MR_THREADS), 0, (hipStream_t)stream, faces,
                     root, length, arg, T, V, F, H, W, tiles_x, frames, NF, mode & 1, (mode & 2) >> 1, (const float*)parts,
                     (const float*)frame_rec, (const float*)pv, (const float*)pn, (const uint32_t*)face_rec, out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
