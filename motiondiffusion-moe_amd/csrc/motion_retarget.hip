// Rig retargeting on the device: the joints and global bone rotations of mdm_motion_fk / mdm_foot_skate -> the
// channels of a given BVH hierarchy (a Mixamo skeleton, a CMU-style rig), retimed.  The hierarchy is data: the host
// (motion_rig.target_rig) derives, in float64, one table per target, which travels as one device buffer (RT_WORDS 32-bit words;
// 128 nodes do not fit a kernel argument).
//   Launch 1, per (sample, source frame t, node): the node's global rotation G in the file's axes.
//     res[node] is the nearest node at or above it that has a rule of its own, or -1 (G = I); nodes without one turn with it.
//     COPY: G = basis^T R[src] M, M = basis A, A the shortest arc from the target's rest direction to the source's rest axis.
//     FIT:  G = basis^T F(cur) M, M = F(rest)^T, F(a, b) the frame e1 = unit(a), e3 = unit(e1 x b), e2 = e3 x e1 as columns;
//           a = x[fa] - x[fb], b = the sum of the unit directions from x[src] to x[bj[.]].  A frame whose a or e1 x b has no
//           length takes G = basis^T R[src] basis, the joint's own rotation.
//     Leg IK (thigh and shin nodes): the hip from the walk up to the root with the G above, the ankle's target s basis^T x[ankle],
//     the reach clamped to [|l1 - l2| + eps, l1 + l2 - eps], the knee on the side of the source's knee, and G = swing * G, the
//     swing the shortest arc from the copied bone direction to the solved one (as a unit quaternion: a rotation whatever the
//     angle; two opposite directions turn about unit(u x e_m), m the axis of u's smallest component, lowest index on ties).
//   Launch 2, per (sample, output frame k, node): L = G[parent]^T G[node] at t0 (and t0 + 1) -> quaternion -> slerp -> Euler
//     angles in degrees, the arithmetic and the integer retiming of motion_rig.hip (rig_math.h); the root's position channels
//     are s basis^T lerp(x[0]) - OFFSET[root], s = the target's leg length over the sample's.
// One thread per item in a grid-stride loop, plain loads and stores, no LDS, any T.  Source frames at or past a length are
// never read; the globals there and the channels at or past length_out are zero.
#include "rig_math.h"

namespace mdm {
namespace {

using namespace rigmath;

constexpr int RT_THREADS = 256;
constexpr int RT_MAX_NODES = 128;
constexpr int RT_MAX_JOINTS = 32;
constexpr int RT_MAX_B = 8;  // the children summed into b of a fitted node
// the table, in 32-bit words: integers, then floats
constexpr int RT_I_HEAD = 16;   // n_nodes, joints, leg_ok, 0, then per leg: hip, knee, ankle joint, thigh node, shin node, 0
constexpr int RT_I_NODE = 16;   // parent, res, kind, src, fa, fb, nb, bj[8], 0
constexpr int RT_F_BASE = RT_I_HEAD + RT_I_NODE * RT_MAX_NODES;
constexpr int RT_F_HEAD = 32;   // basis[9], the target's leg length, then per leg: l1, l2, u1[3], u2[3]
constexpr int RT_F_NODE = 12;   // OFFSET[3], M[9]
constexpr int RT_WORDS = RT_F_BASE + RT_F_HEAD + RT_F_NODE * RT_MAX_NODES;
enum { RT_NONE = 0, RT_COPY = 1, RT_FIT = 2 };

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 sub(const V3& a, const V3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(const V3& a, const V3& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3 axpy(float s, const V3& a, const V3& b) { return {s * a.x + b.x, s * a.y + b.y, s * a.z + b.z}; }
__device__ __forceinline__ V3 load3(const float* __restrict__ p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 apply(const R3& a, const V3& v) {
  return {a.m[0][0] * v.x + a.m[0][1] * v.y + a.m[0][2] * v.z, a.m[1][0] * v.x + a.m[1][1] * v.y + a.m[1][2] * v.z,
          a.m[2][0] * v.x + a.m[2][1] * v.y + a.m[2][2] * v.z};
}
__device__ __forceinline__ V3 tapply(const R3& a, const V3& v) {  // a^T v
  return {a.m[0][0] * v.x + a.m[1][0] * v.y + a.m[2][0] * v.z, a.m[0][1] * v.x + a.m[1][1] * v.y + a.m[2][1] * v.z,
          a.m[0][2] * v.x + a.m[1][2] * v.y + a.m[2][2] * v.z};
}
__device__ __forceinline__ R3 matmul(const R3& a, const R3& b) {
  R3 o;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o.m[r][c] = a.m[r][0] * b.m[0][c] + a.m[r][1] * b.m[1][c] + a.m[r][2] * b.m[2][c];
  return o;
}
__device__ __forceinline__ R3 identity() { return {{{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}}}; }

// a unit vector across the unit vector u: unit(u x e_m), m the axis of u's smallest component, the lowest index on ties
__device__ __forceinline__ V3 across(const V3& u) {
  const float ax = fabsf(u.x), ay = fabsf(u.y), az = fabsf(u.z);
  V3 k;
  if (ax <= ay && ax <= az) k = {0.f, u.z, -u.y};
  else if (ay <= az) k = {-u.z, 0.f, u.x};
  else k = {u.y, -u.x, 0.f};
  const float s = 1.f / sqrtf(dot(k, k));
  return {k.x * s, k.y * s, k.z * s};
}

// the shortest arc taking the unit vector u onto the unit vector v, as the quaternion (1 + u.v, u x v) normalised
__device__ __forceinline__ R3 arc(const V3& u, const V3& v) {
  const V3 k = cross(u, v);
  const float w = 1.f + dot(u, v);
  Q4 q;
  if (w * w + dot(k, k) < 1e-12f) {  // opposite: half a turn about the fixed axis across u
    const V3 h = across(u);
    q = {0.f, h.x, h.y, h.z};
  } else {
    q = normalised({w, k.x, k.y, k.z});
  }
  return quat_matrix(q);
}

struct Tables {
  const int* __restrict__ I;
  const float* __restrict__ F;
  __device__ __forceinline__ const int* node(int n) const { return I + RT_I_HEAD + RT_I_NODE * n; }
  __device__ __forceinline__ const float* fnode(int n) const { return F + RT_F_HEAD + RT_F_NODE * n; }
  __device__ __forceinline__ R3 basis() const { return load_rot(F, 0); }
};

// s of DESIGN.md §27: the target's leg length over the sample's, thigh + shin, left and right averaged
__device__ __forceinline__ float leg_scale(const Tables& tb, const float* __restrict__ off) {
  float src = 0.f;
  for (int l = 0; l < 2; ++l) {
    const int* leg = tb.I + 4 + 6 * l;
    const V3 a = load3(off + 3 * leg[1]), c = load3(off + 3 * leg[2]);
    src += sqrtf(dot(a, a)) + sqrtf(dot(c, c));
  }
  return tb.F[9] / (0.5f * src);
}

// the global rotation, in the file's axes, of a node that has a rule of its own, before the leg IK
__device__ __forceinline__ R3 rule_global(const Tables& tb, int n, const float* __restrict__ x, const float* __restrict__ r) {
  const int* nd = tb.node(n);
  const R3 bs = tb.basis();
  const int src = nd[3];
  const R3 M = load_rot(tb.fnode(n) + 3, 0);
  R3 cur = load_rot(r, src);
  bool fitted = false;
  if (nd[2] == RT_FIT) {
    const V3 at = load3(x + 3 * src);
    const V3 a = sub(load3(x + 3 * nd[4]), load3(x + 3 * nd[5]));
    V3 b = {0.f, 0.f, 0.f};
    for (int i = 0; i < nd[6]; ++i) {
      const V3 d = sub(load3(x + 3 * nd[7 + i]), at);
      const float dd = dot(d, d);
      if (dd > 0.f) b = axpy(1.f / sqrtf(dd), d, b);
    }
    const float aa = dot(a, a);
    if (aa > 1e-20f) {
      const float ia = 1.f / sqrtf(aa);
      const V3 e1 = {a.x * ia, a.y * ia, a.z * ia};
      const V3 c3 = cross(e1, b);
      const float cc = dot(c3, c3);
      if (cc > 1e-12f) {
        const float ic = 1.f / sqrtf(cc);
        const V3 e3 = {c3.x * ic, c3.y * ic, c3.z * ic};
        const V3 e2 = cross(e3, e1);
        cur = {{{e1.x, e2.x, e3.x}, {e1.y, e2.y, e3.y}, {e1.z, e2.z, e3.z}}};
        fitted = true;
      }
    }
  }
  const R3 world = matmul(cur, (nd[2] == RT_FIT && !fitted) ? bs : M);  // the per-frame fallback: the joint's own R
  return tmatmul(bs, world);
}

__device__ __forceinline__ R3 resolved_global(const Tables& tb, int res, const float* __restrict__ x, const float* __restrict__ r) {
  return res < 0 ? identity() : rule_global(tb, res, x, r);
}

// thigh (part 0) or shin (part 1) of leg l after the two-bone IK
__device__ __forceinline__ R3 leg_global(const Tables& tb, int l, int part, float s, const float* __restrict__ x,
                                         const float* __restrict__ r) {
  const int* leg = tb.I + 4 + 6 * l;
  const float* lf = tb.F + 10 + 8 * l;
  const float l1 = lf[0], l2 = lf[1];
  const R3 bs = tb.basis();
  const R3 g_thigh = rule_global(tb, leg[3], x, r), g_shin = rule_global(tb, leg[4], x, r);
  const V3 c1 = apply(g_thigh, load3(lf + 2)), c2 = apply(g_shin, load3(lf + 5));  // the copied bone directions
  // the hip: from the thigh node up to the root, with the globals already decided
  const V3 root = tapply(bs, load3(x));
  V3 hip = {s * root.x, s * root.y, s * root.z};
  for (int a = leg[3]; tb.node(a)[0] >= 0; a = tb.node(a)[0]) {
    const R3 gp = resolved_global(tb, tb.node(tb.node(a)[0])[1], x, r);
    const V3 o = apply(gp, load3(tb.fnode(a)));
    hip = {hip.x + o.x, hip.y + o.y, hip.z + o.z};
  }
  const V3 xh = load3(x + 3 * leg[0]), xk = load3(x + 3 * leg[1]);
  const V3 ank = tapply(bs, load3(x + 3 * leg[2]));
  const V3 d = {s * ank.x - hip.x, s * ank.y - hip.y, s * ank.z - hip.z};
  const float dist = sqrtf(dot(d, d));
  const float eps = 1e-4f * (l1 + l2);
  V3 n = c1;  // a target at the hip: along the copied thigh
  if (dist > 1e-6f * (l1 + l2)) n = {d.x / dist, d.y / dist, d.z / dist};
  const float reach = fminf(fmaxf(dist, fabsf(l1 - l2) + eps), l1 + l2 - eps);
  // the pole: the source's knee off the hip-ankle line; a straight source leg takes the copied thigh's side, then the fixed axis
  const V3 w = tapply(bs, sub(xk, xh));
  V3 pole = axpy(-dot(w, n), n, w);
  float pp = dot(pole, pole);
  if (pp <= 1e-10f * dot(w, w)) {
    pole = axpy(-dot(c1, n), n, c1);
    pp = dot(pole, pole);
    if (pp <= 1e-10f) pole = across(n), pp = 1.f;
  }
  const float ip = 1.f / sqrtf(pp);
  const float ca = fminf(fmaxf((l1 * l1 + reach * reach - l2 * l2) / (2.f * l1 * reach), -1.f), 1.f);
  const float sa = sqrtf(fmaxf(1.f - ca * ca, 0.f));
  const V3 d1 = {ca * n.x + sa * ip * pole.x, ca * n.y + sa * ip * pole.y, ca * n.z + sa * ip * pole.z};  // unit: n and pole are across
  if (part == 0) return matmul(arc(c1, d1), g_thigh);
  V3 d2 = {reach * n.x - l1 * d1.x, reach * n.y - l1 * d1.y, reach * n.z - l1 * d1.z};
  const float i2 = 1.f / sqrtf(dot(d2, d2));  // |d2| = l2 > 0
  d2 = {d2.x * i2, d2.y * i2, d2.z * i2};
  return matmul(arc(c2, d2), g_shin);
}

__global__ __launch_bounds__(RT_THREADS) void retarget_globals_kernel(
    const float* __restrict__ joints, const float* __restrict__ rot, const float* __restrict__ offsets,
    const int* __restrict__ len, const int* __restrict__ tab, int B, int T, int J, int N, int leg_ik, float* __restrict__ globals) {
  const Tables tb = {tab, reinterpret_cast<const float*>(tab) + RT_F_BASE};
  const int64_t total = (int64_t)B * T * N;
  for (int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RT_THREADS) {
    const int node = (int)(i % N);
    const int64_t bt = i / N;
    const int t = (int)(bt % T), b = (int)(bt / T);
    int n = len ? len[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    float* out = globals + i * 9;
    if (t >= n) {  // past the length: zeros, and the frame is not read
      for (int e = 0; e < 9; ++e) out[e] = 0.f;
      continue;
    }
    const float* x = joints + bt * J * 3;
    const float* r = rot + bt * J * 9;
    const int res = tb.node(node)[1];
    R3 g;
    int l = -1, part = 0;
    if (leg_ik && res >= 0) {
      for (int k = 0; k < 2; ++k) {
        if (res == tb.I[4 + 6 * k + 3]) l = k, part = 0;
        if (res == tb.I[4 + 6 * k + 4]) l = k, part = 1;
      }
    }
    if (l >= 0) g = leg_global(tb, l, part, leg_scale(tb, offsets + (int64_t)b * J * 3), x, r);
    else g = resolved_global(tb, res, x, r);
    for (int rr = 0; rr < 3; ++rr)
      for (int c = 0; c < 3; ++c) out[3 * rr + c] = g.m[rr][c];
  }
}

template <int AX0, int AX1, int AX2>
__global__ __launch_bounds__(RT_THREADS) void retarget_channels_kernel(
    const float* __restrict__ joints, const float* __restrict__ globals, const float* __restrict__ offsets,
    const int* __restrict__ len, const int* __restrict__ tab, int B, int T, int J, int N, int num, int den, int T_out,
    const int* __restrict__ len_out, float* __restrict__ chan) {
  const Tables tb = {tab, reinterpret_cast<const float*>(tab) + RT_F_BASE};
  const int C = 3 + 3 * N;
  const float deg = 57.29577951308232f;
  const int64_t total = (int64_t)B * T_out * N;
  for (int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RT_THREADS) {
    const int node = (int)(i % N);
    const int64_t bk = i / N;
    const int k = (int)(bk % T_out), b = (int)(bk / T_out);
    int n = len ? len[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    const int n_out = len_out ? len_out[b] : T_out;
    const int64_t kd = (int64_t)k * den;
    const int64_t t0 = kd / num;
    const int rem = (int)(kd - t0 * num);
    float* ch = chan + bk * C;
    if (k >= n_out || t0 >= n) {  // past the length: zeros, and no source frame is read
      if (node == 0) ch[0] = 0.f, ch[1] = 0.f, ch[2] = 0.f;
      ch[3 + 3 * node] = 0.f, ch[4 + 3 * node] = 0.f, ch[5 + 3 * node] = 0.f;
      continue;
    }
    const bool two = rem != 0 && t0 + 1 < n;  // frame t0 + 1 is read only where it is needed and valid
    const float f = two ? (float)rem / (float)num : 0.f;
    const int par = tb.node(node)[0];
    const float* g0 = globals + ((int64_t)b * T + t0) * N * 9;
    Q4 q = matrix_quat(tmatmul(load_rot(g0, par), load_rot(g0, node)));
    if (two) q = slerp(q, matrix_quat(tmatmul(load_rot(g0 + (int64_t)N * 9, par), load_rot(g0 + (int64_t)N * 9, node))), f);
    float a, bb, c;
    euler_angles<AX0, AX1, AX2>(quat_matrix(q), a, bb, c);
    ch[3 + 3 * node] = a * deg, ch[4 + 3 * node] = bb * deg, ch[5 + 3 * node] = c * deg;
    if (node == 0) {
      const float* p0 = joints + ((int64_t)b * T + t0) * J * 3;
      V3 v = load3(p0);
      if (two) {
        const V3 v1 = load3(p0 + (int64_t)J * 3);
        v = {v.x + f * (v1.x - v.x), v.y + f * (v1.y - v.y), v.z + f * (v1.z - v.z)};
      }
      const float s = leg_scale(tb, offsets + (int64_t)b * J * 3);
      const V3 p = tapply(tb.basis(), v);
      const float* o = tb.fnode(0);
      ch[0] = s * p.x - o[0], ch[1] = s * p.y - o[1], ch[2] = s * p.z - o[2];
    }
  }
}

inline bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!(p[i] - p[i] == 0.f)) return false;
  return true;
}

// the table's own consistency, on the host copy: every index the kernels follow lies inside its array
bool tables_ok(const int32_t* I, int J, int leg_ik) {
  const float* F = reinterpret_cast<const float*>(I) + RT_F_BASE;
  const int N = I[0];
  if (N < 1 || N > RT_MAX_NODES || I[1] != J || J < 1 || J > RT_MAX_JOINTS) return false;
  if (!finite_all(F, RT_F_HEAD + RT_F_NODE * N) || !(F[9] > 0.f)) return false;
  for (int n = 0; n < N; ++n) {
    const int32_t* nd = I + RT_I_HEAD + RT_I_NODE * n;
    if (n == 0 ? nd[0] != -1 : (nd[0] < 0 || nd[0] >= n)) return false;
    const int kind = nd[2];
    if (kind != RT_NONE && kind != RT_COPY && kind != RT_FIT) return false;
    if (kind == RT_NONE) {  // turns with the node its parent resolves to
      if (nd[1] != (n == 0 ? -1 : I[RT_I_HEAD + RT_I_NODE * nd[0] + 1])) return false;
      continue;
    }
    if (nd[1] != n || nd[3] < 0 || nd[3] >= J) return false;
    if (kind == RT_FIT) {
      if (nd[4] < 0 || nd[4] >= J || nd[5] < 0 || nd[5] >= J || nd[6] < 1 || nd[6] > RT_MAX_B) return false;
      for (int i = 0; i < nd[6]; ++i)
        if (nd[7 + i] < 0 || nd[7 + i] >= J) return false;
    }
  }
  const bool leg_ok = I[2] != 0;
  if (leg_ik && !leg_ok) return false;
  for (int l = 0; l < 2; ++l) {
    const int32_t* leg = I + 4 + 6 * l;
    for (int e = 0; e < 3; ++e)
      if (leg[e] < 0 || leg[e] >= J) return false;
    if (!leg_ok) continue;
    const float* lf = F + 10 + 8 * l;
    if (!(lf[0] > 0.f) || !(lf[1] > 0.f)) return false;
    for (int e = 3; e < 5; ++e)  // thigh and shin nodes copy a rotation
      if (leg[e] < 1 || leg[e] >= N || I[RT_I_HEAD + RT_I_NODE * leg[e] + 2] != RT_COPY) return false;
    if (leg[3] == leg[4]) return false;
  }
  return true;
}

}  // namespace
}  // namespace mdm

extern "C" {

int64_t mdm_retarget_table_words(void) { return mdm::RT_WORDS; }

int mdm_retarget_channels(const float* joints, const float* rotations, const float* offsets, const int32_t* length, int32_t B,
                          int32_t T, int32_t J, const int32_t* tables_host, const int32_t* tables_dev, int32_t leg_ik,
                          int32_t axis0, int32_t axis1, int32_t axis2, int32_t num, int32_t den, int32_t T_out,
                          const int32_t* length_out, float* globals_out, float* channels_out, void* stream) {
  if (!joints || !rotations || !offsets || !tables_host || !tables_dev || !globals_out || !channels_out) return MDM_ERR_ARG;
  if (B < 0 || T < 1 || T_out < 1 || num < 1 || den < 1 || (leg_ik != 0 && leg_ik != 1)) return MDM_ERR_ARG;
  if (axis0 < 0 || axis0 > 2 || axis1 < 0 || axis1 > 2 || axis2 < 0 || axis2 > 2) return MDM_ERR_ARG;
  if (((1 << axis0) | (1 << axis1) | (1 << axis2)) != 7) return MDM_ERR_ARG;
  if ((int64_t)(T_out - 1) * den > (int64_t)(T - 1) * num) return MDM_ERR_ARG;  // the last output frame lies past the source
  if (!mdm::tables_ok(tables_host, J, leg_ik)) return MDM_ERR_ARG;
  if (B == 0) return MDM_OK;
  const int N = tables_host[0];
  auto grid_of = [](int64_t total) {
    const int64_t blocks = (total + mdm::RT_THREADS - 1) / mdm::RT_THREADS;
    return (int)(blocks < 4096 ? blocks : 4096);
  };
  hipLaunchKernelGGL(mdm::retarget_globals_kernel, dim3(grid_of((int64_t)B * T * N)), dim3(mdm::RT_THREADS), 0,
                     (hipStream_t)stream, joints, rotations, offsets, length, tables_dev, B, T, J, N, leg_ik, globals_out);
  MDM_RETURN_IF_LAUNCH_FAILED();
  const int grid = grid_of((int64_t)B * T_out * N);
#define MDM_RT_LAUNCH(A0, A1, A2)                                                                                            \
  hipLaunchKernelGGL((mdm::retarget_channels_kernel<A0, A1, A2>), dim3(grid), dim3(mdm::RT_THREADS), 0, (hipStream_t)stream, \
                     joints, globals_out, offsets, length, tables_dev, B, T, J, N, num, den, T_out, length_out, channels_out)
  switch (9 * axis0 + 3 * axis1 + axis2) {
    case 5: MDM_RT_LAUNCH(0, 1, 2); break;
    case 7: MDM_RT_LAUNCH(0, 2, 1); break;
    case 11: MDM_RT_LAUNCH(1, 0, 2); break;
    case 15: MDM_RT_LAUNCH(1, 2, 0); break;
    case 19: MDM_RT_LAUNCH(2, 0, 1); break;
    default: MDM_RT_LAUNCH(2, 1, 0); break;
  }
#undef MDM_RT_LAUNCH
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
