// Rig export on the device: the global rotations of mdm_motion_fk / mdm_foot_skate -> the channels of a node
// tree that a BVH reader can load, retimed to another frame rate.
//   R[c] of mdm_motion_fk orients the bone parent(c) -> c and every chain starts from the root matrix, so a joint with several
//   children has one rotation per outgoing bone.  The host turns the skeleton into a node tree (motion_rig.rig_of): a node
//   carries the R of one joint as its global rotation G, or nothing (G = its parent node's G).  Here, per (sample, output
//   frame k, node): source time k den / num in integers, t0 = (k den) / num, frac = ((k den) % num) / num; the local rotation
//   G[parent]^T G[node] at t0 and t0 + 1 -> unit quaternions (the four branches of the trace test, normalised) -> the second
//   flipped onto the first one's hemisphere -> slerp at frac (lerp where the two nearly coincide) -> normalised -> matrix ->
//   Euler angles in degrees of L = R_A(a) R_B(b) R_C(c).  Root position: scale * lerp(joint0[t0], joint0[t0 + 1], frac).
// Where frac == 0 frame t0 + 1 is not read and no slerp runs: at num == den the result is the frame's own rotation.
// One thread per (sample, frame, node) in a grid-stride loop; plain loads and stores, no LDS, nothing serial, any T.
// Memory-bound and tiny: 4 matrices in, 3 angles (and a quaternion) out per thread.
#include "kernels.h"

namespace mdm {
namespace {

constexpr int RIG_THREADS = 256;
constexpr int RIG_MAX_NODES = 64;

struct RigArg {
  int n;
  int parent[RIG_MAX_NODES];  // parent node, -1 at the root
  int src[RIG_MAX_NODES];     // the joint whose R is the node's G, inherited from the nearest ancestor that carries one; -1: identity
};

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

template <int AX0, int AX1, int AX2>
__global__ __launch_bounds__(RIG_THREADS) void rig_channels_kernel(
    const float* __restrict__ joints, const float* __restrict__ rot, const int* __restrict__ len, const RigArg rig, int B, int T,
    int J, float scale, int num, int den, int T_out, const int* __restrict__ len_out, float* __restrict__ chan,
    float* __restrict__ quat) {
  const int N = rig.n, C = 3 + 3 * N;
  const float deg = 57.29577951308232f;
  const int64_t total = (int64_t)B * T_out * N;
  for (int64_t i = (int64_t)blockIdx.x * RIG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RIG_THREADS) {
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
    float* qo = quat ? quat + i * 4 : nullptr;
    if (k >= n_out || t0 >= n) {  // past the length: zeros, and no source frame is read
      if (node == 0) ch[0] = 0.f, ch[1] = 0.f, ch[2] = 0.f;
      ch[3 + 3 * node] = 0.f, ch[4 + 3 * node] = 0.f, ch[5 + 3 * node] = 0.f;
      if (qo) qo[0] = 0.f, qo[1] = 0.f, qo[2] = 0.f, qo[3] = 0.f;
      continue;
    }
    const bool two = rem != 0 && t0 + 1 < n;  // frame t0 + 1 is read only where it is needed and valid
    const float f = two ? (float)rem / (float)num : 0.f;
    const int par = rig.parent[node], src = rig.src[node], psrc = par < 0 ? -1 : rig.src[par];
    const float* r0 = rot + ((int64_t)b * T + t0) * J * 9;
    Q4 q = matrix_quat(tmatmul(load_rot(r0, psrc), load_rot(r0, src)));
    if (two) q = slerp(q, matrix_quat(tmatmul(load_rot(r0 + (int64_t)J * 9, psrc), load_rot(r0 + (int64_t)J * 9, src))), f);
    float a, bb, c;
    euler_angles<AX0, AX1, AX2>(quat_matrix(q), a, bb, c);
    ch[3 + 3 * node] = a * deg, ch[4 + 3 * node] = bb * deg, ch[5 + 3 * node] = c * deg;
    if (qo) qo[0] = q.w, qo[1] = q.x, qo[2] = q.y, qo[3] = q.z;
    if (node == 0) {
      const float* p0 = joints + ((int64_t)b * T + t0) * J * 3;
      for (int e = 0; e < 3; ++e) {
        float v = p0[e];
        if (two) v = v + f * (p0[(int64_t)J * 3 + e] - v);
        ch[e] = scale * v;
      }
    }
  }
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_rig_channels(const float* joints, const float* rotations, const int32_t* length, int32_t B, int32_t T, int32_t J,
                     int32_t n_nodes, const int32_t* parent, const int32_t* carried, int32_t axis0, int32_t axis1,
                     int32_t axis2, float scale, int32_t num, int32_t den, int32_t T_out, const int32_t* length_out,
                     float* channels_out, float* quaternions_out, void* stream) {
  if (!joints || !rotations || !parent || !carried || !channels_out || B < 0 || T < 1 || J < 1 || T_out < 1) return MDM_ERR_ARG;
  if (n_nodes < 1 || n_nodes > mdm::RIG_MAX_NODES || num < 1 || den < 1) return MDM_ERR_ARG;
  const int seen = (1 << axis0) | (1 << axis1) | (1 << axis2);
  if (axis0 < 0 || axis0 > 2 || axis1 < 0 || axis1 > 2 || axis2 < 0 || axis2 > 2 || seen != 7) return MDM_ERR_ARG;
  if ((int64_t)(T_out - 1) * den > (int64_t)(T - 1) * num) return MDM_ERR_ARG;  // the last output frame lies past the source
  mdm::RigArg rig;
  rig.n = n_nodes;
  for (int n = 0; n < n_nodes; ++n) {
    const int p = parent[n], c = carried[n];
    if ((n == 0 ? p != -1 : (p < 0 || p >= n)) || c < -1 || c >= J) return MDM_ERR_ARG;
    rig.parent[n] = p;
    rig.src[n] = c >= 0 ? c : (p < 0 ? -1 : rig.src[p]);  // parents come first, so theirs is settled
  }
  for (int n = n_nodes; n < mdm::RIG_MAX_NODES; ++n) rig.parent[n] = -1, rig.src[n] = -1;
  if (B == 0) return MDM_OK;
  const int64_t total = (int64_t)B * T_out * n_nodes;
  const int64_t blocks = (total + mdm::RIG_THREADS - 1) / mdm::RIG_THREADS;
  const int grid = (int)(blocks < 4096 ? blocks : 4096);
#define MDM_RIG_LAUNCH(A0, A1, A2)                                                                                              \
  hipLaunchKernelGGL((mdm::rig_channels_kernel<A0, A1, A2>), dim3(grid), dim3(mdm::RIG_THREADS), 0, (hipStream_t)stream, joints, \
                     rotations, length, rig, B, T, J, scale, num, den, T_out, length_out, channels_out, quaternions_out)
  switch (9 * axis0 + 3 * axis1 + axis2) {
    case 5: MDM_RIG_LAUNCH(0, 1, 2); break;
    case 7: MDM_RIG_LAUNCH(0, 2, 1); break;
    case 11: MDM_RIG_LAUNCH(1, 0, 2); break;
    case 15: MDM_RIG_LAUNCH(1, 2, 0); break;
    case 19: MDM_RIG_LAUNCH(2, 0, 1); break;
    default: MDM_RIG_LAUNCH(2, 1, 0); break;
  }
#undef MDM_RIG_LAUNCH
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
