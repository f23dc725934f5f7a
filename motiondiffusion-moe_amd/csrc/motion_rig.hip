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
#include "rig_math.h"

namespace mdm {
namespace {

constexpr int RIG_THREADS = 256;
constexpr int RIG_MAX_NODES = 64;

struct RigArg {
  int n;
  int parent[RIG_MAX_NODES];  // parent node, -1 at the root
  int src[RIG_MAX_NODES];     // the joint whose R is the node's G, inherited from the nearest ancestor that carries one; -1: identity
};

using namespace rigmath;

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
