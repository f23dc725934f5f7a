// Linear blend skinning on the device: the joints and global rotations of mdm_motion_fk / mdm_foot_skate /
// mdm_limb_pin move the vertices of a mesh.
//   Bone 0 is the root (rotation R[0], pivot joint 0); bone c >= 1 is the segment parent(c) -> c (rotation R[c], pivot joint
//   parent(c)), the convention of csrc/motion_fk.hip.  With M_c = R[t, c] Q[c]^T and the bind pivot g_c = G[pivot(c)]:
//     A_c(x)  = P[t, pivot(c)] + M_c (x - g_c)
//     v'[t,i] = sum_k w[i,k] A_{idx[i,k]}(v[i])          n'[t,i] = normalise(sum_k w[i,k] M_{idx[i,k]} n[i])
//   The weights of a vertex sum to 1 (motion_mesh.Mesh sees to it), so the sum is evaluated as a displacement,
//     v' = v + sum_k w_k ((P - g) + (M y - y)),   y = v - g,
//   which rounds at the size of the displacement and not of the position, and in which identity rotations with P = G give the
//   rest vertices bit for bit (M y is y exactly, P - g is 0).
// One workgroup: SKIN_THREADS vertices x SKIN_FRAMES frames of one sample.  The J maps of a frame (M and P - g, 12 floats) are
// built once per workgroup in LDS; a thread owns one vertex, holds its rest position, normal, indices, weights and bind pivots
// in registers and walks the frames, so mesh data is read once per frame tile.  A slot of weight 0 is skipped (its index is
// never used); a live index is clamped into [0, J).  Frames at or past the length are written as zeros and never read.
// Plain 12-byte stores, consecutive lanes on consecutive vertices (768 contiguous bytes a wave), 64-bit offsets.  Staging a
// wave's (64, 3) result through LDS to store whole 16-byte lines measured 10 % slower and is not kept.
#include "kernels.h"

namespace mdm {
namespace {

constexpr int SKIN_THREADS = 256;
constexpr int SKIN_FRAMES = 16;
constexpr int SKIN_MAX_JOINTS = 32;

struct SkinArg {
  int pivot[SKIN_MAX_JOINTS];  // the joint a bone turns about: 0 for bone 0, parent(c) for bone c
};

// arg.pivot[c] for a c that differs from lane to lane: selects over the kernel arguments, no private copy of the table
__device__ __forceinline__ int pivot_of(const SkinArg& arg, int c) {
  int p = 0;
#pragma unroll
  for (int k = 0; k < SKIN_MAX_JOINTS; ++k) p = k == c ? arg.pivot[k] : p;
  return p;
}

template <bool NORMALS>
__global__ __launch_bounds__(SKIN_THREADS) void skin_vertices_kernel(
    const float* __restrict__ joints, const float* __restrict__ rot, const int* __restrict__ len, const SkinArg arg, int T, int J,
    const float* __restrict__ verts, const float* __restrict__ norms, int V, int64_t vert_stride, const float* __restrict__ bind,
    int64_t bind_stride, const float* __restrict__ bind_rot, const int* __restrict__ bone, const float* __restrict__ weight,
    float* __restrict__ out, float* __restrict__ nout) {
  // per (frame, bone) M row-major, then P - g; per bone g_c = G[pivot(c)]
  __shared__ __attribute__((aligned(16))) float maps[SKIN_FRAMES * SKIN_MAX_JOINTS * 12];
  __shared__ float pivots[SKIN_MAX_JOINTS * 3];
  const int b = blockIdx.z, t_base = blockIdx.y * SKIN_FRAMES, tid = threadIdx.x;
  const int v = blockIdx.x * SKIN_THREADS + tid;
  int n = len ? len[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const int frames = min(SKIN_FRAMES, T - t_base);   // frames of this tile
  const int live = max(0, min(frames, n - t_base));  // of which below the length
  const float* g = bind + b * bind_stride;
  if (tid < J * 3) pivots[tid] = g[pivot_of(arg, tid / 3) * 3 + tid % 3];
  for (int i = tid; i < live * J; i += SKIN_THREADS) {
    const int f = i / J, c = i - f * J, p = pivot_of(arg, c);
    const int64_t bt = (int64_t)b * T + t_base + f;
    const float* r = rot + (bt * J + c) * 9;
    const float* x = joints + (bt * J + p) * 3;
    float* m = maps + (f * SKIN_MAX_JOINTS + c) * 12;
    if (bind_rot) {  // M = R Q^T
      const float* q = bind_rot + c * 9;
      for (int a = 0; a < 3; ++a)
        for (int e = 0; e < 3; ++e) m[3 * a + e] = r[3 * a] * q[3 * e] + r[3 * a + 1] * q[3 * e + 1] + r[3 * a + 2] * q[3 * e + 2];
    } else {
      for (int e = 0; e < 9; ++e) m[e] = r[e];
    }
    for (int e = 0; e < 3; ++e) m[9 + e] = x[e] - g[p * 3 + e];
  }
  float x[3] = {0.f, 0.f, 0.f}, nr[3] = {0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
  int idx[4] = {0, 0, 0, 0};
  if (v < V) {
    const float* vp = verts + b * vert_stride + (int64_t)v * 3;
    x[0] = vp[0], x[1] = vp[1], x[2] = vp[2];
    if (NORMALS) {
      const float* np = norms + b * vert_stride + (int64_t)v * 3;
      nr[0] = np[0], nr[1] = np[1], nr[2] = np[2];
    }
    for (int k = 0; k < 4; ++k) {
      w[k] = weight[(int64_t)v * 4 + k];
      const int c = bone[(int64_t)v * 4 + k];
      idx[k] = w[k] != 0.f ? min(max(c, 0), J - 1) : 0;
    }
  }
  __syncthreads();
  if (v >= V) return;
  float y[4][3];
  for (int k = 0; k < 4; ++k)
    for (int e = 0; e < 3; ++e) y[k][e] = x[e] - pivots[idx[k] * 3 + e];
  const int64_t o = (((int64_t)b * T + t_base) * V + v) * 3, step = (int64_t)V * 3;
  for (int f = 0; f < frames; ++f) {
    float d[3] = {0.f, 0.f, 0.f}, s[3] = {0.f, 0.f, 0.f};
    if (f < live) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (w[k] == 0.f) continue;
        const float* m = maps + (f * SKIN_MAX_JOINTS + idx[k]) * 12;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float my = m[3 * a] * y[k][0] + m[3 * a + 1] * y[k][1] + m[3 * a + 2] * y[k][2];
          d[a] += w[k] * (m[9 + a] + (my - y[k][a]));
          if (NORMALS) s[a] += w[k] * (m[3 * a] * nr[0] + m[3 * a + 1] * nr[1] + m[3 * a + 2] * nr[2]);
        }
      }
      d[0] += x[0], d[1] += x[1], d[2] += x[2];
      if (NORMALS) {
        const float l = sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
        if (l > 0.f) s[0] /= l, s[1] /= l, s[2] /= l;  // a zero sum stays zero
      }
    }
    float* po = out + o + f * step;
    po[0] = d[0], po[1] = d[1], po[2] = d[2];
    if (NORMALS) {
      float* pn = nout + o + f * step;
      pn[0] = s[0], pn[1] = s[1], pn[2] = s[2];
    }
  }
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_skin_vertices(const float* joints, const float* rotations, const int32_t* length, int32_t B, int32_t T, int32_t J,
                      const int32_t* parent, const float* vertices, const float* normals, int32_t V, int32_t vertices_per_sample,
                      const float* bind_joints, int32_t bind_per_sample, const float* bind_rotations, const int32_t* bone_index,
                      const float* bone_weight, float* vertices_out, float* normals_out, void* stream) {
  if (!joints || !rotations || !parent || !vertices || !bind_joints || !bone_index || !bone_weight || !vertices_out)
    return MDM_ERR_ARG;
  if (B < 0 || T < 1 || J < 1 || V < 1 || (normals_out && !normals)) return MDM_ERR_ARG;
  if (J > mdm::SKIN_MAX_JOINTS) return MDM_ERR_UNSUPPORTED;
  mdm::SkinArg arg;
  for (int c = 0; c < mdm::SKIN_MAX_JOINTS; ++c) {
    if (c >= 1 && c < J && (parent[c] < 0 || parent[c] >= J || parent[c] == c)) return MDM_ERR_ARG;
    arg.pivot[c] = c >= 1 && c < J ? parent[c] : 0;
  }
  if (B == 0) return MDM_OK;
  const int64_t tiles_v = ((int64_t)V + mdm::SKIN_THREADS - 1) / mdm::SKIN_THREADS;
  const int64_t tiles_t = ((int64_t)T + mdm::SKIN_FRAMES - 1) / mdm::SKIN_FRAMES;
  if (tiles_t > 65535 || B > 65535) return MDM_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)tiles_v, (unsigned)tiles_t, (unsigned)B);
  const int64_t vs = vertices_per_sample ? (int64_t)V * 3 : 0, bs = bind_per_sample ? (int64_t)J * 3 : 0;
#define MDM_SKIN_LAUNCH(N)                                                                                                  \
  hipLaunchKernelGGL((mdm::skin_vertices_kernel<N>), grid, dim3(mdm::SKIN_THREADS), 0, (hipStream_t)stream, joints, rotations, \
                     length, arg, T, J, vertices, normals, V, vs, bind_joints, bs, bind_rotations, bone_index, bone_weight,   \
                     vertices_out, normals_out)
  if (normals_out)
    MDM_SKIN_LAUNCH(true);
  else
    MDM_SKIN_LAUNCH(false);
#undef MDM_SKIN_LAUNCH
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
