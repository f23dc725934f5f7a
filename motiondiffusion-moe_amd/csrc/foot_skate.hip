// Foot-skate clean-up on the device: pin planted feet with two-bone leg IK.  (T, J, 3) joints and four
// foot-contact labels per frame -> (T, J, 3) joints whose ankles stand still while their label is on, optionally the
// (T, J, 3, 3) global rotations turned with the bones, and the slide of each foot joint before and after.
//   labels: given values against four thresholds (a (T, 4) tensor, or the contact columns of normalised rows in place),
//           or detected as foot_detect has them (utils/motion_process.py:39-62): squared displacement to the next frame
//           under feet_thre, the last frame repeating the one before
//   runs:   a maximal interval of frames with the label on; its anchor is the mean (X, Z) of the joint over the run (summed in
//           double in frame order, rounded once); inside the run delta = anchor - p_xz, heights never change
//   blend:  up to `blend` frames either side of a run the neighbouring run's delta fades out by 1 - smoothstep
//   ankle:  two-bone IK with the hip fixed and the knee kept in its own bend plane; toe: aimed at its own target from the
//           new ankle on its own bone length (aimed, not pinned)
//   rotations: R' = Q R for knee, ankle and toe, Q the shortest arc from the old bone to the new one
// A (frame, leg) with no run and no blend weight on its ankle and toe is copied bit for bit, and so is every other joint.
// One workgroup per sample.  The labels (one byte a frame) and which (frame, foot) entries carry a delta live in LDS, the
// deltas in a caller's scratch (T, 4, 2) written and read by this workgroup only, barriers between the phases.  Runs are
// found by the thread whose frame starts one; it walks the run, so the double sum is in frame order whatever the thread or
// wave order.  Per-frame work is one thread per (frame, foot) or (frame, leg).  fp32 in the order of DESIGN.md §18 with
// contraction off, IEEE divide and square root.  Latency of one workgroup; tiny.
#pragma clang fp contract(off)
#include "kernels.h"

namespace mdm {
namespace {

constexpr int FS_THREADS = 256;
constexpr int FS_MAX_FRAMES = 4096;  // 5 bytes of LDS per frame: 20 KiB

struct FsArg {
  int J;
  int feet[4];
  int leg[2][4];  // hip, knee, ankle, toe
  float thre[4];
};

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* p, V3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 unit(V3 a, float n) { return {__fdiv_rn(a.x, n), __fdiv_rn(a.y, n), __fdiv_rn(a.z, n)}; }
// e - (e . u) u
__device__ __forceinline__ V3 reject(V3 e, V3 u) {
  const float p = dot(e, u);
  return {e.x - p * u.x, e.y - p * u.y, e.z - p * u.z};
}
__device__ __forceinline__ bool same_bits(V3 a, V3 b) {
  return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) &&
         __float_as_uint(a.z) == __float_as_uint(b.z);
}
// 1 - smoothstep(k / (blend + 1))
__device__ __forceinline__ float fade(int k, int blend) {
  const float x = __fdiv_rn((float)k, (float)(blend + 1));
  const float x2 = x * x;
  return 1.f - (3.f * x2 - 2.f * (x2 * x));
}

// R' = Q R with Q the shortest arc from bone `from` to bone `to`: Q = I + [v]x + [v]x^2 / (1 + cos), v = x cross y
__device__ __forceinline__ void turn_rotation(const float* Rin, float* Rout, V3 from, V3 to) {
  if (same_bits(from, to)) {
    for (int i = 0; i < 9; ++i) Rout[i] = Rin[i];
    return;
  }
  const V3 x = unit(from, __fsqrt_rn(dot(from, from))), y = unit(to, __fsqrt_rn(dot(to, to)));
  const V3 v = cross(x, y);
  const float s = 1.f + dot(x, y);
  float K[3][3] = {{0.f, -v.z, v.y}, {v.z, 0.f, -v.x}, {-v.y, v.x, 0.f}}, Q[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      Q[r][c] = ((r == c ? 1.f : 0.f) + K[r][c]) + __fdiv_rn(K[r][0] * K[0][c] + K[r][1] * K[1][c] + K[r][2] * K[2][c], s);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Rout[3 * r + c] = Q[r][0] * Rin[c] + Q[r][1] * Rin[3 + c] + Q[r][2] * Rin[6 + c];
}

__global__ __launch_bounds__(FS_THREADS) void foot_skate_kernel(
    const float* __restrict__ joints, const int* __restrict__ len, const FsArg sk, const float* __restrict__ contact,
    int64_t cstride, double feet_thre, int blend, int T, const float* __restrict__ rot_in, float* out, float* rot_out,
    float* __restrict__ slide, int* __restrict__ pairs, float* delta) {
  __shared__ unsigned char lab[FS_MAX_FRAMES];      // bit f: foot f's label
  __shared__ unsigned char act[FS_MAX_FRAMES * 4];  // (frame, foot) carries a delta: in a run, or within `blend` of one
  const int J = sk.J, W = 3 * J;
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = len ? len[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const float* src = joints + (int64_t)b * T * W;
  float* ob = out + (int64_t)b * T * W;
  float* dl = delta + (int64_t)b * T * 8;
  const float* rin = rot_in ? rot_in + (int64_t)b * T * J * 9 : nullptr;
  float* rob = rot_in ? rot_out + (int64_t)b * T * J * 9 : nullptr;

  // labels; everything is copied, the legs are overwritten below; frames past the length are zero and never read
  for (int t = tid; t < n; t += FS_THREADS) {
    unsigned bits = 0;
    if (contact) {
      const float* c = contact + ((int64_t)b * T + t) * cstride;
      for (int f = 0; f < 4; ++f) bits |= (c[f] > sk.thre[f] ? 1u : 0u) << f;
    } else if (n > 1) {
      const int t0 = t < n - 1 ? t : n - 2;  // the last frame repeats the one before
      for (int f = 0; f < 4; ++f) {
        const float* f0 = src + (int64_t)t0 * W + 3 * sk.feet[f];
        const float* f1 = f0 + W;
        const float dx = f1[0] - f0[0], dy = f1[1] - f0[1], dz = f1[2] - f0[2];
        bits |= ((double)(dx * dx + dy * dy + dz * dz) < feet_thre ? 1u : 0u) << f;
      }
    }
    lab[t] = (unsigned char)bits;
  }
  for (int i = tid; i < T * W; i += FS_THREADS) ob[i] = i < n * W ? src[i] : 0.f;
  if (rob)
    for (int i = tid; i < T * J * 9; i += FS_THREADS) rob[i] = i < n * J * 9 ? rin[i] : 0.f;
  __syncthreads();

  // runs: the thread of a run's first frame takes the anchor and the run's deltas
  for (int i = tid; i < n * 4; i += FS_THREADS) {
    const int t = i >> 2, f = i & 3;
    const bool on = (lab[t] >> f) & 1;
    act[i] = on;
    if (!on || (t > 0 && ((lab[t - 1] >> f) & 1))) continue;
    const float* p = src + 3 * sk.feet[f];
    double sx = 0.0, sz = 0.0;
    int e = t;
    for (; e < n && ((lab[e] >> f) & 1); ++e) sx += (double)p[(int64_t)e * W], sz += (double)p[(int64_t)e * W + 2];
    const float ax = (float)(sx / (double)(e - t)), az = (float)(sz / (double)(e - t));
    for (int k = t; k < e; ++k) dl[8 * k + 2 * f] = ax - p[(int64_t)k * W], dl[8 * k + 2 * f + 1] = az - p[(int64_t)k * W + 2];
  }
  __syncthreads();

  // blend: outside the runs, the nearest contact frame of either side within `blend` frames
  for (int i = tid; i < n * 4; i += FS_THREADS) {
    const int t = i >> 2, f = i & 3;
    if ((lab[t] >> f) & 1) continue;
    int kl = 0, kr = 0;
    for (int k = 1; k <= blend && t - k >= 0 && !kl; ++k)
      if ((lab[t - k] >> f) & 1) kl = k;
    for (int k = 1; k <= blend && t + k < n && !kr; ++k)
      if ((lab[t + k] >> f) & 1) kr = k;
    float wl = 0.f, wr = 0.f, lx = 0.f, lz = 0.f, rx = 0.f, rz = 0.f;
    if (kl) wl = fade(kl, blend), lx = dl[8 * (t - kl) + 2 * f], lz = dl[8 * (t - kl) + 2 * f + 1];
    if (kr) wr = fade(kr, blend), rx = dl[8 * (t + kr) + 2 * f], rz = dl[8 * (t + kr) + 2 * f + 1];
    const float den = fmaxf(1.f, wl + wr);
    dl[8 * t + 2 * f] = __fdiv_rn(wl * lx + wr * rx, den), dl[8 * t + 2 * f + 1] = __fdiv_rn(wl * lz + wr * rz, den);
    act[i] = (kl | kr) != 0;
  }
  __syncthreads();

  // legs: two-bone IK to the ankle's target with the hip fixed, the toe aimed at its own
  for (int i = tid; i < n * 2; i += FS_THREADS) {
    const int t = i >> 1, leg = i & 1;
    if (!(act[4 * t + 2 * leg] | act[4 * t + 2 * leg + 1])) continue;
    const int jh = sk.leg[leg][0], jk = sk.leg[leg][1], ja = sk.leg[leg][2], jt = sk.leg[leg][3];
    const float* fr = src + (int64_t)t * W;
    const V3 h = ld3(fr + 3 * jh), k = ld3(fr + 3 * jk), a = ld3(fr + 3 * ja), toe = ld3(fr + 3 * jt);
    const float* d4 = dl + 8 * t + 4 * leg;
    const float dax = act[4 * t + 2 * leg] ? d4[0] : 0.f, daz = act[4 * t + 2 * leg] ? d4[1] : 0.f;
    const float dtx = act[4 * t + 2 * leg + 1] ? d4[2] : 0.f, dtz = act[4 * t + 2 * leg + 1] ? d4[3] : 0.f;
    const V3 kh = sub(k, h), ak = sub(a, k);
    const float l1 = __fsqrt_rn(dot(kh, kh)), l2 = __fsqrt_rn(dot(ak, ak));
    const V3 d = sub(V3{a.x + dax, a.y, a.z + daz}, h);
    const float nd = __fsqrt_rn(dot(d, d));
    const V3 u = unit(d, nd);
    const float lo = fabsf(l1 - l2) * (1.f + 1e-4f) + 1e-6f, hi = (l1 + l2) * (1.f - 1e-4f);
    const float dist = fminf(fmaxf(nd, lo), hi);
    const float bound = 1e-10f * (l1 * l1);
    V3 w = reject(kh, u);
    float w2 = dot(w, w);
    if (w2 < bound) w = reject(V3{0.f, 0.f, 1.f}, u), w2 = dot(w, w);
    if (w2 < bound) w = reject(V3{1.f, 0.f, 0.f}, u), w2 = dot(w, w);
    w = unit(w, __fsqrt_rn(w2));
    float ca = __fdiv_rn((l1 * l1 + dist * dist) - l2 * l2, (2.f * l1) * dist);
    ca = fminf(fmaxf(ca, -1.f), 1.f);
    const float sa = __fsqrt_rn(1.f - ca * ca);
    const V3 k2 = {h.x + l1 * (ca * u.x + sa * w.x), h.y + l1 * (ca * u.y + sa * w.y), h.z + l1 * (ca * u.z + sa * w.z)};
    const V3 a2 = {h.x + dist * u.x, h.y + dist * u.y, h.z + dist * u.z};
    const V3 ta = sub(toe, a);
    const float l3 = __fsqrt_rn(dot(ta, ta));
    const V3 v = sub(V3{toe.x + dtx, toe.y, toe.z + dtz}, a2);
    const float v2 = dot(v, v);
    V3 t2;
    if (v2 < 1e-10f * (l3 * l3)) {
      t2 = {a2.x + ta.x, a2.y + ta.y, a2.z + ta.z};
    } else {
      const V3 vu = unit(v, __fsqrt_rn(v2));
      t2 = {a2.x + l3 * vu.x, a2.y + l3 * vu.y, a2.z + l3 * vu.z};
    }
    float* o = ob + (int64_t)t * W;
    st3(o + 3 * jk, k2), st3(o + 3 * ja, a2), st3(o + 3 * jt, t2);
    if (rob) {
      const float* ri = rin + (int64_t)t * J * 9;
      float* ro = rob + (int64_t)t * J * 9;
      turn_rotation(ri + 9 * jk, ro + 9 * jk, kh, sub(k2, h));
      turn_rotation(ri + 9 * ja, ro + 9 * ja, ak, sub(a2, k2));
      turn_rotation(ri + 9 * jt, ro + 9 * jt, ta, sub(t2, a2));
    }
  }
  if (!slide && !pairs) return;
  __syncthreads();

  // slide: mean XZ step of a foot joint over the pairs of neighbouring contact frames, before (0..3) and after (4..7)
  if (tid < 8) {
    const int f = tid & 3;
    const float* p = (tid < 4 ? src : ob) + 3 * sk.feet[f];
    double acc = 0.0;
    int cnt = 0;
    for (int t = 0; t + 1 < n; ++t) {
      if (!((lab[t] >> f) & 1) || !((lab[t + 1] >> f) & 1)) continue;
      const float dx = p[(int64_t)(t + 1) * W] - p[(int64_t)t * W], dz = p[(int64_t)(t + 1) * W + 2] - p[(int64_t)t * W + 2];
      acc += (double)__fsqrt_rn(dx * dx + dz * dz);
      ++cnt;
    }
    if (slide) slide[(int64_t)b * 8 + tid] = cnt ? (float)(acc / (double)cnt) : 0.f;
    if (pairs && tid < 4) pairs[(int64_t)b * 4 + f] = cnt;
  }
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_foot_skate_max_frames(void) { return mdm::FS_MAX_FRAMES; }

int mdm_foot_skate(const float* joints, const int32_t* length, const MdmSkeleton* skeleton, const float* contact,
                   int64_t contact_stride, const float* contact_thre, double feet_thre, int32_t blend, int32_t B, int32_t T,
                   const float* rotations_in, float* joints_out, float* rotations_out, float* slide_out, int32_t* pairs_out,
                   float* scratch, void* stream) {
  if (!joints || !skeleton || !joints_out || !scratch || B < 0 || T < 1 || blend < 0) return MDM_ERR_ARG;
  if (contact ? (!contact_thre || contact_stride < 4) : !(feet_thre >= 0.0)) return MDM_ERR_ARG;
  if ((rotations_in == nullptr) != (rotations_out == nullptr)) return MDM_ERR_ARG;
  if (joints_out == joints || (rotations_in && rotations_out == rotations_in)) return MDM_ERR_ARG;  // never in place
  int parent[MDM_SKEL_MAX_JOINTS];
  if (!mdm::skeleton_ok(*skeleton, parent)) return MDM_ERR_ARG;
  mdm::FsArg sk;
  sk.J = skeleton->joints;
  // a leg: the last four entries hip, knee, ankle, toe of the chain that ends in the toe joint
  for (int leg = 0; leg < 2; ++leg) {
    const int ankle = skeleton->feet[2 * leg], toe = skeleton->feet[2 * leg + 1];
    bool found = false;
    for (int c = 0; c < skeleton->nchains && !found; ++c) {
      const int lo = skeleton->chain_offsets[c], hi = skeleton->chain_offsets[c + 1];
      if (hi - lo < 4 || skeleton->chain_joints[hi - 1] != toe || skeleton->chain_joints[hi - 2] != ankle) continue;
      for (int k = 0; k < 4; ++k) sk.leg[leg][k] = skeleton->chain_joints[hi - 4 + k];
      found = true;
    }
    if (!found) return MDM_ERR_ARG;
  }
  for (int k = 0; k < 4; ++k)
    if (sk.leg[0][k] == sk.leg[1][k]) return MDM_ERR_ARG;  // two legs, not one twice
  for (int f = 0; f < 4; ++f) sk.feet[f] = skeleton->feet[f], sk.thre[f] = contact ? contact_thre[f] : 0.f;
  if (T > mdm::FS_MAX_FRAMES) return MDM_ERR_UNSUPPORTED;
  if (B == 0) return MDM_OK;
  hipLaunchKernelGGL(mdm::foot_skate_kernel, dim3(B), dim3(mdm::FS_THREADS), 0, (hipStream_t)stream, joints, length, sk, contact,
                     contact_stride, feet_thre, blend, T, rotations_in, joints_out, rotations_out, slide_out, pairs_out,
                     scratch);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
