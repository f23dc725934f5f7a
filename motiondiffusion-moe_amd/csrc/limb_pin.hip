// Exact reach on the device: pin the end joint of two-bone limbs (wrists, ankles) to 3-D targets by limb IK.
// (T, J, 3) joints, (T, J, 3) targets and (T, J, 3) weights -> (T, J, 3) joints whose limb ends lie on their targets where all
// three weights of the end joint are > 0, optionally the (T, J, 3, 3) global rotations turned with the bones, and per limb the
// distance of the end joint to its target before and after.
//   limbs:  up to 8 rows (root, mid, end, tip), tip = -1 where the end joint has no child
//   pins:   frame t < n is a pin frame of a limb iff W[t, end, c] > 0 for c = 0, 1, 2; G is read only there
//   delta:  in a pin frame G[end] - p[end] (3-D); up to `blend` frames outside, the nearest pin frame of either side fades out
//           by 1 - smoothstep, delta = (wL dL + wR dR) / max(1, wL + wR), as §18 blends
//   solve:  §18's two-bone solve with the limb root fixed and the target end + delta: reach clamp, the mid joint kept in its
//           own bend plane, the fallbacks
//   tip:    carried rigidly, tip' = end' + Q2 (tip - end), Q2 the shortest arc of the mid -> end bone
//   rotations: R'[mid] = Q1 R[mid], R'[end] = Q2 R[end], R'[tip] = Q2 R[tip], Q1 the shortest arc of the root -> mid bone
// A (frame, limb) that is neither a pin frame nor within `blend` of one is copied bit for bit, and so is every other joint.
// One workgroup per sample.  LDS: one byte per frame of pin bits (bit l: limb l) and one byte per (frame, limb) that carries
// a delta, 1 + 8 = 9 bytes per frame: 36 KiB.  The deltas live in a caller's scratch (T, L, 3) written and read by this
// workgroup only, barriers between the phases: copy + pin flags + pin deltas (a thread per frame), blend and solve (a thread
// per (frame, limb)), error sums (a thread per limb, double in frame order).  fp32 in the order of DESIGN.md §28 with
// contraction off, IEEE divide and square root.  Latency of one workgroup; tiny.
#pragma clang fp contract(off)
#include "kernels.h"

namespace mdm {
namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_FRAMES = 4096;  // 9 bytes of LDS per frame: 36 KiB
constexpr int LP_MAX_LIMBS = 8;

struct LpArg {
  int J, L;
  int limb[LP_MAX_LIMBS][4];  // root, mid, end, tip (-1: none)
};

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* p, V3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
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

// Q, the shortest arc from bone `from` to bone `to`: Q = I + [v]x + [v]x^2 / (1 + cos), v = x cross y; false (and Q untouched)
// where the bone keeps every bit
__device__ __forceinline__ bool arc(V3 from, V3 to, float Q[3][3]) {
  if (same_bits(from, to)) return false;
  const V3 x = unit(from, __fsqrt_rn(dot(from, from))), y = unit(to, __fsqrt_rn(dot(to, to)));
  const V3 v = cross(x, y);
  const float s = 1.f + dot(x, y);
  const float K[3][3] = {{0.f, -v.z, v.y}, {v.z, 0.f, -v.x}, {-v.y, v.x, 0.f}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      Q[r][c] = ((r == c ? 1.f : 0.f) + K[r][c]) + __fdiv_rn(K[r][0] * K[0][c] + K[r][1] * K[1][c] + K[r][2] * K[2][c], s);
  return true;
}
// R' = Q R, or R where the bone kept every bit
__device__ __forceinline__ void turn(const float* Rin, float* Rout, bool turned, const float Q[3][3]) {
  if (!turned) {
    for (int i = 0; i < 9; ++i) Rout[i] = Rin[i];
    return;
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Rout[3 * r + c] = Q[r][0] * Rin[c] + Q[r][1] * Rin[3 + c] + Q[r][2] * Rin[6 + c];
}

__device__ __forceinline__ float gap(const float* p, const float* g) {
  const float dx = p[0] - g[0], dy = p[1] - g[1], dz = p[2] - g[2];
  return __fsqrt_rn(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(LP_THREADS) void limb_pin_kernel(
    const float* __restrict__ joints, const int* __restrict__ len, const float* __restrict__ targets,
    const float* __restrict__ weights, const LpArg lp, int blend, int T, const float* __restrict__ rot_in, float* out,
    float* rot_out, float* __restrict__ err, int* __restrict__ counts, float* delta) {
  __shared__ unsigned char pin[LP_MAX_FRAMES];                 // bit l: frame is a pin frame of limb l
  __shared__ unsigned char act[LP_MAX_FRAMES * LP_MAX_LIMBS];  // (frame, limb) carries a delta: a pin frame, or within `blend`
  const int J = lp.J, L = lp.L, W = 3 * J;
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = len ? len[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const float* src = joints + (int64_t)b * T * W;
  const float* G = targets + (int64_t)b * T * W;
  const float* Wt = weights + (int64_t)b * T * W;
  float* ob = out + (int64_t)b * T * W;
  float* dl = delta + (int64_t)b * T * L * 3;
  const float* rin = rot_in ? rot_in + (int64_t)b * T * J * 9 : nullptr;
  float* rob = rot_in ? rot_out + (int64_t)b * T * J * 9 : nullptr;

  // pin flags from the weights alone and the pin frames' deltas; everything is copied, the limbs are overwritten below;
  // frames past the length are zero and never read
  for (int t = tid; t < n; t += LP_THREADS) {
    unsigned bits = 0;
    for (int l = 0; l < L; ++l) {
      const int64_t at = (int64_t)t * W + 3 * lp.limb[l][2];
      const bool on = Wt[at] > 0.f && Wt[at + 1] > 0.f && Wt[at + 2] > 0.f;
      act[t * L + l] = on;
      if (!on) continue;
      bits |= 1u << l;
      st3(dl + ((int64_t)t * L + l) * 3, sub(ld3(G + at), ld3(src + at)));
    }
    pin[t] = (unsigned char)bits;
  }
  for (int64_t i = tid; i < (int64_t)T * W; i += LP_THREADS) ob[i] = i < (int64_t)n * W ? src[i] : 0.f;
  if (rob)
    for (int64_t i = tid; i < (int64_t)T * J * 9; i += LP_THREADS) rob[i] = i < (int64_t)n * J * 9 ? rin[i] : 0.f;
  __syncthreads();

  // blend: outside the pin frames, the nearest pin frame of either side within `blend` frames
  for (int i = tid; i < n * L; i += LP_THREADS) {
    const int t = i / L, l = i - t * L;
    if ((pin[t] >> l) & 1) continue;
    int kl = 0, kr = 0;
    for (int k = 1; k <= blend && t - k >= 0 && !kl; ++k)
      if ((pin[t - k] >> l) & 1) kl = k;
    for (int k = 1; k <= blend && t + k < n && !kr; ++k)
      if ((pin[t + k] >> l) & 1) kr = k;
    if (!(kl | kr)) continue;
    float wl = 0.f, wr = 0.f;
    V3 dL = {0.f, 0.f, 0.f}, dR = {0.f, 0.f, 0.f};
    if (kl) wl = fade(kl, blend), dL = ld3(dl + ((int64_t)(t - kl) * L + l) * 3);
    if (kr) wr = fade(kr, blend), dR = ld3(dl + ((int64_t)(t + kr) * L + l) * 3);
    const float den = fmaxf(1.f, wl + wr);
    st3(dl + (int64_t)i * 3, V3{__fdiv_rn(wl * dL.x + wr * dR.x, den), __fdiv_rn(wl * dL.y + wr * dR.y, den),
                                __fdiv_rn(wl * dL.z + wr * dR.z, den)});
    act[i] = 1;
  }
  __syncthreads();

  // limbs: two-bone IK to the end joint's target with the limb root fixed, the tip carried rigidly
  for (int i = tid; i < n * L; i += LP_THREADS) {
    if (!act[i]) continue;
    const int t = i / L, l = i - t * L;
    const int jr = lp.limb[l][0], jm = lp.limb[l][1], je = lp.limb[l][2], jt = lp.limb[l][3];
    const float* fr = src + (int64_t)t * W;
    const V3 h = ld3(fr + 3 * jr), k = ld3(fr + 3 * jm), a = ld3(fr + 3 * je);
    const V3 dd = ld3(dl + (int64_t)i * 3);
    const V3 kh = sub(k, h), ak = sub(a, k);
    const float l1 = __fsqrt_rn(dot(kh, kh)), l2 = __fsqrt_rn(dot(ak, ak));
    const V3 d = sub(add(a, dd), h);
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
    float Q1[3][3], Q2[3][3];
    const bool t2 = arc(ak, sub(a2, k2), Q2);
    float* o = ob + (int64_t)t * W;
    st3(o + 3 * jm, k2), st3(o + 3 * je, a2);
    if (jt >= 0) {
      const V3 ta = sub(ld3(fr + 3 * jt), a);
      const V3 tq = t2 ? V3{Q2[0][0] * ta.x + Q2[0][1] * ta.y + Q2[0][2] * ta.z, Q2[1][0] * ta.x + Q2[1][1] * ta.y + Q2[1][2] * ta.z,
                            Q2[2][0] * ta.x + Q2[2][1] * ta.y + Q2[2][2] * ta.z}
                       : ta;
      st3(o + 3 * jt, add(a2, tq));
    }
    if (rob) {
      const bool t1 = arc(kh, sub(k2, h), Q1);
      const float* ri = rin + (int64_t)t * J * 9;
      float* ro = rob + (int64_t)t * J * 9;
      turn(ri + 9 * jm, ro + 9 * jm, t1, Q1);
      turn(ri + 9 * je, ro + 9 * je, t2, Q2);
      if (jt >= 0) turn(ri + 9 * jt, ro + 9 * jt, t2, Q2);
    }
  }
  if (!err && !counts) return;
  __syncthreads();

  // report: per limb the mean and the maximum distance of the end joint to its target over the pin frames, before (0, 1) and
  // after (2, 3); the pin frames and those of them whose target lay outside the reach clamp
  if (tid < L) {
    const int l = tid, jr = lp.limb[l][0], jm = lp.limb[l][1], je = lp.limb[l][2];
    double acc0 = 0.0, acc1 = 0.0;
    float mx0 = 0.f, mx1 = 0.f;
    int cnt = 0, clamped = 0;
    for (int t = 0; t < n; ++t) {
      if (!((pin[t] >> l) & 1)) continue;
      const int64_t at = (int64_t)t * W;
      const float e0 = gap(src + at + 3 * je, G + at + 3 * je), e1 = gap(ob + at + 3 * je, G + at + 3 * je);
      acc0 += (double)e0, acc1 += (double)e1;
      mx0 = fmaxf(mx0, e0), mx1 = fmaxf(mx1, e1);
      const V3 h = ld3(src + at + 3 * jr), k = ld3(src + at + 3 * jm), a = ld3(src + at + 3 * je);
      const V3 kh = sub(k, h), ak = sub(a, k);
      const float l1 = __fsqrt_rn(dot(kh, kh)), l2 = __fsqrt_rn(dot(ak, ak));
      const V3 d = sub(add(a, ld3(dl + ((int64_t)t * L + l) * 3)), h);
      const float nd = __fsqrt_rn(dot(d, d));
      const float lo = fabsf(l1 - l2) * (1.f + 1e-4f) + 1e-6f, hi = (l1 + l2) * (1.f - 1e-4f);
      clamped += (nd < lo || nd > hi) ? 1 : 0;
      ++cnt;
    }
    if (err) {
      float* e = err + ((int64_t)b * L + l) * 4;
      e[0] = cnt ? (float)(acc0 / (double)cnt) : 0.f, e[1] = mx0;
      e[2] = cnt ? (float)(acc1 / (double)cnt) : 0.f, e[3] = mx1;
    }
    if (counts) counts[((int64_t)b * L + l) * 2] = cnt, counts[((int64_t)b * L + l) * 2 + 1] = clamped;
  }
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_limb_pin_max_frames(void) { return mdm::LP_MAX_FRAMES; }

int mdm_limb_pin(const float* joints, const int32_t* length, const float* targets, const float* weights, const int32_t* limbs,
                 int32_t L, int32_t J, int32_t blend, int32_t B, int32_t T, const float* rotations_in, float* joints_out,
                 float* rotations_out, float* error_out, int32_t* counts_out, float* scratch, void* stream) {
  if (!joints || !targets || !weights || !limbs || !joints_out || !scratch || B < 0 || T < 1 || blend < 0) return MDM_ERR_ARG;
  if (L < 1 || L > mdm::LP_MAX_LIMBS || J < 3 || J > MDM_SKEL_MAX_JOINTS) return MDM_ERR_ARG;
  if ((rotations_in == nullptr) != (rotations_out == nullptr)) return MDM_ERR_ARG;
  if (joints_out == joints || joints_out == targets || joints_out == weights) return MDM_ERR_ARG;  // never in place
  if (rotations_in && rotations_out == rotations_in) return MDM_ERR_ARG;
  mdm::LpArg lp;
  lp.J = J, lp.L = L;
  bool moved[MDM_SKEL_MAX_JOINTS] = {};
  for (int l = 0; l < L; ++l) {
    const int32_t* q = limbs + 4 * l;
    for (int k = 0; k < 4; ++k) {
      if (q[k] >= J || q[k] < (k == 3 ? -1 : 0)) return MDM_ERR_ARG;
      for (int m = 0; m < k; ++m)
        if (q[m] == q[k]) return MDM_ERR_ARG;  // a joint twice within a limb
      lp.limb[l][k] = q[k];
    }
    for (int k = 1; k < 4; ++k) {  // two limbs may share a root, never a joint that one of them moves
      if (q[k] < 0) continue;
      if (moved[q[k]]) return MDM_ERR_ARG;
      moved[q[k]] = true;
    }
  }
  for (int l = 0; l < L; ++l)
    if (moved[limbs[4 * l]]) return MDM_ERR_ARG;  // a root that another limb moves: the result would depend on thread order
  for (int l = L; l < mdm::LP_MAX_LIMBS; ++l)
    for (int k = 0; k < 4; ++k) lp.limb[l][k] = 0;
  if (T > mdm::LP_MAX_FRAMES) return MDM_ERR_UNSUPPORTED;
  if (B == 0) return MDM_OK;
  hipLaunchKernelGGL(mdm::limb_pin_kernel, dim3(B), dim3(mdm::LP_THREADS), 0, (hipStream_t)stream, joints, length, targets,
                     weights, lp, blend, T, rotations_in, joints_out, rotations_out, error_out, counts_out, scratch);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
