// Characters sampled together: on every step, the current clean-motion estimate of every row of a batch is
// turned into the capsule tracks its partners avoid and the contact targets its partners reach for, in front of the
// unchanged guidance kernels of §25.  Several launches behind one entry, because every row's world joints must be complete
// before any row's records are built (five launches with contacts):
//   1. the joints: partner_denorm_kernel writes x0 * std + mean of the steerable columns with the row's own mean / std (two
//      roundings, as torch's `x0 * std + mean`), motion_post.hip's kernel with a one-tap filter recovers P from them, so that
//      P is postprocess.recover_from_ric's bit for bit (the same machine code: the compiler contracts a restated copy of
//      that kernel differently), and partner_world_kernel turns it in place into W = R_y(yaw) P + (x, 0, z) as `to_world`
//      computes it in fp32 (two products, two sums, not fused).
//   2. partner_records_kernel: one wave per (row, frame), a lane a record.  Lanes under Ks read the row's static record,
//      lanes in [Ks, Km) build the keep-out capsule of one bone of one partner in the row's own frame and store it as three
//      16-byte vectors (twelve zero floats for an empty slot or a frame past either length); the frame's ball is a wave
//      reduction over all Km lanes in a fixed order, so the result is the same bits run after run.
//   3. partner_contacts_kernel: one thread per (contact, frame): the meeting point in the world, written into both
//      characters' targets in their own frames.
// Records and targets are data: nothing here is differentiated.  No atomics, no allocation, stream-ordered.
#include "joint_control.h"
#include "kernels.h"

#include <cmath>
#include <cstring>

namespace mdm {
namespace {

constexpr int WORLD_THREADS = 256, CONTACT_THREADS = 256;
constexpr float BOUND_REL = 1e-3f, BOUND_ABS = 1e-3f;  // motion_scene.track_bounds' inflation of the ball

struct Bones {
  int16_t u[MDM_SCENE_MAX_TRACKS], v[MDM_SCENE_MAX_TRACKS];
};

__device__ __forceinline__ int clamp_len(const int* len, int b, int T) {
  const int n = len[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

// p in the world of a character placed at pl = (x, z, cos yaw, sin yaw): to_world's operations in fp32
__device__ __forceinline__ void to_world(const float4 pl, float x, float y, float z, float& ox, float& oy, float& oz) {
#pragma clang fp contract(off)
  const float cx = pl.z * x, sz = pl.w * z, sx = -pl.w * x, cz = pl.z * z;
  ox = (cx + sz) + pl.x;
  oy = y + 0.f;
  oz = (sx + cz) + pl.y;
}

// the inverse: R_y(-yaw) (w - (x, 0, z))
__device__ __forceinline__ void to_local(const float4 pl, float x, float y, float z, float& ox, float& oy, float& oz) {
#pragma clang fp contract(off)
  const float dx = x - pl.x, dz = z - pl.y;
  const float cx = pl.z * dx, sz = -pl.w * dz, sx = pl.w * dx, cz = pl.z * dz;
  ox = cx + sz;
  oy = y;
  oz = sx + cz;
}

// x0 * std + mean of the steerable columns, as two roundings: what `x0 * std + mean` is in torch.  Rows of D = 3 J + 1 floats;
// the first 2 D threads also write the zeros and ones that stand for mean and std in the recovery behind it.
__global__ __launch_bounds__(WORLD_THREADS) void partner_denorm_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                       const float* __restrict__ sd, int64_t n, int T, int feats,
                                                                       int D, float* __restrict__ out, float* __restrict__ unit) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * WORLD_THREADS + threadIdx.x;
  if (i < 2 * D) unit[i] = i < D ? 0.f : 1.f;
  if (i >= n) return;
  const int64_t row = i / D;
  const int c = (int)(i - row * D);
  const int64_t b = row / T;
  const float scaled = x[row * feats + c] * sd[b * feats + c];
  out[i] = scaled + mean[b * feats + c];
}

// in place: the joints of recover_from_ric, zero at and past the row's length, into the world
__global__ __launch_bounds__(WORLD_THREADS) void partner_world_kernel(const int* __restrict__ len, const float4* __restrict__ place,
                                                                      int64_t n, int T, int J, float* __restrict__ world) {
  const int64_t i = (int64_t)blockIdx.x * WORLD_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t bt = i / J;
  const int b = (int)(bt / T), t = (int)(bt - (int64_t)b * T);
  if (t >= clamp_len(len, b, T)) return;
  float* o = world + i * 3;
  float wx, wy, wz;
  to_world(place[b], o[0], o[1], o[2], wx, wy, wz);
  o[0] = wx, o[1] = wy, o[2] = wz;
}

__global__ __launch_bounds__(64) void partner_records_kernel(const float* __restrict__ world, const int* __restrict__ len,
                                                             const float4* __restrict__ place, const int* __restrict__ prow,
                                                             int Pm, Bones bones, int nb, float radius, float margin,
                                                             float weight, int Ks, int Km, int T, int J,
                                                             float4* __restrict__ tracks, float4* __restrict__ bounds) {
  const int bt = blockIdx.x, b = bt / T, t = bt - b * T, k = threadIdx.x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 r0 = zero, r1 = zero, r2 = zero;
  float4* rec = tracks + ((int64_t)bt * Km + k) * 3;
  if (k < Ks) {
    r0 = rec[0], r1 = rec[1], r2 = rec[2];
  } else if (k < Km) {
    const int q = (k - Ks) / nb, i = (k - Ks) - q * nb;
    const int p = prow[b * Pm + q];
    if (p >= 0 && t < clamp_len(len, b, T) && t < clamp_len(len, p, T)) {
      const float4 pl = place[b];
      const float* wa = world + (((int64_t)p * T + t) * J + bones.u[i]) * 3;
      const float* wv = world + (((int64_t)p * T + t) * J + bones.v[i]) * 3;
      float ax, ay, az, bx, by, bz;
      to_local(pl, wa[0], wa[1], wa[2], ax, ay, az);
      to_local(pl, wv[0], wv[1], wv[2], bx, by, bz);
      r0 = make_float4((float)MDM_SCENE_CAPSULE, 1.f, weight, margin);
      r1 = make_float4(ax, ay, az, bx);
      r2 = make_float4(by, bz, radius, 0.f);
    }
    rec[0] = r0, rec[1] = r1, rec[2] = r2;
  }
  // the frame's ball, motion_scene.track_bounds in fp32: centre = mean of the live records' centres, radius = the largest
  // centre distance plus reach plus max(margin, 0), inflated; lanes at or past Km hold kind 0
  const int kind = (int)r0.x;
  const bool live = r0.x != 0.f && r0.z > 0.f;
  const bool cap = kind == MDM_SCENE_CAPSULE;
  const float cx = cap ? 0.5f * (r1.x + r1.w) : r1.x, cy = cap ? 0.5f * (r1.y + r2.x) : r1.y,
              cz = cap ? 0.5f * (r1.z + r2.y) : r1.z;
  float reach;
  if (kind == MDM_SCENE_SPHERE) {
    reach = r1.w;
  } else if (cap) {
    const float ex = r1.w - r1.x, ey = r2.x - r1.y, ez = r2.y - r1.z;
    reach = 0.5f * sqrtf(ex * ex + ey * ey + ez * ez) + r2.z;
  } else {
    reach = sqrtf(r1.w * r1.w + r2.x * r2.x + r2.y * r2.y);
  }
  reach += fmaxf(r0.w, 0.f);
  const float count = wave_sum(live ? 1.f : 0.f);
  const float inv = 1.f / fmaxf(count, 1.f);
  const float mx = wave_sum(live ? cx : 0.f) * inv, my = wave_sum(live ? cy : 0.f) * inv, mz = wave_sum(live ? cz : 0.f) * inv;
  const float dx = cx - mx, dy = cy - my, dz = cz - mz;
  const float far = wave_max(live ? sqrtf(dx * dx + dy * dy + dz * dz) + reach : 0.f);
  const float open = wave_max(live && (kind == MDM_SCENE_HALF_SPACE || r0.y < 0.f) ? 1.f : 0.f);
  if (k == 0) {
    float R = far * (1.f + BOUND_REL) + BOUND_ABS;
    R = open > 0.f ? INFINITY : (count > 0.f ? R : -INFINITY);
    bounds[bt] = count > 0.f ? make_float4(mx, my, mz, R) : make_float4(0.f, 0.f, 0.f, R);
  }
}

// a contact: rows a, b, joints, frames [first, last) and the share `meet` of the way from a's joint to b's
struct Contact {
  int a, ja, b, jb, first, last;
  float meet;
  int pad;
};

__global__ __launch_bounds__(CONTACT_THREADS) void partner_contacts_kernel(const float* __restrict__ world,
                                                                           const int* __restrict__ len,
                                                                           const float4* __restrict__ place,
                                                                           const Contact* __restrict__ contacts, int Nc, int T,
                                                                           int J, float* __restrict__ targets) {
  const int i = blockIdx.x * CONTACT_THREADS + threadIdx.x;
  if (i >= Nc * T) return;
  const int c = i / T, t = i - c * T;
  const Contact ct = contacts[c];
  if (t < ct.first || t >= ct.last || t >= clamp_len(len, ct.a, T) || t >= clamp_len(len, ct.b, T)) return;
  const int64_t ia = (((int64_t)ct.a * T + t) * J + ct.ja) * 3, ib = (((int64_t)ct.b * T + t) * J + ct.jb) * 3;
  const float mx = world[ia] + ct.meet * (world[ib] - world[ia]);
  const float my = world[ia + 1] + ct.meet * (world[ib + 1] - world[ia + 1]);
  const float mz = world[ia + 2] + ct.meet * (world[ib + 2] - world[ia + 2]);
  float ox, oy, oz;
  to_local(place[ct.a], mx, my, mz, ox, oy, oz);
  targets[ia] = ox, targets[ia + 1] = oy, targets[ia + 2] = oz;
  to_local(place[ct.b], mx, my, mz, ox, oy, oz);
  targets[ib] = ox, targets[ib + 1] = oy, targets[ib + 2] = oz;
}

}  // namespace

int64_t step_joints_scratch_floats(int64_t B, int64_t T, int64_t J) {
  const int64_t D = 3 * J + 1;
  return B * T * (D + 3 * J) + 2 * D;
}

// launches 1 and 2 of the head comment: the joints of this step's x0, as postprocess.recover_from_ric gives them
int step_joints(const float* x0, const int* len, const float* mean, const float* sd, int B, int T, int feats, int J, float* scratch,
                float* joints, hipStream_t s) {
  const int D = 3 * J + 1;
  const int64_t nd = (int64_t)B * T * D, nj = (int64_t)B * T * J;
  float* rows = scratch;       // (B, T, D) de-normalised steerable columns
  float* raw = rows + nd;      // (B, T, J, 3): the recovery's unfiltered copy
  float* unit = raw + nj * 3;  // D zeros, D ones
  hipLaunchKernelGGL(partner_denorm_kernel, dim3((unsigned)(((nd > 2 * D ? nd : 2 * D) + WORLD_THREADS - 1) / WORLD_THREADS)),
                     dim3(WORLD_THREADS), 0, s, x0, mean, sd, nd, T, feats, D, rows, unit);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return motion_post(rows, len, unit, unit + D, B, T, D, J, 0, nullptr, raw, joints, s);
}

}  // namespace mdm

extern "C" int mdm_partner_tracks_max_frames(void) { return 64 * 1024 / (5 * (int)sizeof(float)); }

extern "C" int64_t mdm_partner_tracks_scratch_floats(int32_t B, int32_t T, int32_t F) {
  const int64_t J = mdm::control::control_joints(F);
  if (B < 0 || T < 0 || J == 0) return 0;
  return mdm::step_joints_scratch_floats(B, T, J);
}

extern "C" int mdm_partner_tracks(const float* x0, const int32_t* length, const float* mean, const float* std,
                                  const float* placements, const int32_t* partner_rows, const int32_t* partner_rows_host,
                                  int32_t Pm, const int32_t* bones, int32_t nb, float radius, float margin, float weight,
                                  int32_t Ks, int32_t Km, const int32_t* contacts, const int32_t* contacts_host, int32_t Nc,
                                  int32_t B, int32_t T, int32_t F, float* world, float* scratch, float* tracks,
                                  float* track_bounds, float* targets, void* stream) {
  if (!x0 || !length || !mean || !std || !placements || !world || !scratch || B < 0 || T < 0) return MDM_ERR_ARG;
  if (Km < 0 || Km > MDM_SCENE_MAX_TRACKS || Ks < 0 || Pm < 0 || nb < 0 || Nc < 0) return MDM_ERR_ARG;
  if ((int64_t)Ks + (int64_t)Pm * nb != Km) return MDM_ERR_ARG;
  const int J = mdm::control::control_joints(F);
  if (J == 0) return MDM_ERR_ARG;
  if ((uintptr_t)placements & 15) return MDM_ERR_ARG;
  if (Km > 0 && (!tracks || !track_bounds || ((uintptr_t)tracks & 15) || ((uintptr_t)track_bounds & 15))) return MDM_ERR_ARG;
  if (Pm * nb > 0 && (!partner_rows || !partner_rows_host || !bones)) return MDM_ERR_ARG;
  if (Nc > 0 && (!contacts || !contacts_host || !targets)) return MDM_ERR_ARG;
  if (!(std::isfinite(radius) && radius > 0.f) || !std::isfinite(margin) || !(std::isfinite(weight) && weight >= 0.f))
    return MDM_ERR_ARG;
  if (B == 0 || T == 0) return MDM_OK;
  mdm::Bones bn = {};
  if (Pm * nb > 0) {
    for (int i = 0; i < nb; ++i) {
      const int u = bones[2 * i], v = bones[2 * i + 1];
      if (u < 0 || u >= J || v < 0 || v >= J) return MDM_ERR_ARG;
      bn.u[i] = (int16_t)u, bn.v[i] = (int16_t)v;
    }
    for (int64_t i = 0; i < (int64_t)B * Pm; ++i) {
      const int p = partner_rows_host[i];
      if (p < -1 || p >= B || p == (int)(i / Pm)) return MDM_ERR_ARG;
    }
  }
  for (int c = 0; c < Nc; ++c) {
    const int32_t* q = contacts_host + 8 * (int64_t)c;
    float meet;
    memcpy(&meet, q + 6, sizeof meet);
    if (q[0] < 0 || q[0] >= B || q[2] < 0 || q[2] >= B || q[1] < 0 || q[1] >= J || q[3] < 0 || q[3] >= J || q[4] > q[5] ||
        !(meet >= 0.f && meet <= 1.f))
      return MDM_ERR_ARG;
  }
  if (T > mdm_partner_tracks_max_frames()) return MDM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const float4* place = (const float4*)placements;
  const int64_t nj = (int64_t)B * T * J;
  const int st = mdm::step_joints(x0, length, mean, std, B, T, F, J, scratch, world, s);
  if (st != MDM_OK) return st;
  hipLaunchKernelGGL(mdm::partner_world_kernel, dim3((unsigned)((nj + mdm::WORLD_THREADS - 1) / mdm::WORLD_THREADS)),
                     dim3(mdm::WORLD_THREADS), 0, s, length, place, nj, T, J, world);
  MDM_RETURN_IF_LAUNCH_FAILED();
  if (Km > 0) {
    hipLaunchKernelGGL(mdm::partner_records_kernel, dim3((unsigned)((int64_t)B * T)), dim3(64), 0, s, world, length, place,
                       partner_rows, Pm, bn, nb > 0 ? nb : 1, radius, margin, weight, Ks, Km, T, J, (float4*)tracks,
                       (float4*)track_bounds);
    MDM_RETURN_IF_LAUNCH_FAILED();
  }
  if (Nc > 0) {
    const int64_t blocks = ((int64_t)Nc * T + mdm::CONTACT_THREADS - 1) / mdm::CONTACT_THREADS;
    hipLaunchKernelGGL(mdm::partner_contacts_kernel, dim3((unsigned)blocks), dim3(mdm::CONTACT_THREADS), 0, s, world, length,
                       place, (const mdm::Contact*)contacts, Nc, T, J, targets);
    MDM_RETURN_IF_LAUNCH_FAILED();
  }
  return MDM_OK;
}
