// Joint-position control: the weighted squared distance of recover_from_ric(x0 * std + mean) to target
// joint positions, its gradient with respect to the normalised features, and the guidance that moves a step's x0 down it.
//   P = recover_from_ric(x0 * std + mean)    forward exactly as motion_post_kernel (fp64 scans, same operation order)
//   L = sum_{t < len, j, k} W (P - G)^2      dL/dP = 2 W (P - G), zero wherever W == 0 (G is then never read into it)
// Backward, per sample:
//   ric columns   (4 + 3(j-1) ..): rotated by the inverse root rotation of their own frame -> transpose of that rotation
//   root height   (3):             P[t, 0, y] directly
//   root XZ       (1, 2):          P[t, :, x|z] += px|pz[t], px[t] = sum_{s <= t} rot(ang[s]) v[s - 1, 1|2]
//                                  -> suffix sums of dL/dpx, dL/dpz, then the transpose of the rotation of frame s
//   heading       (0):             ang[t] = sum_{s < t} v[s, 0] -> strict suffix sum of dL/dang, which collects the chain
//                                  through rot_y / cos / sin of the ric joints and of the root velocity of frame t
// One workgroup per sample; the sample's 4 + 3(J-1) steerable columns live in LDS for all iterations, row stride padded odd
// (no bank conflicts between frame threads).  Frame phases run one thread per frame (a thread walks its frame's J joints, so
// per-frame sums need no atomics and the result is deterministic); the three scans run in one thread with fp64
// accumulators.  No other column of the feature row enters recover_from_ric, so none is read or written.
// Host side: the eight entries fill joint_control.h's Terms and Clock, name their level and call launch_control, which holds
// the frame limit, the common checks (args_ok), the choice of the kernel form and the file's one launch.
#include "joint_control.h"
#include "kernels.h"

namespace mdm {
namespace {

using namespace control;

constexpr int CTRL_THREADS = 256;
constexpr int CTRL_LDS_BYTES = 64 * 1024;
enum { CW, SW, RX, RZ, PX, PZ, GX, GZ, GA, GH, FR };  // fields of the per-frame record
constexpr int CTRL_FRAME_BYTES = FR * 4 + 8;          // per frame: the record + the fp64 loss

// GUIDE = false: mdm_joint_loss_grad (one evaluation; loss_out and the dense gradient grad_out written).
// GUIDE = true:  mdm_joint_guidance (iters steps of x0 -= scale (1 - m) grad in LDS, then x0 / x updated where delta != 0).
// SCENE = true:  the mdm_joint_scene_* calls: the scene's penalty of every joint (scene_sdf.h) joins the loss
//                and dL/dP, with K primitive records and the joints' (radius, weight) per sample; targets / weights may
//                then both be null (no target term).
// TRACKS = true: the mdm_joint_tracks_* calls, with SCENE: Km more records per frame, read from global memory
//                at tracks + ((b T + t) Km) SCENE_REC, behind the frame's bounding ball of tbounds (null: never skipped).
// TERRAIN = true: the mdm_joint_terrain_* calls, with TRACKS (Km may be 0): the height grid of the sample at
//                terrain + b Gz Gx with its record at trec + b TERRAIN_REC, gdim = Gx | Gz << 16, and the stand weights of
//                frame t at stand + (b T + t) J (null: all 0), all three read from global memory (terrain.h).
template <bool GUIDE, bool MASK, bool SCENE, bool TRACKS = false, bool TERRAIN = false>
__global__ __launch_bounds__(CTRL_THREADS) void joint_control_kernel(
    float* x0, float* x, const float* __restrict__ mask, const int* __restrict__ len, const float* __restrict__ mean,
    const float* __restrict__ sd, const float* __restrict__ targets, const float* __restrict__ weights, int T, int F,
    int J, float scale, int iters, const float* __restrict__ coef, int steps, const int* __restrict__ t_ptr, int t_imm,
    float* __restrict__ loss_out, float* __restrict__ grad_out, const float* __restrict__ scene, int K,
    const float* __restrict__ jparams, const float* __restrict__ tracks, int Km, const float* __restrict__ tbounds,
    const float* __restrict__ terrain, const float* __restrict__ trec, int gdim, const float* __restrict__ stand) {
  static_assert(SCENE || !TRACKS, "tracks use the scene's joint parameters");
  static_assert(TRACKS || !TERRAIN, "the terrain rides on the forms that keep their pointers in vector registers");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int D = 3 * J + 1;               // steerable columns: root (4) + ric (3 (J - 1))
  const int DS = D | 1;                  // odd LDS row stride
  double* lossF = (double*)smem_raw;     // [T]
  float* lsd = (float*)(lossF + T);      // [DS] std and mean of the steerable columns (in LDS: as scalar loads hoisted
  float* lmean = lsd + DS;               //      out of the loops they would take scalar registers the kernel lacks)
  float* prims = lmean + DS;             // SCENE: [K][SCENE_REC] the primitive records and [J][2] the joints' (radius, weight)
  float* jp = prims + (SCENE ? K * scene::SCENE_REC : 0);
  float* xs = jp + (SCENE ? 2 * J : 0);  // [T][DS] the steerable columns of x0, normalised
  // per-frame record fr[t * FR + k] (one LDS base for all of them):
  //   CW, SW   cos / sin of the heading of frame t
  //   RX, RZ   root velocity of frame t - 1 rotated by the heading of frame t
  //   PX, PZ   root XZ; after the frame phase: dL/dv[t, 1], dL/dv[t, 2]
  //   GX, GZ   sum_j dL/dP[t, j, x] and z
  //   GA       dL/dang[t] of the ric joints; after the scan: dL/dv[t, 0]
  //   GH       dL/dv[t, 3] (root height)
  float* fr = xs + T * DS;
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = len[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  const int64_t row0 = (int64_t)b * T * F;
  const float* tg = scene::own<TRACKS>(targets + (int64_t)b * T * J * 3);
  const float* wt = scene::own<TRACKS>(weights + (int64_t)b * T * J * 3);
  const float* mk = MASK ? scene::own<TRACKS>(mask + row0) : nullptr;
  const bool aim = !SCENE || targets != nullptr;  // a scene may come without targets
  grad_out = scene::own<TRACKS && !GUIDE>(grad_out);
  x0 = scene::own<TRACKS>(x0), x = scene::own<TRACKS && GUIDE>(x);
  float c0 = 0.f;  // read before the iterations: keeps the table's pointers out of the loop's scalar registers
  if (GUIDE) {
    int ts = t_ptr ? *t_ptr : t_imm;
    ts = min(max(ts, 0), steps - 1);
    c0 = coef[4 * ts + 1];
  }

  // TRACKS: the records and the ball of frame tid, as addresses of this thread's own (in vector registers: the two pointers
  // would take scalar registers the iteration loop lacks)
  const float* trk0 = nullptr;
  const float* bnd0 = nullptr;
  if (TRACKS) {
    trk0 = tracks + ((int64_t)b * T + tid) * Km * scene::SCENE_REC;
    if (!TERRAIN && tbounds) bnd0 = tbounds + ((int64_t)b * T + tid) * 4;  // TERRAIN: set below, never null
  }
  // TERRAIN: the grid, the record and the stand weights of frame tid, held the same way; the grid's sides in one register.
  // Without stand weights (and without balls) the reads go to the sample's record with steps of 0, and their bits are
  // masked out: a test of the pointer inside the iteration loop is hoisted as a lane mask into a pair of scalar registers.
  const float* hgrid = nullptr;
  const float* hrec = nullptr;
  const float* std0 = nullptr;
  int gd = 0, sstep = 0, bstep = 0;
  if (TERRAIN) {
    gd = terrain::own(gdim);
    hgrid = scene::own<TERRAIN>(terrain + (int64_t)b * (gdim & 0xffff) * (gdim >> 16));
    hrec = scene::own<TERRAIN>(trec + (int64_t)b * terrain::TERRAIN_REC);
    std0 = scene::own<TERRAIN>(stand ? stand + ((int64_t)b * T + tid) * J : trec + (int64_t)b * terrain::TERRAIN_REC);
    sstep = terrain::own(stand ? 1 : 0);
    bnd0 = scene::own<TERRAIN>(tbounds ? tbounds + ((int64_t)b * T + tid) * 4 : trec + (int64_t)b * terrain::TERRAIN_REC);
    bstep = terrain::own(tbounds ? 1 : 0);
  }

  if (!GUIDE) {  // every entry that cannot receive gradient: frames past the length and the columns past D
    float* gb = grad_out + row0;
    for (int64_t i = tid; i < (int64_t)T * F; i += CTRL_THREADS) {
      const int t = (int)(i / F), c = (int)(i - (int64_t)t * F);
      if (t >= n || c >= D) gb[i] = 0.f;
    }
  }
  for (int i = tid; i < n * D; i += CTRL_THREADS) {
    const int t = i / D, c = i - t * D;
    xs[t * DS + c] = x0[row0 + (int64_t)t * F + c];
  }
  for (int c = tid; c < D; c += CTRL_THREADS) lsd[c] = sd[(int64_t)b * F + c], lmean[c] = mean[(int64_t)b * F + c];
  if (SCENE) {
    for (int i = tid; i < K * scene::SCENE_REC; i += CTRL_THREADS) prims[i] = scene[(int64_t)b * K * scene::SCENE_REC + i];
    for (int i = tid; i < 2 * J; i += CTRL_THREADS) jp[i] = jparams[(int64_t)b * 2 * J + i];
  }
  __syncthreads();
  auto val = [&](int t, int c) { return add(mul(xs[t * DS + c], lsd[c]), lmean[c]); };
  // one gradient entry g (w.r.t. the normalised feature): written out, or the guidance step applied in LDS
  // TERRAIN: the step size and the mask's row stride as values of the thread's own as well
  const float step = TERRAIN ? __int_as_float(terrain::own(__float_as_int(scale))) : scale;
  const int mF = TERRAIN && MASK ? terrain::own(F) : F;
  auto emit = [&](int t, int c, float g) {
    if (GUIDE) {
      const float u = MASK ? (1.f - mk[(int64_t)t * mF + c]) * g : g;
      xs[t * DS + c] = xs[t * DS + c] - step * u;
    } else {
      grad_out[row0 + (int64_t)t * F + c] = g;
    }
  };

#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // heading: exclusive prefix sum of the rotation velocity (motion_post_kernel order)
    if (tid == 0) {
      double acc = 0.0;
      for (int t = 0; t < n; ++t) {
        if (t > 0) acc += (double)val(t - 1, 0);
        const float a = (float)acc;
        fr[t * FR + CW] = cosf(a), fr[t * FR + SW] = sinf(a);
      }
    }
    __syncthreads();
    for (int t = tid; t < n; t += CTRL_THREADS) {
      float vx = 0.f, vz = 0.f;
      if (t > 0) vx = val(t - 1, 1), vz = val(t - 1, 2);
      float ox, oz;
      rot_y(fr[t * FR + CW], -fr[t * FR + SW], vx, vz, ox, oz);
      fr[t * FR + RX] = ox, fr[t * FR + RZ] = oz;
    }
    __syncthreads();
    if (tid == 0) {
      double ax = 0.0, az = 0.0;
      for (int t = 0; t < n; ++t) {
        ax += (double)fr[t * FR + RX], az += (double)fr[t * FR + RZ];
        fr[t * FR + PX] = (float)ax, fr[t * FR + PZ] = (float)az;
      }
    }
    __syncthreads();
    // frame phase: P, dL/dP, the ric columns' gradient (local to the frame) and the per-frame sums the scans need
    for (int t = tid; t < n; t += CTRL_THREADS) {
      const float c = fr[t * FR + CW], s = fr[t * FR + SW], qx = fr[t * FR + PX], qz = fr[t * FR + PZ];
      const RotD r = rot_d(c, s);
      const float* tgt = tg + (int64_t)t * J * 3;
      const float* wgt = wt + (int64_t)t * J * 3;
      double lsum = 0.0, sx = 0.0, sz = 0.0, sa = 0.0;
      float g[3];
      const float* trk = nullptr;  // TRACKS: the frame's records and its ball
      float ball[4] = {0.f, 0.f, 0.f, INFINITY};
      if (TRACKS) {
        trk = trk0 + (int64_t)(t - tid) * Km * scene::SCENE_REC;
        if (!TERRAIN && bnd0) {
          const float4 bb = *reinterpret_cast<const float4*>(bnd0 + (int64_t)(t - tid) * 4);
          ball[0] = bb.x, ball[1] = bb.y, ball[2] = bb.z, ball[3] = bb.w;
        }
      }
      float hr[terrain::TERRAIN_REC];  // TERRAIN: the sample's record and the frame's stand weights
      const float* stw = nullptr;
      if (TERRAIN) {
        terrain::load_record(hrec, hr);
        stw = std0 + (int64_t)(t - tid) * J * sstep;
        const float4 bb = *reinterpret_cast<const float4*>(bnd0 + (int64_t)(t - tid) * 4 * bstep);
        ball[0] = bb.x, ball[1] = bb.y, ball[2] = bb.z, ball[3] = terrain::pick(bb.w, INFINITY, bstep);  // no balls: never skipped
      }
      auto dl = [&](int k, float p) {  // dL/dP of one coordinate; W == 0 contributes nothing, whatever G holds
        if (SCENE && !aim) return 0.f;
        const float w = wgt[k];
        if (w == 0.f) return 0.f;
        const float d = p - tgt[k];
        lsum += (double)w * (double)d * (double)d;
        return 2.f * w * d;
      };
      {  // joint 0: root XZ and height
        const float py = val(t, 3);
        g[0] = dl(0, qx), g[1] = dl(1, py), g[2] = dl(2, qz);
        if (SCENE && !TRACKS) lsum += scene::penalty(prims, K, jp[0], jp[1], qx, py, qz, g);
        if (TRACKS) lsum += scene::penalty_tracks(prims, K, trk, Km, ball, jp[0], jp[1], qx, py, qz, g);
        if (TERRAIN)
          lsum += terrain::penalty(hgrid, gd & 0xffff, gd >> 16, hr, jp[0], jp[1], terrain::stand_weight(stw, 0, sstep), qx, py,
                                   qz, g);
        sx += g[0], sz += g[2];
        fr[t * FR + GH] = g[1];
      }
#pragma unroll 1
      for (int j = 1; j < J; ++j) {
        const int col = 4 + 3 * (j - 1);
        const float vx = val(t, col), vy = val(t, col + 1), vz = val(t, col + 2);
        float ox, oz;
        rot_y(c, -s, vx, vz, ox, oz);
        const float px = add(ox, qx), pz = add(oz, qz);
        g[0] = dl(3 * j, px), g[1] = dl(3 * j + 1, vy), g[2] = dl(3 * j + 2, pz);
        if (SCENE && !TRACKS) lsum += scene::penalty(prims, K, jp[2 * j], jp[2 * j + 1], px, vy, pz, g);
        if (TRACKS) lsum += scene::penalty_tracks(prims, K, trk, Km, ball, jp[2 * j], jp[2 * j + 1], px, vy, pz, g);
        if (TERRAIN)
          lsum += terrain::penalty(hgrid, gd & 0xffff, gd >> 16, hr, jp[2 * j], jp[2 * j + 1],
                                   terrain::stand_weight(stw, j, sstep), px, vy, pz, g);
        if (GUIDE && g[0] == 0.f && g[1] == 0.f && g[2] == 0.f) continue;  // no step: the entries keep their bits
        sx += g[0], sz += g[2];
        sa += 2.0 * ((double)g[0] * (r.e * vz + r.f * vx) + (double)g[2] * (r.f * vz - r.e * vx));
        const float gvx = (float)((double)g[0] * r.a11 - (double)g[2] * r.a13);
        const float gvz = (float)((double)g[0] * r.a13 + (double)g[2] * r.a11);
        emit(t, col, gvx * lsd[col]);
        emit(t, col + 1, g[1] * lsd[col + 1]);
        emit(t, col + 2, gvz * lsd[col + 2]);
      }
      lossF[t] = lsum;
      fr[t * FR + GX] = (float)sx, fr[t * FR + GZ] = (float)sz, fr[t * FR + GA] = (float)sa;
    }
    __syncthreads();
    // reverse scans (fp64): dL/drx[t] = sum_{u >= t} GX[u]; dL/dv[t, 0] = sum_{u > t} dL/dang[u].  Reads CW / SW /
    // the root velocity columns (not yet updated); writes dL/dv[t-1, 1|2] into PX / PZ and dL/dv[t, 0] over GA.
    if (tid == 0) {
      double sx = 0.0, sz = 0.0, sang = 0.0, loss = 0.0;
      if (n > 0) fr[(n - 1) * FR + PX] = 0.f, fr[(n - 1) * FR + PZ] = 0.f;
      for (int t = n - 1; t >= 0; --t) {
        sx += (double)fr[t * FR + GX], sz += (double)fr[t * FR + GZ];
        double gat = (double)fr[t * FR + GA];
        if (t > 0) {
          const RotD r = rot_d(fr[t * FR + CW], fr[t * FR + SW]);
          const double vx = (double)val(t - 1, 1), vz = (double)val(t - 1, 2);
          gat += 2.0 * (sx * (r.e * vz + r.f * vx) + sz * (r.f * vz - r.e * vx));
          fr[(t - 1) * FR + PX] = (float)(sx * r.a11 - sz * r.a13);
          fr[(t - 1) * FR + PZ] = (float)(sx * r.a13 + sz * r.a11);
        }
        fr[t * FR + GA] = (float)sang;
        sang += gat;
      }
      if (!GUIDE) {
        for (int t = 0; t < n; ++t) loss += lossF[t];
        loss_out[b] = (float)loss;
      }
    }
    __syncthreads();
    for (int t = tid; t < n; t += CTRL_THREADS) {
      emit(t, 0, fr[t * FR + GA] * lsd[0]);
      emit(t, 1, fr[t * FR + PX] * lsd[1]);
      emit(t, 2, fr[t * FR + PZ] * lsd[2]);
      emit(t, 3, fr[t * FR + GH] * lsd[3]);
    }
    __syncthreads();
  }
  if (GUIDE) {  // delta = x0' - x0: x0 <- x0', x <- x + c0[t] delta; nothing stored where delta == 0
    for (int i = tid; i < n * D; i += CTRL_THREADS) {
      const int t = i / D, c = i - t * D;
      const int64_t e = row0 + (int64_t)t * F + c;
      const float nv = xs[t * DS + c], ov = x0[e], dlt = nv - ov;
      if (dlt != 0.f) {
        x0[e] = nv;
        x[e] = x[e] + c0 * dlt;
      }
    }
  }
}

// prims < 0: no scene; else the K = prims primitive records and the joints' (radius, weight) as well
size_t control_lds_bytes(int T, int J, int prims = -1) {
  const int DS = (3 * J + 1) | 1;
  const size_t scene = prims < 0 ? 0 : ((size_t)prims * scene::SCENE_REC + 2 * J) * 4;
  return (size_t)2 * DS * 4 + scene + (size_t)T * ((size_t)DS * 4 + CTRL_FRAME_BYTES);
}

// Every entry below: the checks of an entry of `level`, then the one launch, of the form the terms present ask for.
// g: the clock of a guidance call (x and x0 updated), null for a loss_grad call (loss_out and grad_out written).
int launch_control(Level level, const Clock* g, float* x, float* x0, const float* mask, const int32_t* length, const float* mean,
                   const float* std, const float* targets, const float* weights, const Terms& o, int B, int T, int F,
                   float* loss_out, float* grad_out, void* stream) {
  if (!x0 || !length || !mean || !std || (g ? !x : !loss_out || !grad_out)) return MDM_ERR_ARG;
  if (!args_ok(level, targets, weights, o, g)) return MDM_ERR_ARG;
  const int J = control_joints(F);
  // the frame limit is the level's, also where the call falls through to a form that would hold more frames
  const int limit = level == PLAIN ? mdm_joint_control_max_frames(F) : mdm_joint_scene_max_frames(F, o.K);
  if (J == 0 || B < 0 || T < 1 || T > limit) return MDM_ERR_ARG;
  if (B == 0) return MDM_OK;
  const Level form = kernel_form(targets, o.K, o.Km, o.terrain);
  const Terms u = terms_of(form, o);
  const Clock c = g ? *g : ONE_EVALUATION;
  const size_t smem = control_lds_bytes(T, J, form == PLAIN ? -1 : u.K);
  dispatch(g != nullptr, mask != nullptr, form, [&](auto k) {
    using Kn = decltype(k);
    hipLaunchKernelGGL((joint_control_kernel<Kn::GUIDE, Kn::MASK, Kn::SCENE, Kn::TRACKS, Kn::TERRAIN>), dim3(B), dim3(CTRL_THREADS),
                       smem, (hipStream_t)stream, x0, x, mask, length, mean, std, targets, weights, T, F, J, c.scale, c.iters,
                       c.coef, c.steps, c.t_dev, c.t_imm, loss_out, grad_out, u.scene, u.K, u.joint_params, u.tracks, u.Km,
                       u.track_bounds, u.terrain, u.terrain_rec, u.Gx | u.Gz << 16, u.stand);
  });
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int max_frames(int J, int prims) {
  const size_t fixed = control_lds_bytes(0, J, prims), frame = control_lds_bytes(1, J, prims) - fixed;
  return (int)((CTRL_LDS_BYTES - fixed) / frame);
}

}  // namespace
}  // namespace mdm

namespace ctl = mdm::control;

extern "C" {

int mdm_joint_control_max_frames(int32_t feats) {
  const int J = ctl::control_joints(feats);
  return J == 0 ? 0 : mdm::max_frames(J, -1);
}

int mdm_joint_scene_max_frames(int32_t feats, int32_t prims) {
  const int J = ctl::control_joints(feats);
  return J == 0 || prims < 0 || prims > MDM_SCENE_MAX_PRIMS ? 0 : mdm::max_frames(J, prims);
}

int mdm_joint_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                        const float* weights, int32_t B, int32_t T, int32_t F, float* loss_out, float* grad_out,
                        void* stream) {
  return mdm::launch_control(ctl::PLAIN, nullptr, nullptr, const_cast<float*>(x0), nullptr, length, mean, std, targets,
                             weights, ctl::Terms{}, B, T, F, loss_out, grad_out, stream);
}

int mdm_joint_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                       const float* targets, const float* weights, int32_t B, int32_t T, int32_t F, float scale,
                       int32_t iters, const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm,
                       void* stream) {
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_control(ctl::PLAIN, &g, x, x0, mask, length, mean, std, targets, weights, ctl::Terms{}, B, T, F, nullptr,
                             nullptr, stream);
}

int mdm_joint_scene_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                              const float* weights, const float* scene, int32_t K, const float* joint_params, int32_t B,
                              int32_t T, int32_t F, float* loss_out, float* grad_out, void* stream) {
  const ctl::Terms o = {scene, K, joint_params};
  return mdm::launch_control(ctl::SCENE, nullptr, nullptr, const_cast<float*>(x0), nullptr, length, mean, std, targets,
                             weights, o, B, T, F, loss_out, grad_out, stream);
}

int mdm_joint_scene_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                             const float* targets, const float* weights, const float* scene, int32_t K,
                             const float* joint_params, int32_t B, int32_t T, int32_t F, float scale, int32_t iters,
                             const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, void* stream) {
  const ctl::Terms o = {scene, K, joint_params};
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_control(ctl::SCENE, &g, x, x0, mask, length, mean, std, targets, weights, o, B, T, F, nullptr,
                             nullptr, stream);
}

int mdm_joint_tracks_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                               const float* weights, const float* scene, int32_t K, const float* joint_params,
                               const float* tracks, int32_t Km, const float* track_bounds, int32_t B, int32_t T, int32_t F,
                               float* loss_out, float* grad_out, void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds};
  return mdm::launch_control(ctl::TRACKS, nullptr, nullptr, const_cast<float*>(x0), nullptr, length, mean, std, targets,
                             weights, o, B, T, F, loss_out, grad_out, stream);
}

int mdm_joint_tracks_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                              const float* targets, const float* weights, const float* scene, int32_t K,
                              const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds, int32_t B,
                              int32_t T, int32_t F, float scale, int32_t iters, const float* coef, int32_t steps,
                              const int32_t* t_dev, int32_t t_imm, void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds};
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_control(ctl::TRACKS, &g, x, x0, mask, length, mean, std, targets, weights, o, B, T, F, nullptr,
                             nullptr, stream);
}

int mdm_joint_terrain_loss_grad(const float* x0, const int32_t* length, const float* mean, const float* std, const float* targets,
                                const float* weights, const float* scene, int32_t K, const float* joint_params,
                                const float* tracks, int32_t Km, const float* track_bounds, const float* terrain,
                                const float* terrain_rec, int32_t Gx, int32_t Gz, const float* stand, int32_t B, int32_t T,
                                int32_t F, float* loss_out, float* grad_out, void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds, terrain, terrain_rec, Gx, Gz, stand};
  return mdm::launch_control(ctl::TERRAIN, nullptr, nullptr, const_cast<float*>(x0), nullptr, length, mean, std,
                             targets, weights, o, B, T, F, loss_out, grad_out, stream);
}

int mdm_joint_terrain_guidance(float* x, float* x0, const float* mask, const int32_t* length, const float* mean, const float* std,
                               const float* targets, const float* weights, const float* scene, int32_t K,
                               const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds,
                               const float* terrain, const float* terrain_rec, int32_t Gx, int32_t Gz, const float* stand,
                               int32_t B, int32_t T, int32_t F, float scale, int32_t iters, const float* coef, int32_t steps,
                               const int32_t* t_dev, int32_t t_imm, void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds, terrain, terrain_rec, Gx, Gz, stand};
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_control(ctl::TERRAIN, &g, x, x0, mask, length, mean, std, targets, weights, o, B, T, F, nullptr,
                             nullptr, stream);
}

}  // extern "C"
