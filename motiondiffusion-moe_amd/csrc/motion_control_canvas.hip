// Joint-position control over a long motion's canvas: the loss and gradient of motion_control.hip (§14)
// over canvas frames whose feature rows a table names, with no limit on the canvas length.
//   canvas frames of motion m:  c in [motion_offsets[m], motion_offsets[m + 1]);  feature row of c:  frame_rows[c]
//   P = recover_from_ric(x0 * std + mean),  L_m = sum W (P - G)^2,  gradient with respect to the normalised features
// One workgroup per motion.  Frames go through it in blocks of CV_THREADS, one frame per thread, so canvas frame t always
// belongs to thread t % CV_THREADS; what a frame keeps between passes lives in the workspace (global memory, written and
// re-read by this workgroup only, across __syncthreads()): the working copy of its 3J + 1 steerable columns, laid out
// [column][frame] so that the lanes of a wave touch consecutive addresses, and a record of six floats.
// An iteration is two passes over the blocks, every scan an additive fp64 scan: shuffle scan inside a wave, the four wave
// totals through LDS, the carry of the blocks already done in a register of every thread.
//   forward pass, blocks ascending:   heading ang[t] = sum_{s < t} v[s, 0]  (inclusive scan of the velocity shifted by one frame)
//                                     root XZ = inclusive scan of the rotated root velocity;  then the frame's own work:
//                                     P, dL/dP, the ric columns' gradient, and the sums GX, GZ, GA, GH the reverse pass needs
//   reverse pass, blocks descending:  sx, sz[t] = suffix sums of GX, GZ;  frame-parallel: the XZ gradient of row t - 1 and
//                                     gat[t] = GA[t] + the chain of sx, sz through the rotation of frame t;
//                                     dL/dv[t, 0] = strict suffix sum of gat
// The forward pass writes ric columns only (read by their own frame); the reverse pass writes the root columns: row t's
// heading velocity and height by thread t, row t - 1's XZ by thread t, which is also the only thread that reads them in that
// pass.  The next forward pass reads row t - 1 from thread t: one barrier between iterations orders that.
// Every lane executes every shuffle and barrier: frames at or past the motion's end contribute zeros, and the trip counts
// of the loops around barriers depend on the motion alone.  The summation order differs from motion_post_kernel's serial
// scans: P agrees with mdm_motion_postprocess to rounding, not bit for bit.
// Host side: the eight entries fill joint_control.h's Terms and Clock, name their level and call launch_canvas, which holds
// the workspace and LDS-size checks, the common checks (args_ok), the choice of the kernel form and the file's one launch.
#include "joint_control.h"
#include "kernels.h"

#include <cstdint>

namespace mdm {
namespace {

using namespace control;

constexpr int CV_THREADS = 256;
constexpr int CV_WAVES = CV_THREADS / 64;
constexpr int CV_JOINTS = 3;  // joints whose inputs a frame's thread has in flight
constexpr int CV_TILE = 64;  // frames per LDS tile when the working copy is loaded and written back
constexpr int CV_BATCH = 6;  // elements of a tile a thread has in flight in the write-back
enum { CW, SW, GX, GZ, GA, GH, FR };  // fields of the per-frame record

// Inclusive prefix (REVERSE: suffix) sum of v over the workgroup's threads, on top of `carry`, the sum of the blocks
// already scanned; `carry` then takes this block in.  `excl` (may be null): the same without the thread's own value.
// slot: CV_WAVES doubles of LDS.  Two barriers; all threads of the workgroup call it.  A lane without a partner at
// distance d adds its partner's value times 0.0, one fma: as lane masks the twelve loop-invariant conditions of the two
// directions would take scalar registers the kernel lacks (values are finite: the runner checks its inputs).
template <bool REVERSE>
__device__ __forceinline__ double block_scan(double v, double& carry, double* slot, double* excl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = REVERSE ? __shfl_down(v, d, 64) : __shfl_up(v, d, 64);
    v = fma(o, (double)(REVERSE ? lane + d < 64 : lane >= d), v);
  }
  const double nb = REVERSE ? __shfl_down(v, 1, 64) : __shfl_up(v, 1, 64);
  if (lane == (REVERSE ? 0 : 63)) slot[wave] = v;
  __syncthreads();
  double pre = carry, total = carry;
#pragma unroll
  for (int i = 0; i < CV_WAVES; ++i) {
    const int w = REVERSE ? CV_WAVES - 1 - i : i;  // in scan order
    const double s = slot[w];
    if (REVERSE ? w > wave : w < wave) pre += s;
    total += s;
  }
  __syncthreads();  // the slot may be written again
  carry = total;
  if (excl) *excl = pre + (lane == (REVERSE ? 63 : 0) ? 0.0 : nb);
  return pre + v;
}

// GUIDE = false: mdm_canvas_joint_loss_grad.  GUIDE = true: mdm_canvas_joint_guidance.
// SCENE = true: the mdm_canvas_scene_* calls: the scene's penalty of every joint (scene_sdf.h) joins the loss
// and dL/dP, with K primitive records and the joints' (radius, weight) per motion, in the canvas frame; targets / weights
// may then both be null.
// TRACKS = true: the mdm_canvas_tracks_* calls, with SCENE: Km more records per canvas frame, read from global
// memory at tracks + ((motion_offsets[m] + t) Km) SCENE_REC, behind the frame's bounding ball of tbounds (null: never skipped).
// TERRAIN = true: the mdm_canvas_terrain_* calls, with TRACKS (Km may be 0): the height grid of motion m at
// terrain + m Gz Gx with its record at trec + m TERRAIN_REC, gdim = Gx | Gz << 16, and the stand weights of canvas frame t at
// stand + (motion_offsets[m] + t) J (null: all 0), all three read from global memory (terrain.h), in the canvas frame.
template <bool GUIDE, bool MASK, bool SCENE, bool TRACKS = false, bool TERRAIN = false>
__global__ __launch_bounds__(CV_THREADS) void canvas_control_kernel(
    float* x0, float* x, const float* __restrict__ mask, const int* __restrict__ offs, const int* __restrict__ frows,
    const float* __restrict__ mean, const float* __restrict__ sd, const float* __restrict__ targets,
    const float* __restrict__ weights, int F, int J, float scale, int iters, const float* __restrict__ coef, int steps,
    const int* __restrict__ t_ptr, int t_imm, float* loss_out, float* grad_out, float* ws,
    const float* __restrict__ scene, int K, const float* __restrict__ jparams, const float* __restrict__ tracks, int Km,
    const float* __restrict__ tbounds, const float* __restrict__ terrain, const float* __restrict__ trec, int gdim,
    const float* __restrict__ stand) {
  static_assert(SCENE || !TRACKS, "tracks use the scene's joint parameters");
  static_assert(TRACKS || !TERRAIN, "the terrain rides on the forms that keep their pointers in vector registers");
  __shared__ double slots[3][CV_WAVES];  // the wave totals of up to three scans in flight
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int D = 3 * J + 1;          // steerable columns: root (4) + ric (3 (J - 1))
  float* lsd = (float*)smem_raw;    // [D] std and mean of the steerable columns
  float* lmean = lsd + D;           // [D]
  const int DS = D | 1;             // odd row stride of the tile: frames along the lanes without bank conflicts
  float* prims = lmean + D;         // SCENE: [K][SCENE_REC] the primitive records and [J][2] the joints' (radius, weight)
  float* jp = prims + (SCENE ? K * scene::SCENE_REC : 0);
  float* tile = jp + (SCENE ? 2 * J : 0);  // [CV_TILE][DS]
  const int m = blockIdx.x, tid = threadIdx.x;
  const int c0 = offs[m];
  const int n = min(max(offs[m + 1] - c0, 0), INT32_MAX / (D + FR));  // offsets inside a motion's state are int32
  const int nblk = (n + CV_THREADS - 1) / CV_THREADS;
  float* xs = scene::own<TRACKS>(ws + (int64_t)c0 * (D + FR));  // [D][n] the steerable columns of x0, normalised
  float* fr = xs + D * n;  // [n][FR] the record (read back by the thread that wrote it):
  //   CW, SW   cos / sin of the heading of frame t
  //   GX, GZ   sum_j dL/dP[t, j, x] and z
  //   GA       dL/dang[t] of the ric joints
  //   GH       dL/dv[t, 3] (root height)
  const int* rows = scene::own<TRACKS>(frows + c0);
  const float* tg = scene::own<TRACKS>(targets + (int64_t)c0 * J * 3);
  const float* wt = scene::own<TRACKS>(weights + (int64_t)c0 * J * 3);
  const bool aim = !SCENE || targets != nullptr;  // a scene may come without targets
  mask = scene::own<TRACKS && MASK>(mask), grad_out = scene::own<TRACKS && !GUIDE>(grad_out);
  x0 = scene::own<TRACKS>(x0), x = scene::own<TRACKS && GUIDE>(x), loss_out = scene::own<TRACKS && !GUIDE>(loss_out);
  float c0t = 0.f;
  if (GUIDE) {
    int ts = t_ptr ? *t_ptr : t_imm;
    ts = min(max(ts, 0), steps - 1);
    c0t = coef[4 * ts + 1];
  }

  // TRACKS: the records and the ball of canvas frame tid of this motion, as addresses of this thread's own (in vector
  // registers: the two pointers would take scalar registers the iteration loop lacks)
  const float* trk0 = nullptr;
  const float* bnd0 = nullptr;
  if (TRACKS) {
    trk0 = tracks + ((int64_t)c0 + tid) * Km * scene::SCENE_REC;
    if (!TERRAIN && tbounds) bnd0 = tbounds + ((int64_t)c0 + tid) * 4;  // TERRAIN: set below, never null
  }
  // TERRAIN: the grid, the record and the stand weights of canvas frame tid, held the same way; the grid's sides in one
  // register.  Without stand weights (and without balls) the reads go to the motion's record with steps of 0, and their bits
  // are masked out: a test of the pointer inside the iteration loop is hoisted as a lane mask into a pair of scalar registers.
  const float* hgrid = nullptr;
  const float* hrec = nullptr;
  const float* std0 = nullptr;
  int gd = 0, sstep = 0, bstep = 0;
  if (TERRAIN) {
    gd = terrain::own(gdim);
    hgrid = scene::own<TERRAIN>(terrain + (int64_t)m * (gdim & 0xffff) * (gdim >> 16));
    hrec = scene::own<TERRAIN>(trec + (int64_t)m * terrain::TERRAIN_REC);
    std0 = scene::own<TERRAIN>(stand ? stand + ((int64_t)c0 + tid) * J : trec + (int64_t)m * terrain::TERRAIN_REC);
    sstep = terrain::own(stand ? 1 : 0);
    bnd0 = scene::own<TERRAIN>(tbounds ? tbounds + ((int64_t)c0 + tid) * 4 : trec + (int64_t)m * terrain::TERRAIN_REC);
    bstep = terrain::own(tbounds ? 1 : 0);
  }

  if (!GUIDE) {  // the columns past D never receive gradient
    float* gb = grad_out + (int64_t)c0 * F;
    const int R = F - D;
    for (int64_t i = tid; i < (int64_t)n * R; i += CV_THREADS) {
      const int64_t t = i / R;
      gb[t * F + D + (i - t * R)] = 0.f;
    }
  }
  // The working copy is the transpose of the rows ([column][frame]): tiles of CV_TILE frames go through LDS, so that the
  // rows are read along their columns and the copy is written along its frames, both with the lanes on consecutive
  // addresses (one element at a time costs a cache-line transaction per lane on one side or the other).
  for (int t0 = 0; t0 < n; t0 += CV_TILE) {
    const int nt = min(CV_TILE, n - t0);
    for (int i = tid; i < nt * D; i += CV_THREADS) {
      const int tt = i / D, c = i - tt * D;
      tile[tt * DS + c] = x0[(int64_t)rows[t0 + tt] * F + c];
    }
    __syncthreads();
    for (int i = tid; i < nt * D; i += CV_THREADS) {
      const int c = i / nt, tt = i - c * nt;
      xs[c * n + t0 + tt] = tile[tt * DS + c];
    }
    __syncthreads();
  }
  for (int c = tid; c < D; c += CV_THREADS) lsd[c] = sd[(int64_t)m * F + c], lmean[c] = mean[(int64_t)m * F + c];
  if (SCENE) {
    for (int i = tid; i < K * scene::SCENE_REC; i += CV_THREADS) prims[i] = scene[(int64_t)m * K * scene::SCENE_REC + i];
    for (int i = tid; i < 2 * J; i += CV_THREADS) jp[i] = jparams[(int64_t)m * 2 * J + i];
  }
  __syncthreads();
  auto val = [&](int t, int c) { return add(mul(xs[c * n + t], lsd[c]), lmean[c]); };
  // one gradient entry g (w.r.t. the normalised feature): written out, or the guidance step applied to the working copy
  auto emit = [&](int t, int c, float g) {
    if (GUIDE) {
      const float u = MASK ? (1.f - mask[(int64_t)rows[t] * F + c]) * g : g;
      float* p = xs + (c * n + t);
      *p = *p - scale * u;
    } else {
      grad_out[(int64_t)(c0 + t) * F + c] = g;
    }
  };

  double lacc = 0.0;  // this thread's frames' share of the loss
  const int passes = TERRAIN && !GUIDE ? 1 : iters;  // the loss and gradient are one evaluation: no counter to hold
#pragma unroll 1
  for (int it = 0; it < passes; ++it) {
    // ---- forward pass ----
    double cang = 0.0, cpx = 0.0, cpz = 0.0;
#pragma unroll 1
    for (int b = 0; b < nblk; ++b) {
      const int t = b * CV_THREADS + tid;
      const bool live = t < n;
      const bool prev = live && t > 0;
      const double ang = block_scan<false>(prev ? (double)val(t - 1, 0) : 0.0, cang, slots[0], nullptr);
      const float a = (float)ang;
      const float c = cosf(a), s = sinf(a);
      float ox = 0.f, oz = 0.f;
      if (live) {
        float vx = 0.f, vz = 0.f;
        if (prev) vx = val(t - 1, 1), vz = val(t - 1, 2);
        rot_y(c, -s, vx, vz, ox, oz);
      }
      const float qx = (float)block_scan<false>((double)ox, cpx, slots[1], nullptr);
      const float qz = (float)block_scan<false>((double)oz, cpz, slots[2], nullptr);
      if (live) {  // the frame: P, dL/dP, the ric columns' gradient (local to the frame) and the sums the scans need
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
        float hr[terrain::TERRAIN_REC];  // TERRAIN: the motion's record and the frame's stand weights
        const float* stw = nullptr;
        if (TERRAIN) {
          terrain::load_record(hrec, hr);
          stw = std0 + (int64_t)(t - tid) * J * sstep;
          const float4 bb = *reinterpret_cast<const float4*>(bnd0 + (int64_t)(t - tid) * 4 * bstep);
          ball[0] = bb.x, ball[1] = bb.y, ball[2] = bb.z, ball[3] = terrain::pick(bb.w, INFINITY, bstep);  // no balls: never skipped
        }
        auto dl = [&](float w, float gk, float p) {  // dL/dP of one coordinate; W == 0 contributes nothing, whatever G holds
          if (w == 0.f) return 0.f;
          const float d = p - gk;
          lsum += (double)w * (double)d * (double)d;
          return 2.f * w * d;
        };
        {  // joint 0
          const float py = val(t, 3);
          float w0[3] = {0.f, 0.f, 0.f}, g0[3] = {0.f, 0.f, 0.f};
          if (aim) {
#pragma unroll
            for (int k = 0; k < 3; ++k) w0[k] = wgt[k], g0[k] = tgt[k];
          }
          g[0] = dl(w0[0], g0[0], qx), g[1] = dl(w0[1], g0[1], py), g[2] = dl(w0[2], g0[2], qz);
          if (SCENE && !TRACKS) lsum += scene::penalty(prims, K, jp[0], jp[1], qx, py, qz, g);
          if (TRACKS) lsum += scene::penalty_tracks(prims, K, trk, Km, ball, jp[0], jp[1], qx, py, qz, g);
          if (TERRAIN)
            lsum += terrain::penalty(hgrid, gd & 0xffff, gd >> 16, hr, jp[0], jp[1], terrain::stand_weight(stw, 0, sstep), qx, py,
                                     qz, g);
        }
        sx += g[0], sz += g[2];
        fr[t * FR + GH] = g[1];
        // CV_JOINTS joints at a time, every load of a group issued before its first store (the working copy and the
        // gradient may alias the inputs for all the compiler knows): a frame's walk is a chain of memory latencies
        // otherwise, in HBM's on the first iteration of a step
#pragma unroll 1
        for (int j0 = 1; j0 < J; j0 += CV_JOINTS) {
          float wv[CV_JOINTS][3], gv[CV_JOINTS][3], xv[CV_JOINTS][3], mv[CV_JOINTS][3];
#pragma unroll
          for (int u = 0; u < CV_JOINTS; ++u) {
            const int j = min(j0 + u, J - 1), col = 4 + 3 * (j - 1);  // a group past the last joint re-reads it, unused
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              wv[u][k] = aim ? wgt[3 * j + k] : 0.f, gv[u][k] = aim ? tgt[3 * j + k] : 0.f, xv[u][k] = xs[(col + k) * n + t];
              mv[u][k] = GUIDE && MASK ? mask[(int64_t)rows[t] * F + col + k] : 0.f;
            }
          }
#pragma unroll
          for (int u = 0; u < CV_JOINTS; ++u) {
            const int j = j0 + u, col = 4 + 3 * (j - 1);
            if (j >= J) break;
            const float vx = add(mul(xv[u][0], lsd[col]), lmean[col]), vy = add(mul(xv[u][1], lsd[col + 1]), lmean[col + 1]),
                        vz = add(mul(xv[u][2], lsd[col + 2]), lmean[col + 2]);
            float rx, rz;
            rot_y(c, -s, vx, vz, rx, rz);
            const float px = add(rx, qx), pz = add(rz, qz);
            g[0] = dl(wv[u][0], gv[u][0], px), g[1] = dl(wv[u][1], gv[u][1], vy), g[2] = dl(wv[u][2], gv[u][2], pz);
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
            const float gk[3] = {gvx * lsd[col], g[1] * lsd[col + 1], gvz * lsd[col + 2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {  // emit() on the values already loaded
              if (GUIDE)
                xs[(col + k) * n + t] = xv[u][k] - scale * (MASK ? (1.f - mv[u][k]) * gk[k] : gk[k]);
              else
                grad_out[(int64_t)(c0 + t) * F + col + k] = gk[k];
            }
          }
        }
        lacc += lsum;
        fr[t * FR + CW] = c, fr[t * FR + SW] = s;
        fr[t * FR + GX] = (float)sx, fr[t * FR + GZ] = (float)sz, fr[t * FR + GA] = (float)sa;
      }
    }
    // ---- reverse pass: a thread reads back its own frames' records only ----
    double csx = 0.0, csz = 0.0, cga = 0.0;
#pragma unroll 1
    for (int b = nblk - 1; b >= 0; --b) {
      const int t = b * CV_THREADS + tid;
      const bool live = t < n;
      const double sx = block_scan<true>(live ? (double)fr[t * FR + GX] : 0.0, csx, slots[0], nullptr);
      const double sz = block_scan<true>(live ? (double)fr[t * FR + GZ] : 0.0, csz, slots[1], nullptr);
      double gat = 0.0;
      float gvx = 0.f, gvz = 0.f;
      if (live) {
        gat = (double)fr[t * FR + GA];
        if (t > 0) {
          const RotD r = rot_d(fr[t * FR + CW], fr[t * FR + SW]);
          const double vx = (double)val(t - 1, 1), vz = (double)val(t - 1, 2);
          gat += 2.0 * (sx * (r.e * vz + r.f * vx) + sz * (r.f * vz - r.e * vx));
          gvx = (float)(sx * r.a11 - sz * r.a13);
          gvz = (float)(sx * r.a13 + sz * r.a11);
        }
      }
      double after;  // sum_{u > t} gat[u] = dL/dv[t, 0]
      block_scan<true>(gat, cga, slots[2], &after);
      if (live) {
        emit(t, 0, (float)after * lsd[0]);
        emit(t, 3, fr[t * FR + GH] * lsd[3]);
        if (t > 0) emit(t - 1, 1, gvx * lsd[1]), emit(t - 1, 2, gvz * lsd[2]);
        if (!GUIDE && t == n - 1) emit(t, 1, 0.f), emit(t, 2, 0.f);  // the last frame's root velocity moves no joint
      }
    }
    __syncthreads();  // the next forward pass reads row t - 1's root columns
  }

  if (GUIDE) {  // delta = x0' - x0: x0 <- x0', x <- x + c0[t] delta; nothing stored where delta == 0
    for (int t0 = 0; t0 < n; t0 += CV_TILE) {  // through LDS tiles, as the copy was loaded
      const int nt = min(CV_TILE, n - t0);
      for (int i = tid; i < nt * D; i += CV_THREADS) {
        const int c = i / nt, tt = i - c * nt;
        tile[tt * DS + c] = xs[c * n + t0 + tt];
      }
      __syncthreads();
      // CV_BATCH elements per thread and round, every load of a round issued before its first store: x0 and x may
      // alias for all the compiler knows, and one element at a time is a chain of memory latencies
      for (int base = tid; base < nt * D; base += CV_THREADS * CV_BATCH) {
        float nv[CV_BATCH], ov[CV_BATCH], xv[CV_BATCH];
        int64_t e[CV_BATCH];
#pragma unroll
        for (int u = 0; u < CV_BATCH; ++u) {
          const int i = base + u * CV_THREADS;
          if (i < nt * D) {
            const int tt = i / D, c = i - tt * D;
            e[u] = (int64_t)rows[t0 + tt] * F + c;
            nv[u] = tile[tt * DS + c], ov[u] = x0[e[u]], xv[u] = x[e[u]];
          }
        }
#pragma unroll
        for (int u = 0; u < CV_BATCH; ++u) {
          if (base + u * CV_THREADS < nt * D) {
            const float dlt = nv[u] - ov[u];
            if (dlt != 0.f) {
              x0[e[u]] = nv[u];
              x[e[u]] = xv[u] + c0t * dlt;
            }
          }
        }
      }
      __syncthreads();
    }
  } else {
    double carry = 0.0;
    const double total = block_scan<false>(lacc, carry, slots[0], nullptr);
    if (tid == CV_THREADS - 1) loss_out[m] = (float)total;
  }
}

// prims < 0: no scene; else the K = prims primitive records and the joints' (radius, weight) as well
size_t canvas_lds_bytes(int J, int prims = -1) {
  const int D = 3 * J + 1;
  const size_t scene = prims < 0 ? 0 : (size_t)prims * scene::SCENE_REC + 2 * J;
  return ((size_t)2 * D + scene + (size_t)CV_TILE * (D | 1)) * 4;
}

// Every entry below: the checks of an entry of `level`, then the one launch, of the form the terms present ask for.
// g: the clock of a guidance call (x and x0 updated), null for a loss_grad call (loss_out and grad_out written).
int launch_canvas(Level level, const Clock* g, float* x, float* x0, const float* mask, const int32_t* motion_offsets,
                  const int32_t* frame_rows, const float* mean, const float* std, const float* targets, const float* weights,
                  const Terms& o, int M, int F, float* loss_out, float* grad_out, float* workspace, void* stream) {
  if (!x0 || !motion_offsets || !frame_rows || !mean || !std || !workspace || (g ? !x : !loss_out || !grad_out))
    return MDM_ERR_ARG;
  if (!args_ok(level, targets, weights, o, g)) return MDM_ERR_ARG;
  const int J = control_joints(F);
  if (J == 0 || M < 0) return MDM_ERR_ARG;
  if (M == 0) return MDM_OK;
  const Level form = kernel_form(targets, o.K, o.Km, o.terrain);
  const Terms u = terms_of(form, o);
  const Clock c = g ? *g : ONE_EVALUATION;
  const size_t smem = canvas_lds_bytes(J, form == PLAIN ? -1 : u.K);
  if (smem > 60 * 1024) return MDM_ERR_UNSUPPORTED;
  dispatch(g != nullptr, mask != nullptr, form, [&](auto k) {
    using Kn = decltype(k);
    hipLaunchKernelGGL((canvas_control_kernel<Kn::GUIDE, Kn::MASK, Kn::SCENE, Kn::TRACKS, Kn::TERRAIN>), dim3(M), dim3(CV_THREADS),
                       smem, (hipStream_t)stream, x0, x, mask, motion_offsets, frame_rows, mean, std, targets, weights, F, J,
                       c.scale, c.iters, c.coef, c.steps, c.t_dev, c.t_imm, loss_out, grad_out, workspace, u.scene, u.K,
                       u.joint_params, u.tracks, u.Km, u.track_bounds, u.terrain, u.terrain_rec, u.Gx | u.Gz << 16, u.stand);
  });
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // namespace
}  // namespace mdm

namespace ctl = mdm::control;

extern "C" {

int64_t mdm_canvas_control_workspace_floats(int32_t total_frames, int32_t F) {
  const int J = ctl::control_joints(F);
  if (J == 0 || total_frames < 0) return 0;
  return (int64_t)total_frames * (3 * J + 1 + mdm::FR);
}

int mdm_canvas_joint_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                               const float* std, const float* targets, const float* weights, int32_t M, int32_t F,
                               float* loss_out, float* grad_out, float* workspace, void* stream) {
  return mdm::launch_canvas(ctl::PLAIN, nullptr, nullptr, const_cast<float*>(x0), nullptr, motion_offsets, frame_rows, mean, std,
                            targets, weights, ctl::Terms{}, M, F, loss_out, grad_out, workspace, stream);
}

int mdm_canvas_joint_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                              const float* mean, const float* std, const float* targets, const float* weights, int32_t M,
                              int32_t F, float scale, int32_t iters, const float* coef, int32_t steps, const int32_t* t_dev,
                              int32_t t_imm, float* workspace, void* stream) {
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_canvas(ctl::PLAIN, &g, x, x0, mask, motion_offsets, frame_rows, mean, std, targets, weights, ctl::Terms{}, M,
                            F, nullptr, nullptr, workspace, stream);
}

int mdm_canvas_scene_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                               const float* std, const float* targets, const float* weights, const float* scene, int32_t K,
                               const float* joint_params, int32_t M, int32_t F, float* loss_out, float* grad_out,
                               float* workspace, void* stream) {
  const ctl::Terms o = {scene, K, joint_params};
  return mdm::launch_canvas(ctl::SCENE, nullptr, nullptr, const_cast<float*>(x0), nullptr, motion_offsets, frame_rows, mean, std,
                            targets, weights, o, M, F, loss_out, grad_out, workspace, stream);
}

int mdm_canvas_scene_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                              const float* mean, const float* std, const float* targets, const float* weights,
                              const float* scene, int32_t K, const float* joint_params, int32_t M, int32_t F, float scale,
                              int32_t iters, const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm,
                              float* workspace, void* stream) {
  const ctl::Terms o = {scene, K, joint_params};
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_canvas(ctl::SCENE, &g, x, x0, mask, motion_offsets, frame_rows, mean, std, targets, weights, o, M, F, nullptr,
                            nullptr, workspace, stream);
}

int mdm_canvas_tracks_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                                const float* std, const float* targets, const float* weights, const float* scene, int32_t K,
                                const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds, int32_t M,
                                int32_t F, float* loss_out, float* grad_out, float* workspace, void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds};
  return mdm::launch_canvas(ctl::TRACKS, nullptr, nullptr, const_cast<float*>(x0), nullptr, motion_offsets, frame_rows, mean, std,
                            targets, weights, o, M, F, loss_out, grad_out, workspace, stream);
}

int mdm_canvas_tracks_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                               const float* mean, const float* std, const float* targets, const float* weights,
                               const float* scene, int32_t K, const float* joint_params, const float* tracks, int32_t Km,
                               const float* track_bounds, int32_t M, int32_t F, float scale, int32_t iters, const float* coef,
                               int32_t steps, const int32_t* t_dev, int32_t t_imm, float* workspace, void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds};
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_canvas(ctl::TRACKS, &g, x, x0, mask, motion_offsets, frame_rows, mean, std, targets, weights, o, M, F, nullptr,
                            nullptr, workspace, stream);
}

int mdm_canvas_terrain_loss_grad(const float* x0, const int32_t* motion_offsets, const int32_t* frame_rows, const float* mean,
                                 const float* std, const float* targets, const float* weights, const float* scene, int32_t K,
                                 const float* joint_params, const float* tracks, int32_t Km, const float* track_bounds,
                                 const float* terrain, const float* terrain_rec, int32_t Gx, int32_t Gz, const float* stand,
                                 int32_t M, int32_t F, float* loss_out, float* grad_out, float* workspace, void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds, terrain, terrain_rec, Gx, Gz, stand};
  return mdm::launch_canvas(ctl::TERRAIN, nullptr, nullptr, const_cast<float*>(x0), nullptr, motion_offsets, frame_rows, mean,
                            std, targets, weights, o, M, F, loss_out, grad_out, workspace, stream);
}

int mdm_canvas_terrain_guidance(float* x, float* x0, const float* mask, const int32_t* motion_offsets, const int32_t* frame_rows,
                                const float* mean, const float* std, const float* targets, const float* weights,
                                const float* scene, int32_t K, const float* joint_params, const float* tracks, int32_t Km,
                                const float* track_bounds, const float* terrain, const float* terrain_rec, int32_t Gx,
                                int32_t Gz, const float* stand, int32_t M, int32_t F, float scale, int32_t iters,
                                const float* coef, int32_t steps, const int32_t* t_dev, int32_t t_imm, float* workspace,
                                void* stream) {
  const ctl::Terms o = {scene, K, joint_params, tracks, Km, track_bounds, terrain, terrain_rec, Gx, Gz, stand};
  const ctl::Clock g = {scale, iters, coef, steps, t_dev, t_imm};
  return mdm::launch_canvas(ctl::TERRAIN, &g, x, x0, mask, motion_offsets, frame_rows, mean, std, targets, weights, o, M, F,
                            nullptr, nullptr, workspace, stream);
}

}  // extern "C"
