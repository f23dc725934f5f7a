// What the joint-position control over a window (motion_control.hip) and over a canvas
// (motion_control_canvas.hip, §23) share: the fp32 helpers of their kernels, the joint count of a feature width, and the host
// side of their sixteen entries -- the optional terms and the guidance clock as structs, one argument check, the choice of
// the kernel form and the dispatch onto its instantiation.  Each file keeps its kernel, its LDS size and its one launch.
#pragma once
#include "mdm_common.h"
#include "scene_sdf.h"
#include "terrain.h"

#include <cmath>

namespace mdm {
namespace control {

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }

// motion_post.hip's rot_y with q = qy, w: the same operations in the same order (P agrees with mdm_motion_postprocess)
__device__ __forceinline__ void rot_y(float w, float qy, float vx, float vz, float& ox, float& oz) {
  const float uvx = mul(qy, vz), uvz = -mul(qy, vx);
  const float uuvx = mul(qy, uvz), uuvz = -mul(qy, uvx);
  ox = add(vx, mul(2.f, add(mul(w, uvx), uuvx)));
  oz = add(vz, mul(2.f, add(mul(w, uvz), uuvz)));
}

// Partials of rot_y(w = cos a, qy = -sin a) in exact arithmetic:
//   ox = a11 vx + a13 vz, oz = -a13 vx + a11 vz with a11 = 1 - 2 qy^2, a13 = 2 w qy
//   dox/da = 2 (e vz + f vx), doz/da = 2 (f vz - e vx) with e = qy^2 - w^2, f = 2 qy w
struct RotD {
  double a11, a13, e, f;
};
__device__ __forceinline__ RotD rot_d(float cw, float sw) {
  const double w = cw, q = -(double)sw;
  return {1.0 - 2.0 * q * q, 2.0 * w * q, q * q - w * w, 2.0 * q * w};
}

// joints of a feature row of width F = 12 J - 1 (HumanML3D layout); 0: no such row
inline int control_joints(int F) { return (F + 1) % 12 == 0 && F >= 11 ? (F + 1) / 12 : 0; }

static_assert(scene::MAX_TRACKS == MDM_SCENE_MAX_TRACKS, "scene_sdf.h and mdm_hip.h disagree");
static_assert(terrain::MAX_GRID == MDM_TERRAIN_MAX_GRID && terrain::TERRAIN_REC == MDM_TERRAIN_REC, "terrain.h and mdm_hip.h disagree");

// The optional terms of the loss, named as the ABI names them; an entry whose signature lacks some leaves them zero.
struct Terms {
  const float* scene;  // §24: K primitive records and the joints' (radius, weight)
  int K;
  const float* joint_params;
  const float* tracks;  // §25: Km records a frame behind the frames' bounding balls
  int Km;
  const float* track_bounds;
  const float* terrain;  // §29: a Gz x Gx height grid, its record, the stand weights
  const float* terrain_rec;
  int Gx, Gz;
  const float* stand;
};
// The clock of a guidance call (a loss_grad call has none).
struct Clock {
  float scale;
  int iters;
  const float* coef;
  int steps;
  const int* t_dev;
  int t_imm;
};
constexpr Clock ONE_EVALUATION = {0.f, 1, nullptr, 1, nullptr, 0};  // what the kernels get from a loss_grad call

// An entry's level: how much of Terms its signature carries.  A kernel's form: which of the terms its instantiation reads
// (SCENE, TRACKS and TERRAIN each with the ones before it).
enum Level { PLAIN, SCENE, TRACKS, TERRAIN };

// The checks every entry of `level` makes of targets, weights, terms and clock (null: a loss_grad call).
inline bool args_ok(Level level, const float* targets, const float* weights, const Terms& o, const Clock* g) {
  if (level == PLAIN ? !targets || !weights : !targets != !weights || !o.joint_params) return false;
  if (level >= SCENE && (o.K < 0 || o.K > MDM_SCENE_MAX_PRIMS || (o.K > 0 && !o.scene))) return false;
  if (level >= TRACKS && !scene::tracks_ok(o.tracks, o.Km, o.track_bounds)) return false;  // Km == 0 too: the alignment
  if (level >= TERRAIN && o.terrain && !terrain::terrain_ok(o.terrain, o.terrain_rec, o.Gx, o.Gz, o.stand)) return false;
  if (!g) return true;
  if (!g->coef || g->iters < 1 || g->iters > MDM_CONTROL_MAX_ITERS || !std::isfinite(g->scale)) return false;
  return g->steps > 0 && (g->t_dev || (g->t_imm >= 0 && g->t_imm < g->steps));
}

// The form that runs: the cheapest instantiation that reads every term present.
constexpr Level kernel_form(bool targets, int K, int Km, bool terrain) {
  return terrain ? TERRAIN : Km > 0 ? TRACKS : K == 0 && targets ? PLAIN : SCENE;
}
// (targets, K, Km, terrain), every combination: a wrong pick would run, only slower
static_assert(kernel_form(true, 0, 0, false) == PLAIN && kernel_form(false, 0, 0, false) == SCENE, "");
static_assert(kernel_form(true, 3, 0, false) == SCENE && kernel_form(false, 3, 0, false) == SCENE, "");
static_assert(kernel_form(true, 0, 2, false) == TRACKS && kernel_form(false, 0, 2, false) == TRACKS, "");
static_assert(kernel_form(true, 3, 2, false) == TRACKS && kernel_form(false, 3, 2, false) == TRACKS, "");
static_assert(kernel_form(true, 0, 0, true) == TERRAIN && kernel_form(false, 0, 0, true) == TERRAIN, "");
static_assert(kernel_form(true, 3, 0, true) == TERRAIN && kernel_form(false, 3, 0, true) == TERRAIN, "");
static_assert(kernel_form(true, 0, 2, true) == TERRAIN && kernel_form(false, 0, 2, true) == TERRAIN, "");
static_assert(kernel_form(true, 3, 2, true) == TERRAIN && kernel_form(false, 3, 2, true) == TERRAIN, "");

// The terms as the kernel of `form` gets them: what it does not read is null / 0, whatever the caller passed.
inline Terms terms_of(Level form, Terms o) {
  if (form < TERRAIN) o.terrain = o.terrain_rec = o.stand = nullptr, o.Gx = o.Gz = 0;
  if (form < TRACKS) o.tracks = o.track_bounds = nullptr, o.Km = 0;
  if (form < SCENE) o.scene = o.joint_params = nullptr, o.K = 0;
  return o;
}

// The template arguments of a control kernel.  dispatch() calls fn once with the Flags of (guide, mask, form): one of the
// twelve instantiations there are -- a loss_grad call reads no mask, each form brings the forms under it.
template <bool G, bool M, Level FORM>
struct Flags {
  static constexpr bool GUIDE = G, MASK = M, SCENE = FORM >= control::SCENE, TRACKS = FORM >= control::TRACKS,
                        TERRAIN = FORM >= control::TERRAIN;
};
template <Level FORM, class Fn>
void dispatch_form(bool guide, bool mask, Fn& fn) {
  if (!guide)
    fn(Flags<false, false, FORM>());
  else if (mask)
    fn(Flags<true, true, FORM>());
  else
    fn(Flags<true, false, FORM>());
}
template <class Fn>
void dispatch(bool guide, bool mask, Level form, Fn fn) {
  switch (form) {
    case PLAIN: return dispatch_form<PLAIN>(guide, mask, fn);
    case SCENE: return dispatch_form<SCENE>(guide, mask, fn);
    case TRACKS: return dispatch_form<TRACKS>(guide, mask, fn);
    case TERRAIN: return dispatch_form<TERRAIN>(guide, mask, fn);
  }
}

}  // namespace control
}  // namespace mdm
