// rg_srb_contact.hip -- the tick with measured foot contact of include/rg_srb.h (rg_srb_step_contact, rg_srb_contact.h): a
// swinging foot is tested against the ground, stops on it and reports contact.  Its own translation unit of librg_mpc.so,
// so that rg_srb.hip and rg_srb_terrain.hip keep reporting exactly their kernels.
//
// Layout: that of rg_srb_terrain.hip.  The step kernel is rg_srb_terrain_step_kernel with step 1 and the force rule in
// their second form: lane = (robot, leg), float64, no LDS, every lane guarded at its stores only, lanes past the batch
// computing on the last robot, no branch around a cross-lane operation.  The ground is asked at the same two points a tick
// (the foot -- the swing target or the landing foot, chosen by a select -- and the fall test), and one kernel serves all
// three ground kinds: kind is wave-uniform, and the plane gives the literal 0 without evaluating anything.
//
// Parity: tests/contact_model.py restates the rule in float64 numpy.  Floating-point contraction is off for the whole file,
// the controller's leg_fk / leg_ik included.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rg_srb.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_mpc_dev.h"

namespace {

#include "rg_srb_dev.inc"

}  // namespace

#include "rg_srb_handle.h"

namespace {

constexpr int kBlock = kSrbBlock;

// sum over the four lanes of a robot: (x_0 + x_1) + (x_2 + x_3) in every lane
__device__ __forceinline__ double sum4(double x) {
  x = x + __shfl_xor(x, 1);
  return x + __shfl_xor(x, 2);
}

// kCoordBound, the hash chain and Ground, h(x, y; robot) of rg_srb.h: shared with rg_srb_terrain.hip
#include "rg_srb_ground.inc"

// One control tick with measured contact on the ground g (kind 0: the plane).  rg_srb_terrain_step_kernel with step 1 and
// the force rule replaced, and otherwise its text, statement for statement.  touch: [4][B] or NULL.
__global__ void __launch_bounds__(kBlock) rg_srb_contact_step_kernel(const DevCfg *__restrict__ kc, SrbCfg c, rg_srb_ground g,
                                                                      const double *__restrict__ body, double *__restrict__ state,
                                                                      const float *__restrict__ grf, const float *__restrict__ foot_target,
                                                                      const int *__restrict__ leg_state, const double *__restrict__ ext, Obs o,
                                                                      int *__restrict__ touch) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const Ground ground{g};
  const bool plane = g.kind == RG_SRB_TERRAIN_FLAT;   // wave-uniform
  const int leg = t & 3;
  const bool in_batch = (t >> 2) < c.B;
  const int b = in_batch ? (t >> 2) : c.B - 1;   // lanes past the batch compute on the last robot and store nothing
  const size_t sB = (size_t)c.B;
  double p[3], qt[4], v[3], w[3], foot[3], q[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    p[i] = state[(RG_SRB_ROW_P + i) * sB + b];
    v[i] = state[(RG_SRB_ROW_V + i) * sB + b];
    w[i] = state[(RG_SRB_ROW_W + i) * sB + b];
    foot[i] = state[(RG_SRB_ROW_FOOT + 3 * leg + i) * sB + b];
    q[i] = state[(RG_SRB_ROW_Q + 3 * leg + i) * sB + b];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) qt[i] = state[(RG_SRB_ROW_QUAT + i) * sB + b];
  double stance = state[(RG_SRB_ROW_STANCE + leg) * sB + b];
  double steps = state[RG_SRB_ROW_STEPS * sB + b];
  const bool running = state[RG_SRB_ROW_STATUS * sB + b] == 0.0;
  const double mass = body[b];
  double I[9], Iinv[9];
#pragma unroll
  for (int i = 0; i < 9; i++) { I[i] = body[(1 + i) * sB + b]; Iinv[i] = body[(10 + i) * sB + b]; }
  double R[9];
  quat_rot(qt, R);
  // 1. feet: one ground evaluation per lane, at the swing target or under the foot
  const int ls = leg_state[(size_t)b * 4 + leg];
  const bool swung = ls == 0 /* RG_LEG_SWING */ || ls == 3 /* RG_LEG_LOSE_CONTACT */;
  const double ft[3] = {foot_target[(size_t)b * 12 + 3 * leg], foot_target[(size_t)b * 12 + 3 * leg + 1], foot_target[(size_t)b * 12 + 3 * leg + 2]};
  double r0[3];
  rot(R, ft, r0);
  const double cx = p[0] + r0[0], cy = p[1] + r0[1], cz = p[2] + r0[2];
  const double gx = swung ? cx : foot[0], gy = swung ? cy : foot[1];
  const double gh = plane ? 0.0 : ground(b, gx, gy);
  const bool touches = swung && cz <= gh;
  if (swung) {
    foot[0] = cx; foot[1] = cy; foot[2] = touches ? gh : cz;
    stance = touches ? 1.0 : 0.0;
  } else if (stance == 0.0) {
    foot[2] = gh; stance = 1.0;
  }
  // the ground pushes only through a foot that is on it
  double fbody[3];
#pragma unroll
  for (int i = 0; i < 3; i++) fbody[i] = stance == 1.0 ? -(double)grf[(size_t)b * 12 + 3 * leg + i] : 0.0;
  double eF[3] = {0.0, 0.0, 0.0}, eT[3] = {0.0, 0.0, 0.0};
  if (ext) {
#pragma unroll
    for (int i = 0; i < 3; i++) { eF[i] = ext[i * sB + b]; eT[i] = ext[(3 + i) * sB + b]; }
  }
  const double dt = c.dt, wz = mass * -c.g;
  // 2. sub-steps
  for (int s = 0; s < c.substeps; s++) {
    double f[3], r[3], tq[3];
    quat_rot(qt, R);
    rot(R, fbody, f);
    r[0] = foot[0] - p[0]; r[1] = foot[1] - p[1]; r[2] = foot[2] - p[2];
    tq[0] = r[1] * f[2] - r[2] * f[1];
    tq[1] = r[2] * f[0] - r[0] * f[2];
    tq[2] = r[0] * f[1] - r[1] * f[0];
    double F[3], T[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { F[i] = sum4(f[i]); T[i] = sum4(tq[i]); }
    F[0] = F[0] + eF[0]; F[1] = F[1] + eF[1]; F[2] = F[2] + wz + eF[2];
    T[0] = T[0] + eT[0]; T[1] = T[1] + eT[1]; T[2] = T[2] + eT[2];
    double tb[3], wb[3], Iw[3], rhs[3], ab[3], aw[3];
    rot_t(R, T, tb);
    rot_t(R, w, wb);
    rot(I, wb, Iw);
    rhs[0] = tb[0] - (wb[1] * Iw[2] - wb[2] * Iw[1]);
    rhs[1] = tb[1] - (wb[2] * Iw[0] - wb[0] * Iw[2]);
    rhs[2] = tb[2] - (wb[0] * Iw[1] - wb[1] * Iw[0]);
    rot(Iinv, rhs, ab);
    rot(R, ab, aw);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      w[i] = w[i] + dt * aw[i];
      v[i] = v[i] + dt * F[i] / mass;
      p[i] = p[i] + dt * v[i];
    }
    const double ax = 0.5 * dt * w[0], ay = 0.5 * dt * w[1], az = 0.5 * dt * w[2];
    const double dx = ax * qt[3] + ay * qt[2] - az * qt[1];
    const double dy = ay * qt[3] + az * qt[0] - ax * qt[2];
    const double dz = az * qt[3] + ax * qt[1] - ay * qt[0];
    const double dw = -(ax * qt[0]) - ay * qt[1] - az * qt[2];
    qt[0] = qt[0] + dx; qt[1] = qt[1] + dy; qt[2] = qt[2] + dz; qt[3] = qt[3] + dw;
    const double nrm = sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3]);
    qt[0] = qt[0] / nrm; qt[1] = qt[1] / nrm; qt[2] = qt[2] / nrm; qt[3] = qt[3] / nrm;
  }
  steps = steps + (double)c.substeps;
  // 3. fall
  int bad = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) bad |= !isfinite(p[i]) || !isfinite(v[i]) || !isfinite(w[i]) || !isfinite(foot[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) bad |= !isfinite(qt[i]);
  bad |= __shfl_xor(bad, 1);
  bad |= __shfl_xor(bad, 2);
  const double under = plane ? 0.0 : ground(b, p[0], p[1]);
  const bool fallen = bad || p[2] - under < c.fall_z || (1 - 2 * (qt[0] * qt[0] + qt[1] * qt[1])) < c.cos_tilt;
  const bool live = in_batch && running;
  if (live && leg == 0) state[RG_SRB_ROW_STATUS * sB + b] = fallen ? 1.0 : 0.0;
  const bool store = live && !bad;
  if (store) {
#pragma unroll
    for (int i = 0; i < 3; i++) state[(RG_SRB_ROW_FOOT + 3 * leg + i) * sB + b] = foot[i];
    state[(RG_SRB_ROW_STANCE + leg) * sB + b] = stance;
    if (leg == 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        state[(RG_SRB_ROW_P + i) * sB + b] = p[i];
        state[(RG_SRB_ROW_V + i) * sB + b] = v[i];
        state[(RG_SRB_ROW_W + i) * sB + b] = w[i];
      }
#pragma unroll
      for (int i = 0; i < 4; i++) state[(RG_SRB_ROW_QUAT + i) * sB + b] = qt[i];
      state[RG_SRB_ROW_STEPS * sB + b] = steps;
    }
  }
  // touch is this tick's: a robot that is frozen, or keeps its last state, touched nothing
  if (touch && in_batch) touch[(size_t)leg * sB + b] = store && touches ? 1 : 0;
  // 4. observation
  write_obs(kc, c, o, state, b, leg, store, p, qt, v, w, foot, q, stance, steps, 1);
}

}  // namespace

extern "C" {

int rg_srb_step_contact(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *leg_state,
                        const double *ext, const rg_srb_obs_ptrs *obs, int32_t *touch, void *stream) {
  if (!h) { rg_srb_thread_error("step_contact: null handle"); return RG_SRB_ERR_INVALID; }
  const char *missing = !state ? "state" : !grf ? "grf" : !foot_target ? "foot_target" : !leg_state ? "leg_state" : !obs ? "obs" : nullptr;
  if (missing) { h->err = std::string("step_contact: null ") + missing; return RG_SRB_ERR_INVALID; }
  if (!obs_ok(obs)) { h->err = "step_contact: null pointer in obs"; return RG_SRB_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const unsigned lanes = 4u * (unsigned)h->B;
  hipLaunchKernelGGL(rg_srb_contact_step_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->dcfg, h->c,
                     h->ground, h->body, state, grf, foot_target, leg_state, ext, to_obs(obs), touch);
  return launch_status(h, "rg_srb_contact_step_kernel launch");
}

}  // extern "C"
