// rg_srb_contact.hip -- the tick with measured foot contact of include/rg_srb.h (rg_srb_step_contact, rg_srb_contact.h): a
// swinging foot is tested against the ground, stops on it and reports contact.  Its own translation unit of librg_mpc.so,
// so that rg_srb.hip and rg_srb_terrain.hip keep reporting exactly their kernels.
//
// Layout: that of rg_srb_terrain.hip.  The step kernel stands on the shared body of a tick (rg_srb_tick.inc, where the
// cross-lane operations and their invariants are stated) and owns step 1 and the force rule in their second form and the
// touch output: lane = (robot, leg), float64, no LDS.  The ground is asked at the same two points a tick
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

// sum4 and the tick_* functions, the body of a tick: shared with the other three step kernels
#include "rg_srb_tick.inc"

// kCoordBound, the hash chain and Ground, h(x, y; robot) of rg_srb.h: shared with rg_srb_terrain.hip
#include "rg_srb_ground.inc"

// One control tick with measured contact on the ground g (kind 0: the plane).  Its own: step 1 in its measured form (a swung
// foot is tested against the ground and stops on it), the commanded force through the feet that are on the ground only, the
// clearance of rg_srb_terrain_step_kernel, and touch: [4][B] or NULL.
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
  double p[3], qt[4], v[3], w[3], foot[3], q[3], stance, steps, I[9], Iinv[9], eF[3], eT[3];
  const bool running = tick_load_state(state, sB, b, leg, p, qt, v, w, foot, q, stance, steps);
  const double mass = tick_load_body(body, sB, b, I, Iinv);
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
  tick_load_ext(ext, sB, b, eF, eT);
  const double dt = c.dt, wz = mass * -c.g;
  // 2. sub-steps
  for (int s = 0; s < c.substeps; s++) {
    double f[3], F[3], T[3];
    quat_rot(qt, R);
    rot(R, fbody, f);
    tick_wrench(f, foot, p, eF, eT, wz, F, T);
    tick_body(R, I, Iinv, mass, dt, F, T, w, v, p);
    tick_quat(dt, w, qt);
  }
  steps = steps + (double)c.substeps;
  // 3. fall, and the stores
  const int bad = tick_bad(p, qt, v, w, foot);
  const double under = plane ? 0.0 : ground(b, p[0], p[1]);
  const bool store = tick_store(state, c, b, leg, in_batch && running, bad, p[2] - under, p, qt, v, w, foot, stance, steps);
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
