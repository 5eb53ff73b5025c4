// rg_srb_friction.hip -- the tick with Coulomb friction at the stance feet of include/rg_srb.h (rg_srb_step_friction,
// rg_srb_friction.h) and the per-episode draw of the coefficient (rg_srb_friction_draw).  Its own translation unit of
// librg_mpc.so, so that rg_srb.hip, rg_srb_terrain.hip and rg_srb_contact.hip keep the code they have.
//
// Layout: that of rg_srb_contact.hip.  The step kernel stands on the shared body of a tick (rg_srb_tick.inc, where the
// cross-lane operations and their invariants are stated) and owns step 1 chosen by `measured` (wave-uniform), the force rule in
// its third form, the foot's slide and the touch and slip outputs: lane = (robot, leg), float64, no LDS.  The friction rule is
// written with selects, so a robot that grips (mu +inf, NaN or negative) runs the operations of the tick without friction on
// the values it had.  The ground is asked at the two points of the contact tick and, for a foot that slid, a third time under
// the foot; one kernel serves all three ground kinds (kind is wave-uniform, the plane gives the literal 0).
//
// Parity: tests/friction_model.py restates the rule in float64 numpy.  Floating-point contraction is off for the whole file,
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

// kCoordBound, the stream (rg_stream_dev.inc) and Ground, h(x, y; robot) of rg_srb.h: shared with rg_srb_terrain.hip
#include "rg_srb_ground.inc"

static_assert(purposes_in_block(3, RG_SRB_FRICTION_PURPOSE_MU), "rg_stream.h: the friction unit owns purposes 48..63");

// One control tick with friction on the ground g (kind 0: the plane).  Its own: step 1 of rg_srb_contact_step_kernel or of
// rg_srb_terrain_step_kernel, chosen by `measured`; the force rule of rg_srb_friction.h inside the sub-step loop, between the
// force's rotation and the wrench, and the foot's slide between the body update and the quaternion update; a third ground query
// under a foot that slid; and touch, slip: [4][B] or NULL.  The wrench and the body update of its sub-step are typed out here,
// for speed (below); the loads, the quaternion update, the finite test and the stores are the shared ones.
__global__ void __launch_bounds__(kBlock) rg_srb_friction_step_kernel(const DevCfg *__restrict__ kc, SrbCfg c, rg_srb_ground g,
                                                                       const double *__restrict__ body, double *__restrict__ state,
                                                                       const float *__restrict__ grf, const float *__restrict__ foot_target,
                                                                       const int *__restrict__ leg_state, int measured,
                                                                       const double *__restrict__ ext, Obs o, const double *__restrict__ mu_row,
                                                                       double slip_gain, double slip_speed_max, int *__restrict__ touch,
                                                                       double *__restrict__ slip) {
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
  const double mu = mu_row[b];
  const bool grips = !(mu >= 0.0 && mu < INFINITY);   // +inf, NaN, negative: the tick without friction
  double R[9];
  quat_rot(qt, R);
  // 1. feet: one ground evaluation per lane, at the swing target (measured) or under the foot
  const int ls = leg_state[(size_t)b * 4 + leg];
  const bool swung = ls == 0 /* RG_LEG_SWING */ || (measured && ls == 3 /* RG_LEG_LOSE_CONTACT */);
  const bool tested = swung && measured;   // a swung foot is tested against the ground in the measured form only
  const double ft[3] = {foot_target[(size_t)b * 12 + 3 * leg], foot_target[(size_t)b * 12 + 3 * leg + 1], foot_target[(size_t)b * 12 + 3 * leg + 2]};
  double r0[3];
  rot(R, ft, r0);
  const double cx = p[0] + r0[0], cy = p[1] + r0[1], cz = p[2] + r0[2];
  const double gx = tested ? cx : foot[0], gy = tested ? cy : foot[1];
  const double gh = plane ? 0.0 : ground(b, gx, gy);
  const bool touches = tested && cz <= gh;
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
  const bool rubs = !grips && stance == 1.0;   // the lanes the friction rule applies to
  tick_load_ext(ext, sB, b, eF, eT);
  const double dt = c.dt, wz = mass * -c.g;
  double slid = 0.0;
  // 2. sub-steps
  for (int s = 0; s < c.substeps; s++) {
    double f[3], F[3], T[3];
    quat_rot(qt, R);
    rot(R, fbody, f);
    // friction: the ground does not pull, and holds at most mu times the normal force.  A NaN fails the comparison and slips.
    const double fn = fmax(f[2], 0.0);
    const double t2 = f[0] * f[0] + f[1] * f[1], lim = mu * fn;
    const bool slips = rubs && !(t2 <= lim * lim);
    const double tn = sqrt(t2);
    const double sc = lim / tn, ux = f[0] / tn, uy = f[1] / tn;
    const double d = dt * fmin(slip_gain * (tn - lim), slip_speed_max);
    f[0] = slips ? f[0] * sc : f[0];
    f[1] = slips ? f[1] * sc : f[1];
    f[2] = rubs ? fn : f[2];
    // tick_wrench and tick_body of rg_srb_tick.inc, inline in this one kernel: on the calls its mu = 0.3 tick measured above the
    // parent's range at batch 4096 on the plane, on this text every figure lies below it (profiles/srb_tick_identity.txt)
    double r[3], tq[3];
    r[0] = foot[0] - p[0]; r[1] = foot[1] - p[1]; r[2] = foot[2] - p[2];
    tq[0] = r[1] * f[2] - r[2] * f[1];
    tq[1] = r[2] * f[0] - r[0] * f[2];
    tq[2] = r[0] * f[1] - r[1] * f[0];
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
    // the slipping foot moves against the friction force
    foot[0] = slips ? foot[0] - ux * d : foot[0];
    foot[1] = slips ? foot[1] - uy * d : foot[1];
    slid = slips ? slid + d : slid;
    tick_quat(dt, w, qt);
  }
  steps = steps + (double)c.substeps;
  // a foot that slid stands on the ground where it is now (no cross-lane operation inside the branch)
  if (!plane && slid > 0.0) foot[2] = ground(b, foot[0], foot[1]);
  // 3. fall, and the stores
  const int bad = tick_bad(p, qt, v, w, foot);
  const double under = plane ? 0.0 : ground(b, p[0], p[1]);
  const bool store = tick_store(state, c, b, leg, in_batch && running, bad, p[2] - under, p, qt, v, w, foot, stance, steps);
  // touch and slip are this tick's: a robot that is frozen, or keeps its last state, touched nothing and slid nowhere
  if (touch && in_batch) touch[(size_t)leg * sB + b] = store && touches ? 1 : 0;
  if (slip && in_batch) slip[(size_t)leg * sB + b] = store ? slid : 0.0;
  // 4. observation
  write_obs(kc, c, o, state, b, leg, store, p, qt, v, w, foot, q, stance, steps, 1);
}

// mu[b] = lo + (hi - lo) * u(seed; key, draws, RG_SRB_FRICTION_PURPOSE_MU, 0) for the robots of the mask: one lane per robot
__global__ void __launch_bounds__(kBlock) rg_srb_friction_draw_kernel(int B, const int *__restrict__ mask, const double *__restrict__ key,
                                                                       const double *__restrict__ draws, unsigned long long seed, double lo, double hi,
                                                                       double *__restrict__ mu) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;   // no cross-lane operation in this kernel
  if (mask[b] == 0) return;
  const unsigned long long hd = mix_word(mix_word(seed, word_of(key[b])), word_of(draws[b]));
  mu[b] = lo + (hi - lo) * unit53(mix_word(mix_word(hd, RG_SRB_FRICTION_PURPOSE_MU), 0));
}

// the text of a refusal goes to the handle, or, for a call that was given none, to the thread
int refuse(rg_srb_handle *h, const std::string &text) {
  if (h) h->err = text;
  else rg_srb_thread_error(text.c_str());
  return RG_SRB_ERR_INVALID;
}

}  // namespace

extern "C" {

// Both entries check their arguments BEFORE the handle, so that a bad argument is named on any machine.

int rg_srb_step_friction(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *leg_state,
                         int32_t measured, const double *ext, const rg_srb_obs_ptrs *obs, const double *mu, double slip_gain,
                         double slip_speed_max, int32_t *touch, double *slip, void *stream) {
  const char *missing = !state ? "state" : !grf ? "grf" : !foot_target ? "foot_target" : !leg_state ? "leg_state" : !obs ? "obs" : !mu ? "mu" : nullptr;
  if (missing) return refuse(h, std::string("step_friction: null ") + missing);
  if (!obs_ok(obs)) return refuse(h, "step_friction: null pointer in obs");
  if (measured != 0 && measured != 1) return refuse(h, "step_friction: measured must be 0 or 1");
  if (!(std::isfinite(slip_gain) && slip_gain >= 0.0)) return refuse(h, "step_friction: slip_gain must be finite and >= 0");
  if (!(std::isfinite(slip_speed_max) && slip_speed_max >= 0.0)) return refuse(h, "step_friction: slip_speed_max must be finite and >= 0");
  if (!h) return refuse(h, "step_friction: null handle");
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const unsigned lanes = 4u * (unsigned)h->B;
  hipLaunchKernelGGL(rg_srb_friction_step_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->dcfg, h->c,
                     h->ground, h->body, state, grf, foot_target, leg_state, (int)measured, ext, to_obs(obs), mu, slip_gain, slip_speed_max, touch,
                     slip);
  return launch_status(h, "rg_srb_friction_step_kernel launch");
}

int rg_srb_friction_draw(rg_srb_handle *h, const int32_t *mask, const double *key, const double *draws, uint64_t seed, double lo,
                         double hi, double *mu, void *stream) {
  const char *missing = !mask ? "mask" : !key ? "key" : !draws ? "draws" : !mu ? "mu" : nullptr;
  if (missing) return refuse(h, std::string("friction_draw: null ") + missing);
  if (!(std::isfinite(lo) && lo >= 0.0)) return refuse(h, "friction_draw: lo must be finite and >= 0");
  if (!(std::isfinite(hi) && hi >= lo)) return refuse(h, "friction_draw: hi must be finite and >= lo");
  if (!h) return refuse(h, "friction_draw: null handle");
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_srb_friction_draw_kernel, dim3(((unsigned)h->B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->B, mask,
                     key, draws, (unsigned long long)seed, lo, hi, mu);
  return launch_status(h, "rg_srb_friction_draw_kernel launch");
}

}  // extern "C"
