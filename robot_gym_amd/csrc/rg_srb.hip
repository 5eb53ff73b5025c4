// rg_srb.hip -- the batched single-rigid-body simulator of include/rg_srb.h.  Its own translation unit of librg_mpc.so.
//
// Layout: lane = (robot, leg), four lanes per robot, 16 robots per wave, float64 throughout.  The dependent chain of a
// tick is dominated by the four leg IKs of the observation (up to ik_iters forward-kinematics passes of three sincos
// each), which are independent per leg: each lane owns its leg's foot update, force, lever arm and IK.  The wrench is
// summed over the four lanes of a robot with an xor butterfly (1, then 2): every lane forms (x_0 + x_1) + (x_2 + x_3) up
// to commutation, so the four lanes hold bit-identical sums, and the 13 body values are integrated redundantly in all
// four -- the sub-step loop needs no broadcast.  State and observation rows are component-major, so stores coalesce.  No
// LDS.  Every lane is guarded by b < B and by the robot's status at its stores only: nothing returns or branches around
// a cross-lane operation.  The body of the tick -- the loads, the wrench with that sum, the integrator, the finite test and
// the stores -- is rg_srb_tick.inc, one definition under the four step kernels; the kernel here owns step 1 on the plane.
//
// Parity: tests/srb_model.py restates this file and rg_srb_tick.inc operation for operation in float64 numpy.  Floating-point contraction is
// off for the whole file, the controller's leg_fk / leg_ik included (rg_mpc_dev.h is included after the pragma, read-only).
// What remains different: the joint rotations of leg_fk come from sincos_joint (rg_mpc_dev.h), a Cody-Waite reduction with
// fdlibm polynomials written with explicit fma() -- the pragma does not touch those -- against numpy's sin / cos in the model
// (< 1 ulp each; it reaches the q and jac rows only); the reset's sincos, the observation's atan2 / asin, and sqrt / division
// are the device's against libm's.
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

// SrbCfg, Obs, the rotations, write_obs, srb_reset_robot and the configuration checks: shared with rg_episode.hip
#include "rg_srb_dev.inc"

}  // namespace

// the handle and the host-side helpers: shared with rg_srb_terrain.hip
#include "rg_srb_handle.h"

namespace {

constexpr int kBlock = kSrbBlock, kBodyRows = kSrbBodyRows, kResetRows = kSrbResetRows;

// sum4 and the tick_* functions, the body of a tick: shared with the other three step kernels
#include "rg_srb_tick.inc"

// One control tick on the plane.  Its own: the schedule's step 1 (a swinging foot follows its target, a landing foot is put at
// height 0), the commanded force through every stance foot, and the body's height as the clearance of the fall test.
__global__ void __launch_bounds__(kBlock) rg_srb_step_kernel(const DevCfg *__restrict__ kc, SrbCfg c, const double *__restrict__ body,
                                                              double *__restrict__ state, const float *__restrict__ grf,
                                                              const float *__restrict__ foot_target, const int *__restrict__ desired,
                                                              const double *__restrict__ ext, Obs o) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const int leg = t & 3;
  const bool in_batch = (t >> 2) < c.B;
  const int b = in_batch ? (t >> 2) : c.B - 1;   // lanes past the batch compute on the last robot and store nothing
  const size_t sB = (size_t)c.B;
  double p[3], qt[4], v[3], w[3], foot[3], q[3], stance, steps, I[9], Iinv[9], eF[3], eT[3];
  const bool running = tick_load_state(state, sB, b, leg, p, qt, v, w, foot, q, stance, steps);
  const double mass = tick_load_body(body, sB, b, I, Iinv);
  double R[9];
  quat_rot(qt, R);
  // 1. feet
  const bool swing = desired[(size_t)b * 4 + leg] == 0 /* RG_LEG_SWING */;
  double fbody[3] = {0.0, 0.0, 0.0};
  if (swing) {
    const double ft[3] = {foot_target[(size_t)b * 12 + 3 * leg], foot_target[(size_t)b * 12 + 3 * leg + 1], foot_target[(size_t)b * 12 + 3 * leg + 2]};
    double r[3];
    rot(R, ft, r);
    foot[0] = p[0] + r[0]; foot[1] = p[1] + r[1]; foot[2] = p[2] + r[2];
    stance = 0.0;
  } else {
    if (stance == 0.0) { foot[2] = 0.0; stance = 1.0; }
#pragma unroll
    for (int i = 0; i < 3; i++) fbody[i] = -(double)grf[(size_t)b * 12 + 3 * leg + i];
  }
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
  const bool store = tick_store(state, c, b, leg, in_batch && running, bad, p[2], p, qt, v, w, foot, stance, steps);
  // 4. observation
  write_obs(kc, c, o, state, b, leg, store, p, qt, v, w, foot, q, stance, steps, 1);
}

// Reset of n robots: lane = (entry, leg).  rs = staging [kResetRows][n]: robot, x, y, yaw, height.
__global__ void __launch_bounds__(kBlock) rg_srb_reset_kernel(const DevCfg *__restrict__ kc, SrbCfg c, int n, const double *__restrict__ rs,
                                                               double *__restrict__ state, Obs o) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const int leg = t & 3, k = t >> 2;
  if (k >= n) return;   // no cross-lane operation in this kernel
  const size_t sn = (size_t)n;
  srb_reset_robot(kc, c, o, state, (int)rs[k], leg, rs[sn + k], rs[2 * sn + k], rs[3 * sn + k], rs[4 * sn + k]);
}

thread_local std::string g_create_err;

void default_body(rg_srb_handle *h, int b) {
  const size_t B = (size_t)h->B;
  h->body_host[b] = h->cfg.mass;
  for (int i = 0; i < 9; i++) { h->body_host[(1 + i) * B + b] = h->cfg.inertia[i]; h->body_host[(10 + i) * B + b] = h->cfg_Iinv[i]; }
}

}  // namespace

void rg_srb_thread_error(const char *text) { g_create_err = text; }

extern "C" {

int32_t rg_srb_abi_version(void) { return RG_SRB_ABI_VERSION; }
int32_t rg_srb_config_size(void) { return (int32_t)sizeof(rg_srb_config); }
int32_t rg_srb_state_rows(void) { return RG_SRB_STATE_ROWS; }
const char *rg_srb_last_error(const rg_srb_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_srb_create(const rg_srb_config *cfg, int32_t batch, int32_t device, rg_srb_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_SRB_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  double Iinv[9];
  if (!srb_validate(cfg, batch, Iinv, err)) { g_create_err = err; return RG_SRB_ERR_INVALID; }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_SRB_ERR_NO_DEVICE, RG_SRB_ERR_INVALID, RG_SRB_ERR_HIP, g_create_err)) return rc;
  rg_srb_handle *h = new rg_srb_handle();
  h->B = batch;
  h->device = device;
  h->cfg = *cfg;
  memcpy(h->cfg_Iinv, Iinv, sizeof(Iinv));
  srb_fill_cfg(cfg, batch, h->c);
  const size_t B = (size_t)batch;
  h->body_host.resize(kBodyRows * B);
  h->stage_host.resize(kResetRows * B);
  for (int b = 0; b < batch; b++) default_body(h, b);
  DevCfg *kin = new DevCfg();
  srb_fill_kinematics(cfg, kin);
  hipError_t e = hipMalloc((void **)&h->dcfg, sizeof(DevCfg));
  if (e == hipSuccess) e = hipMalloc((void **)&h->body, kBodyRows * B * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&h->stage, kResetRows * B * sizeof(double));
  if (e != hipSuccess) {
    g_create_err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
    delete kin;
    rg_srb_destroy(h);
    return RG_SRB_ERR_ALLOC;
  }
  e = hipMemcpy(h->dcfg, kin, sizeof(DevCfg), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->body, h->body_host.data(), kBodyRows * B * sizeof(double), hipMemcpyHostToDevice);
  delete kin;
  if (e != hipSuccess) {
    g_create_err = std::string("hipMemcpy failed: ") + hipGetErrorString(e);
    rg_srb_destroy(h);
    return RG_SRB_ERR_HIP;
  }
  *out = h;
  return RG_SRB_OK;
}

void rg_srb_destroy(rg_srb_handle *h) {
  if (!h) return;
  {
    DeviceScope dev(h->device);
    if (h->dcfg) (void)hipFree(h->dcfg);
    if (h->body) (void)hipFree(h->body);
    if (h->stage) (void)hipFree(h->stage);
    if (h->reset_mask) (void)hipFree(h->reset_mask);
  }
  delete h;
}

int rg_srb_set_body(rg_srb_handle *h, const int32_t *idx_host, int32_t n, const double *mass, const double *inertia, void *stream) {
  if (!h) { g_create_err = "set_body: null handle"; return RG_SRB_ERR_INVALID; }
  const int B = h->B;
  const size_t sB = (size_t)B;
  if (!mass && !inertia) {
    if (idx_host || n != 0) { h->err = "set_body: no field given (n = 0 and a null index list return every robot to the config)"; return RG_SRB_ERR_INVALID; }
    for (int b = 0; b < B; b++) default_body(h, b);
  } else {
    if (idx_host ? (n < 1 || n > B) : n != B) { h->err = "set_body: n must be the batch without an index list, 1..batch with one"; return RG_SRB_ERR_INVALID; }
    char msg[200];
    auto bad = [&](int k, const char *what) {
      snprintf(msg, sizeof(msg), "set_body: robot %d (entry %d): %s", idx_host ? idx_host[k] : k, k, what);
      h->err = msg;
      return RG_SRB_ERR_INVALID;
    };
    // validate every entry before anything is written: a refused call leaves the rows as they were
    std::vector<double> inv(inertia ? 9 * (size_t)n : 0);
    for (int k = 0; k < n; k++) {
      if (idx_host && (idx_host[k] < 0 || idx_host[k] >= B)) return bad(k, "index out of range");
      if (mass && !(mass[k] > 0 && mass[k] <= 1e300)) return bad(k, "mass must be positive and finite");
      if (inertia) {
        double I[9];
        for (int i = 0; i < 9; i++) I[i] = inertia[(size_t)i * n + k];
        if (const char *what = check_inertia(I, &inv[9 * (size_t)k])) return bad(k, what);
      }
    }
    for (int k = 0; k < n; k++) {
      const int b = idx_host ? idx_host[k] : k;
      if (mass) h->body_host[b] = mass[k];
      if (inertia)
        for (int i = 0; i < 9; i++) { h->body_host[(1 + i) * sB + b] = inertia[(size_t)i * n + k]; h->body_host[(10 + i) * sB + b] = inv[9 * (size_t)k + i]; }
    }
  }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipError_t e = hipMemcpyAsync(h->body, h->body_host.data(), kBodyRows * sB * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  return e != hipSuccess ? hip_fail(h, "set_body copy", e) : RG_SRB_OK;
}

int rg_srb_reset(rg_srb_handle *h, const int32_t *idx_host, int32_t n, const double *xy, const double *yaw, const double *height,
                 double *state, const rg_srb_obs_ptrs *obs, void *stream) {
  if (!h) { g_create_err = "reset: null handle"; return RG_SRB_ERR_INVALID; }
  if (!state || !obs_ok(obs)) { h->err = "reset: null state or observation pointer"; return RG_SRB_ERR_INVALID; }
  const int B = h->B;
  if (n < 1 || n > B) { h->err = "reset: n outside [1, batch]"; return RG_SRB_ERR_INVALID; }
  const size_t sn = (size_t)n;
  char msg[160];
  std::vector<char> taken(idx_host ? (size_t)B : 0, 0);   // two entries for one robot would race on its column
  for (int k = 0; k < n; k++) {
    const int b = idx_host ? idx_host[k] : k;
    if (b < 0 || b >= B) { snprintf(msg, sizeof(msg), "reset: entry %d: robot %d out of range", k, b); h->err = msg; return RG_SRB_ERR_INVALID; }
    if (idx_host) {
      if (taken[b]) { snprintf(msg, sizeof(msg), "reset: entry %d: robot %d given twice", k, b); h->err = msg; return RG_SRB_ERR_INVALID; }
      taken[b] = 1;
    }
    const double x = xy ? xy[k] : 0.0, y = xy ? xy[sn + k] : 0.0, a = yaw ? yaw[k] : 0.0, z = height ? height[k] : h->cfg.body_height;
    if (!(fabs(x) <= 1e300 && fabs(y) <= 1e300 && fabs(a) <= 1e300 && z > 0 && z <= 1e300)) {
      snprintf(msg, sizeof(msg), "reset: entry %d (robot %d): xy and yaw must be finite, height positive and finite", k, b);
      h->err = msg;
      return RG_SRB_ERR_INVALID;
    }
    double *s = h->stage_host.data();
    s[k] = (double)b; s[sn + k] = x; s[2 * sn + k] = y; s[3 * sn + k] = a; s[4 * sn + k] = z;
  }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(h->stage, h->stage_host.data(), kResetRows * sn * sizeof(double), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(h, "reset copy", e);
  const unsigned lanes = 4u * (unsigned)n;
  hipLaunchKernelGGL(rg_srb_reset_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, s, h->dcfg, h->c, n, h->stage, state, to_obs(obs));
  int rc = launch_status(h, "rg_srb_reset_kernel launch");
  if (rc) return rc;
  if (h->ground.kind != 0) {   // a reset on a terrain is the flat reset followed by settle, for the robots just reset
    const int32_t *mask = nullptr;
    if (idx_host || n != B) {
      h->mask_host.assign((size_t)B, 0);
      for (int k = 0; k < n; k++) h->mask_host[idx_host ? idx_host[k] : k] = 1;
      e = hipMemcpyAsync(h->reset_mask, h->mask_host.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s);
      if (e != hipSuccess) return hip_fail(h, "reset mask copy", e);
      mask = h->reset_mask;
    }
    rc = rg_srb_terrain_settle_launch(h, state, mask, obs, s);
    if (rc) return rc;
  }
  e = hipStreamSynchronize(s);   // the staging buffers are reused by the next call
  return e != hipSuccess ? hip_fail(h, "reset", e) : RG_SRB_OK;
}

int rg_srb_step(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *desired_state,
                const double *ext, const rg_srb_obs_ptrs *obs, void *stream) {
  if (!h) { g_create_err = "step: null handle"; return RG_SRB_ERR_INVALID; }
  if (!state || !grf || !foot_target || !desired_state || !obs_ok(obs)) { h->err = "step: null state, controller output or observation pointer"; return RG_SRB_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  if (h->ground.kind != 0) return rg_srb_terrain_step_launch(h, state, grf, foot_target, desired_state, ext, obs, (hipStream_t)stream);
  const unsigned lanes = 4u * (unsigned)h->B;
  hipLaunchKernelGGL(rg_srb_step_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->dcfg, h->c, h->body,
                     state, grf, foot_target, desired_state, ext, to_obs(obs));
  return launch_status(h, "rg_srb_step_kernel launch");
}

}  // extern "C"
