// rg_srb.hip -- the batched single-rigid-body simulator of include/rg_srb.h.  Its own translation unit of librg_mpc.so.
//
// Layout: lane = (robot, leg), four lanes per robot, 16 robots per wave, float64 throughout.  The dependent chain of a
// tick is dominated by the four leg IKs of the observation (up to ik_iters forward-kinematics passes of three sincos
// each), which are independent per leg: each lane owns its leg's foot update, force, lever arm and IK.  The wrench is
// summed over the four lanes of a robot with an xor butterfly (1, then 2): every lane forms (x_0 + x_1) + (x_2 + x_3) up
// to commutation, so the four lanes hold bit-identical sums, and the 13 body values are integrated redundantly in all
// four -- the sub-step loop needs no broadcast.  State and observation rows are component-major, so stores coalesce.  No
// LDS.  Every lane is guarded by b < B and by the robot's status at its stores only: nothing returns or branches around
// a cross-lane operation.
//
// Parity: tests/srb_model.py restates this file operation for operation in float64 numpy.  Floating-point contraction is
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

#pragma clang fp contract(off)

#include "rg_mpc_dev.h"

namespace {

constexpr int kBlock = 256;            // 64 robots per workgroup
constexpr int kBodyRows = 19;          // per-robot true body [kBodyRows][B]: mass, I[9], I^-1[9]
constexpr int kResetRows = 5;          // reset staging [kResetRows][B]: robot, x, y, yaw, height
constexpr double kIkDone = 1e-18;      // squared foot error (1e-9 m) below which the reset stops repeating the IK

struct SrbCfg {
  int B, substeps;
  double dt, g, body_height, fall_z, cos_tilt;
  double hip[12], init_q[12];
};

struct Obs {
  float *rpy, *rpy_rate, *v_world, *quat, *q, *foot_pos, *jac;
  int *contact;
  double *t_robot;
};

// rotation of the quaternion (x, y, z, w), row-major
__device__ __forceinline__ void quat_rot(const double *qt, double *R) {
  const double x = qt[0], y = qt[1], z = qt[2], w = qt[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
// R v and R' v
__device__ __forceinline__ void rot(const double *R, const double *v, double *o) {
  const double a = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  const double b = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  const double c = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
  o[0] = a; o[1] = b; o[2] = c;
}
__device__ __forceinline__ void rot_t(const double *R, const double *v, double *o) {
  const double a = R[0] * v[0] + R[3] * v[1] + R[6] * v[2];
  const double b = R[1] * v[0] + R[4] * v[1] + R[7] * v[2];
  const double c = R[2] * v[0] + R[5] * v[1] + R[8] * v[2];
  o[0] = a; o[1] = b; o[2] = c;
}
// arr[3 * leg + i] of a 12-entry kernel argument without indexing it by a lane's value
__device__ __forceinline__ void pick3(const double *arr, int leg, double *o) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double a = leg & 1 ? arr[3 + i] : arr[i], b = leg & 1 ? arr[9 + i] : arr[6 + i];
    o[i] = leg & 2 ? b : a;
  }
}
// sum over the four lanes of a robot: (x_0 + x_1) + (x_2 + x_3) in every lane
__device__ __forceinline__ double sum4(double x) {
  x = x + __shfl_xor(x, 1);
  return x + __shfl_xor(x, 2);
}

// Step 4 of rg_srb.h for one (robot, leg) lane: the leg's IK and rows, and (leg 0) the body rows.  `passes` IK passes at
// most, repeated while the foot error is 1e-9 m or more (1 in a tick; RG_SRB_RESET_IK_PASSES at a reset).
__device__ inline void write_obs(const DevCfg *kc, const SrbCfg &c, const Obs &o, double *state, int b, int leg, bool store,
                                 const double *p, const double *qt, const double *v, const double *w, const double *foot,
                                 const double *q0, double stance, double steps, int passes) {
  const size_t sB = (size_t)c.B;
  double R[9], d[3] = {foot[0] - p[0], foot[1] - p[1], foot[2] - p[2]}, fb[3], q[3] = {q0[0], q0[1], q0[2]}, pf[3], J[9];
  quat_rot(qt, R);
  rot_t(R, d, fb);
  for (int k = 0; k < passes; k++) {
    leg_ik(kc, leg, fb, q, q);
    leg_fk(kc, leg, q, pf, J);
    const double e0 = fb[0] - pf[0], e1 = fb[1] - pf[1], e2 = fb[2] - pf[2];
    if (e0 * e0 + e1 * e1 + e2 * e2 < kIkDone) break;
  }
  if (!store) return;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    state[(RG_SRB_ROW_Q + 3 * leg + i) * sB + b] = q[i];
    o.q[(3 * leg + i) * sB + b] = (float)q[i];
    o.foot_pos[(3 * leg + i) * sB + b] = (float)fb[i];
  }
#pragma unroll
  for (int i = 0; i < 9; i++) o.jac[(9 * leg + i) * sB + b] = (float)J[i];
  o.contact[leg * sB + b] = (int)stance;
  if (leg == 0) {
    double wb[3];
    rot_t(R, w, wb);
    double sp = R[6];
    sp = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);
    o.rpy[b] = (float)atan2(R[7], R[8]);
    o.rpy[sB + b] = (float)(-asin(sp));
    o.rpy[2 * sB + b] = (float)atan2(R[3], R[0]);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      o.rpy_rate[i * sB + b] = (float)wb[i];
      o.v_world[i * sB + b] = (float)v[i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) o.quat[i * sB + b] = (float)qt[i];
    o.t_robot[b] = steps * c.dt;
  }
}

__global__ void __launch_bounds__(kBlock) rg_srb_step_kernel(const DevCfg *__restrict__ kc, SrbCfg c, const double *__restrict__ body,
                                                              double *__restrict__ state, const float *__restrict__ grf,
                                                              const float *__restrict__ foot_target, const int *__restrict__ desired,
                                                              const double *__restrict__ ext, Obs o) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
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
  const bool fallen = bad || p[2] < c.fall_z || (1 - 2 * (qt[0] * qt[0] + qt[1] * qt[1])) < c.cos_tilt;
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
  // 4. observation
  write_obs(kc, c, o, state, b, leg, store, p, qt, v, w, foot, q, stance, steps, 1);
}

// Reset of n robots: lane = (entry, leg).  rs = staging [kResetRows][n]: robot, x, y, yaw, height.
__global__ void __launch_bounds__(kBlock) rg_srb_reset_kernel(const DevCfg *__restrict__ kc, SrbCfg c, int n, const double *__restrict__ rs,
                                                               double *__restrict__ state, Obs o) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const int leg = t & 3, k = t >> 2;
  if (k >= n) return;   // no cross-lane operation in this kernel
  const size_t sB = (size_t)c.B, sn = (size_t)n;
  const int b = (int)rs[k];
  const double x = rs[sn + k], y = rs[2 * sn + k], yaw = rs[3 * sn + k], height = rs[4 * sn + k];
  const double p[3] = {x, y, height}, zero[3] = {0.0, 0.0, 0.0};
  double sn_y, cs_y;
  sincos(0.5 * yaw, &sn_y, &cs_y);
  const double qt[4] = {0.0, 0.0, sn_y, cs_y};
  double R[9], h[3], hip[3], q0[3];
  pick3(c.hip, leg, hip);
  pick3(c.init_q, leg, q0);
  quat_rot(qt, R);
  rot(R, hip, h);
  const double foot[3] = {h[0] + x, h[1] + y, 0.0};
#pragma unroll
  for (int i = 0; i < 3; i++) state[(RG_SRB_ROW_FOOT + 3 * leg + i) * sB + b] = foot[i];
  state[(RG_SRB_ROW_STANCE + leg) * sB + b] = 1.0;
  if (leg == 0) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      state[(RG_SRB_ROW_P + i) * sB + b] = p[i];
      state[(RG_SRB_ROW_V + i) * sB + b] = 0.0;
      state[(RG_SRB_ROW_W + i) * sB + b] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) state[(RG_SRB_ROW_QUAT + i) * sB + b] = qt[i];
    state[RG_SRB_ROW_STEPS * sB + b] = 0.0;
    state[RG_SRB_ROW_STATUS * sB + b] = 0.0;
  }
  write_obs(kc, c, o, state, b, leg, true, p, qt, zero, zero, foot, q0, 1.0, 0.0, RG_SRB_RESET_IK_PASSES);
}

// The calling thread's current device is restored on scope exit (rg_mpc.h conventions).
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess && prev >= 0; }
  }
  ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

thread_local std::string g_create_err;

// rot_zyx_host of rg_mpc.hip: the fixed rotation of a joint origin, Rz Ry Rx of the URDF rpy
void rot_zyx_host(const double *rpy, double *R) {
  const double cr = cos(rpy[0]), sr = sin(rpy[0]), cp = cos(rpy[1]), sp = sin(rpy[1]), cy = cos(rpy[2]), sy = sin(rpy[2]);
  const double m[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                       sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                       -sp, cp * sr, cp * cr};
  memcpy(R, m, sizeof(m));
}

// finite, symmetric, positive definite (the checks of rg_mpc_set_body); on success the inverse
const char *check_inertia(const double *I, double *inv) {
  double mx = 0.0;
  for (int i = 0; i < 9; i++) { if (!(fabs(I[i]) <= 1e300)) return "inertia must be finite"; mx = fmax(mx, fabs(I[i])); }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < i; j++) if (fabs(I[3 * i + j] - I[3 * j + i]) > 1e-12 * mx) return "inertia must be symmetric";
  const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
  const double m2 = I[0] * I[4] - I[1] * I[3], det = I[0] * c00 + I[1] * c01 + I[2] * c02;
  if (!(I[0] > 0 && m2 > 0 && det > 0)) return "inertia must be positive definite";
  const double d = 1.0 / det;
  inv[0] = c00 * d; inv[1] = (I[2] * I[7] - I[1] * I[8]) * d; inv[2] = (I[1] * I[5] - I[2] * I[4]) * d;
  inv[3] = c01 * d; inv[4] = (I[0] * I[8] - I[2] * I[6]) * d; inv[5] = (I[2] * I[3] - I[0] * I[5]) * d;
  inv[6] = c02 * d; inv[7] = (I[1] * I[6] - I[0] * I[7]) * d; inv[8] = (I[0] * I[4] - I[1] * I[3]) * d;
  return nullptr;
}

}  // namespace

struct rg_srb_handle {
  SrbCfg c;
  rg_srb_config cfg;
  double cfg_Iinv[9];
  int B = 0, device = 0;
  DevCfg *dcfg = nullptr;     // the kinematic fields of the controller's DevCfg, for leg_fk / leg_ik
  double *body = nullptr;     // [kBodyRows][B]
  double *stage = nullptr;    // [kResetRows][B]
  std::vector<double> body_host, stage_host;
  std::string err;
};

namespace {

bool validate(const rg_srb_config *cfg, int32_t batch, double *Iinv, std::string &err) {
  char msg[200];
  if (cfg->abi_version != RG_SRB_ABI_VERSION) {
    snprintf(msg, sizeof(msg), "config.abi_version: %d, this library is version %d", cfg->abi_version, RG_SRB_ABI_VERSION);
    err = msg;
    return false;
  }
  if (cfg->reserved0 != 0) { err = "config.reserved0: must be 0"; return false; }
  if (batch < 1 || batch > RG_SRB_MAX_BATCH) {
    snprintf(msg, sizeof(msg), "batch: %d outside [1, %d]", batch, RG_SRB_MAX_BATCH);
    err = msg;
    return false;
  }
  struct F { const char *name; const double *p; int n; bool positive; };
  const F fields[] = {{"mass", &cfg->mass, 1, true}, {"inertia", cfg->inertia, 9, false}, {"gravity", &cfg->gravity, 1, true},
                      {"body_height", &cfg->body_height, 1, true}, {"hip", cfg->hip, 12, false}, {"motor_dir", cfg->motor_dir, 12, false},
                      {"motor_off", cfg->motor_off, 12, false}, {"jxyz", cfg->jxyz, 36, false}, {"jrpy", cfg->jrpy, 36, false},
                      {"jaxis", cfg->jaxis, 36, false}, {"toe_xyz", cfg->toe_xyz, 12, false}, {"toe_com", cfg->toe_com, 12, false},
                      {"base_com", cfg->base_com, 3, false}, {"init_q", cfg->init_q, 12, false}, {"ik_damping", &cfg->ik_damping, 1, false},
                      {"ik_max_step", &cfg->ik_max_step, 1, true}, {"dt_sim", &cfg->dt_sim, 1, true},
                      {"fall_height_scale", &cfg->fall_height_scale, 1, false}, {"fall_tilt", &cfg->fall_tilt, 1, true}};
  for (const F &f : fields)
    for (int i = 0; i < f.n; i++) {
      const double v = f.p[i];
      if (!std::isfinite(v) || (f.positive && !(v > 0))) {
        if (f.n > 1) snprintf(msg, sizeof(msg), "config.%s[%d]: %g is not finite", f.name, i, v);
        else snprintf(msg, sizeof(msg), "config.%s: %g must be finite%s", f.name, v, f.positive ? " and > 0" : "");
        err = msg;
        return false;
      }
    }
  if (const char *what = check_inertia(cfg->inertia, Iinv)) { err = std::string("config.inertia: ") + what; return false; }
  for (int i = 0; i < 12; i++) {
    if (!(cfg->motor_dir[i] == 1.0 || cfg->motor_dir[i] == -1.0)) {
      snprintf(msg, sizeof(msg), "config.motor_dir[%d]: %g must be +-1", i, cfg->motor_dir[i]);
      err = msg;
      return false;
    }
    const double *a = &cfg->jaxis[3 * i];
    if (!(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] > 0)) {
      snprintf(msg, sizeof(msg), "config.jaxis[%d]: zero joint axis", 3 * i);
      err = msg;
      return false;
    }
  }
  if (cfg->ik_iters < 1 || cfg->ik_iters > 64) { snprintf(msg, sizeof(msg), "config.ik_iters: %d outside [1, 64]", cfg->ik_iters); err = msg; return false; }
  if (cfg->substeps < 1 || cfg->substeps > RG_SRB_MAX_SUBSTEPS) {
    snprintf(msg, sizeof(msg), "config.substeps: %d outside [1, %d]", cfg->substeps, RG_SRB_MAX_SUBSTEPS);
    err = msg;
    return false;
  }
  if (cfg->ik_damping < 0) { snprintf(msg, sizeof(msg), "config.ik_damping: %g must be >= 0", cfg->ik_damping); err = msg; return false; }
  if (!(cfg->fall_height_scale >= 0 && cfg->fall_height_scale < 1)) {
    snprintf(msg, sizeof(msg), "config.fall_height_scale: %g outside [0, 1)", cfg->fall_height_scale);
    err = msg;
    return false;
  }
  if (!(cfg->fall_tilt <= 3.141592653589793)) { snprintf(msg, sizeof(msg), "config.fall_tilt: %g outside (0, pi]", cfg->fall_tilt); err = msg; return false; }
  return true;
}

// The kinematic fields of DevCfg as build_devcfg of rg_mpc.hip fills them; leg_fk / leg_ik read nothing else.
void fill_kinematics(const rg_srb_config *c, DevCfg *d) {
  memset(d, 0, sizeof(*d));
  d->ik_iters = c->ik_iters;
  memcpy(d->mdir, c->motor_dir, sizeof(d->mdir)); memcpy(d->moff, c->motor_off, sizeof(d->moff));
  memcpy(d->jxyz, c->jxyz, sizeof(d->jxyz));
  for (int lj = 0; lj < 12; lj++) {
    rot_zyx_host(&c->jrpy[3 * lj], &d->jRf[9 * lj]);
    const double *a = &c->jaxis[3 * lj];
    const double nrm = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int k = 0; k < 3; k++) d->jaxis[3 * lj + k] = nrm > 0 ? a[k] / nrm : 0.0;
  }
  for (int i = 0; i < 12; i++) d->tip[i] = c->toe_xyz[i] + c->toe_com[i];
  memcpy(d->base_com, c->base_com, sizeof(d->base_com));
  d->ik_damping = c->ik_damping; d->ik_max_step = c->ik_max_step;
}

void default_body(rg_srb_handle *h, int b) {
  const size_t B = (size_t)h->B;
  h->body_host[b] = h->cfg.mass;
  for (int i = 0; i < 9; i++) { h->body_host[(1 + i) * B + b] = h->cfg.inertia[i]; h->body_host[(10 + i) * B + b] = h->cfg_Iinv[i]; }
}

int hip_fail(rg_srb_handle *h, const char *what, hipError_t e) {
  h->err = std::string(what) + ": " + hipGetErrorString(e);
  return RG_SRB_ERR_HIP;
}

int launch_status(rg_srb_handle *h, const char *what) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(h, what, e) : RG_SRB_OK;
}

bool obs_ok(const rg_srb_obs_ptrs *o) {
  return o && o->rpy && o->rpy_rate && o->v_world && o->quat && o->q && o->foot_pos && o->jac && o->contact && o->t_robot;
}

Obs to_obs(const rg_srb_obs_ptrs *o) { return {o->rpy, o->rpy_rate, o->v_world, o->quat, o->q, o->foot_pos, o->jac, o->contact, o->t_robot}; }

}  // namespace

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
  if (!validate(cfg, batch, Iinv, err)) { g_create_err = err; return RG_SRB_ERR_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_err = "no HIP device available"; return RG_SRB_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { g_create_err = "device index out of range"; return RG_SRB_ERR_INVALID; }
  DeviceScope dev(device);
  if (dev.err != hipSuccess) { g_create_err = std::string("hipSetDevice failed: ") + hipGetErrorString(dev.err); return RG_SRB_ERR_HIP; }
  rg_srb_handle *h = new rg_srb_handle();
  h->B = batch;
  h->device = device;
  h->cfg = *cfg;
  memcpy(h->cfg_Iinv, Iinv, sizeof(Iinv));
  SrbCfg &c = h->c;
  c.B = batch; c.substeps = cfg->substeps;
  c.dt = cfg->dt_sim; c.g = cfg->gravity; c.body_height = cfg->body_height;
  c.fall_z = cfg->fall_height_scale * cfg->body_height;
  c.cos_tilt = cos(cfg->fall_tilt);
  memcpy(c.hip, cfg->hip, sizeof(c.hip)); memcpy(c.init_q, cfg->init_q, sizeof(c.init_q));
  const size_t B = (size_t)batch;
  h->body_host.resize(kBodyRows * B);
  h->stage_host.resize(kResetRows * B);
  for (int b = 0; b < batch; b++) default_body(h, b);
  DevCfg *kin = new DevCfg();
  fill_kinematics(cfg, kin);
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
  const int rc = launch_status(h, "rg_srb_reset_kernel launch");
  if (rc) return rc;
  e = hipStreamSynchronize(s);   // the staging buffers are reused by the next call
  return e != hipSuccess ? hip_fail(h, "reset", e) : RG_SRB_OK;
}

int rg_srb_step(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *desired_state,
                const double *ext, const rg_srb_obs_ptrs *obs, void *stream) {
  if (!h) { g_create_err = "step: null handle"; return RG_SRB_ERR_INVALID; }
  if (!state || !grf || !foot_target || !desired_state || !obs_ok(obs)) { h->err = "step: null state, controller output or observation pointer"; return RG_SRB_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const unsigned lanes = 4u * (unsigned)h->B;
  hipLaunchKernelGGL(rg_srb_step_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->dcfg, h->c, h->body,
                     state, grf, foot_target, desired_state, ext, to_obs(obs));
  return launch_status(h, "rg_srb_step_kernel launch");
}

}  // extern "C"
