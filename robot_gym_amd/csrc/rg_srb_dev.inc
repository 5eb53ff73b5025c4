// rg_srb_dev.inc -- code of the single-rigid-body simulator shared by rg_srb.hip and rg_episode.hip (the reset on the
// device): the kernel-side configuration, the observation writer (step 4 of include/rg_srb.h), the body of a reset for
// one (robot, leg) lane, and the host-side checks and fills of rg_srb_config (on the helpers of rg_host.h).  Included after
// `#pragma clang fp contract(off)` and rg_mpc_dev.h, inside the including file's anonymous namespace.

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

inline bool obs_ok(const rg_srb_obs_ptrs *o) {
  return o && o->rpy && o->rpy_rate && o->v_world && o->quat && o->q && o->foot_pos && o->jac && o->contact && o->t_robot;
}

inline Obs to_obs(const rg_srb_obs_ptrs *o) { return {o->rpy, o->rpy_rate, o->v_world, o->quat, o->q, o->foot_pos, o->jac, o->contact, o->t_robot}; }

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

// The reset of rg_srb_reset for one (robot, leg) lane: the robot stands at (x, y, height) with heading yaw.  No cross-lane
// operation.
__device__ inline void srb_reset_robot(const DevCfg *kc, const SrbCfg &c, const Obs &o, double *state, int b, int leg, double x, double y,
                                       double yaw, double height) {
  const size_t sB = (size_t)c.B;
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

// rot_zyx_host of rg_mpc.hip: the fixed rotation of a joint origin, Rz Ry Rx of the URDF rpy
inline void rot_zyx_host(const double *rpy, double *R) {
  const double cr = cos(rpy[0]), sr = sin(rpy[0]), cp = cos(rpy[1]), sp = sin(rpy[1]), cy = cos(rpy[2]), sy = sin(rpy[2]);
  const double m[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                       sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                       -sp, cp * sr, cp * cr};
  memcpy(R, m, sizeof(m));
}

// finite, symmetric, positive definite (the checks of rg_mpc_set_body); on success the inverse
inline const char *check_inertia(const double *I, double *inv) {
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

// The checks of rg_srb_create on the configuration and the batch; false: err names the field.  Iinv: the inverse inertia.
inline bool srb_validate(const rg_srb_config *cfg, int32_t batch, double *Iinv, std::string &err) {
  char msg[200];
  const RealField reals[] = {{"mass", &cfg->mass, 1, kPositive}, {"inertia", cfg->inertia, 9, kFinite}, {"gravity", &cfg->gravity, 1, kPositive},
                             {"body_height", &cfg->body_height, 1, kPositive}, {"hip", cfg->hip, 12, kFinite}, {"motor_dir", cfg->motor_dir, 12, kFinite},
                             {"motor_off", cfg->motor_off, 12, kFinite}, {"jxyz", cfg->jxyz, 36, kFinite}, {"jrpy", cfg->jrpy, 36, kFinite},
                             {"jaxis", cfg->jaxis, 36, kFinite}, {"toe_xyz", cfg->toe_xyz, 12, kFinite}, {"toe_com", cfg->toe_com, 12, kFinite},
                             {"base_com", cfg->base_com, 3, kFinite}, {"init_q", cfg->init_q, 12, kFinite}, {"ik_damping", &cfg->ik_damping, 1, kFinite},
                             {"ik_max_step", &cfg->ik_max_step, 1, kPositive}, {"dt_sim", &cfg->dt_sim, 1, kPositive},
                             {"fall_height_scale", &cfg->fall_height_scale, 1, kFinite}, {"fall_tilt", &cfg->fall_tilt, 1, kPositive}};
  if (!check_abi("config.", cfg->abi_version, RG_SRB_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err) ||
      !check_batch(batch, RG_SRB_MAX_BATCH, err) || !check_reals("config.", reals, err))
    return false;
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
  const IntField ints[] = {{"ik_iters", cfg->ik_iters, 1, 64}, {"substeps", cfg->substeps, 1, RG_SRB_MAX_SUBSTEPS}};
  if (!check_ints("config.", ints, err)) return false;
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
inline void srb_fill_kinematics(const rg_srb_config *c, DevCfg *d) {
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

// SrbCfg of a validated rg_srb_config
inline void srb_fill_cfg(const rg_srb_config *cfg, int batch, SrbCfg &c) {
  c.B = batch; c.substeps = cfg->substeps;
  c.dt = cfg->dt_sim; c.g = cfg->gravity; c.body_height = cfg->body_height;
  c.fall_z = cfg->fall_height_scale * cfg->body_height;
  c.cos_tilt = cos(cfg->fall_tilt);
  memcpy(c.hip, cfg->hip, sizeof(c.hip)); memcpy(c.init_q, cfg->init_q, sizeof(c.init_q));
}
