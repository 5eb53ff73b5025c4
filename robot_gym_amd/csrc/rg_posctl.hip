// rg_posctl.hip -- the position-mode controllers of include/rg_posctl.h: the Bezier trot, the body-pose controller and
// the POSITION branch of the motor model, batched over B robots.  Its own translation unit of librg_mpc.so.
//
// Layout: one lane per robot, 64-lane workgroups, float64 throughout.  Parameters, clocks and state rows are
// component-major, so a wave's loads and stores of one row coalesce; angles are written row-major as float32.  Within a
// robot the four legs of the gait are serial (alpha is carried from leg to leg, FR, FL, RR, RL, and from tick to tick:
// bezier_controller.py:118-152, 154-185); the four IK solves after them are independent.
//
// Parity: every step restates the reference operation for operation in IEEE float64.  Floating-point contraction is
// off for this file (the reference rounds after every numpy operation), numpy's deg2rad / rad2deg are one multiply by
// pi/180 / 180/pi, and the phase is one subtraction and one correctly rounded division, so phi and last_time come out
// bit-identical to the reference and every branch on them is taken the same way.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <string>
#include "../../include/rg_posctl.h"
#include "rg_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 64;              // one wave per workgroup
constexpr double kPi = 3.141592653589793;  // np.pi
constexpr double kDeg2Rad = kPi / 180.0;   // np.deg2rad: x * (pi / 180)
constexpr double kRad2Deg = 180.0 / kPi;   // np.rad2deg: x * (180 / pi)

// BezierController.loop (bezier_controller.py:157-160): period floor and phase wrap
constexpr double kPeriodFloor = 0.01;
constexpr double kPhaseWrap = 0.99;
// update_controller_params passes direction 1.0 (:189)
constexpr double kDirection = 1.0;
// calculate_stance (:56-65): amplitude A and half-length of the stance stroke
constexpr double kStanceA = 0.001;
constexpr double kStanceHalfL = 0.05;
constexpr double kStanceW = kPi / (2 * kStanceHalfL);   // np.pi / (2 * half_l), evaluated as the reference does
// calculate_bezier_swing (:67-72): control points of the degree-11 curve (bezier_curve, :51-53)
constexpr int kBezierN = 11;
constexpr double kBezierX[12] = {-0.04, -0.056, -0.06, -0.06, -0.06, 0., 0., 0., 0.06, 0.06, 0.056, 0.04};
constexpr double kBezierZ[12] = {0., 0., 0.0405, 0.0405, 0.0405, 0.0405, 0.0405, 0.0495, 0.0495, 0.0495, 0., 0.};
// solve_bin_factor(11, k) (:48-49): factorial ratios, exact in float64
constexpr double kBinom11[12] = {1., 11., 55., 165., 330., 462., 462., 330., 165., 55., 11., 1.};
// kinematics.check_domain (pose/kinematics.py:59-65): an IK domain outside [-1, 1] becomes +-0.99
constexpr double kDomainClamp = 0.99;

// What the kernels read of the configuration, passed by value.
struct PosCfg {
  double hip, leg, foot;
  double hip_v[12];
  double pose_frames[12];
  double start_frames[12];
  double r[4], foot_angle[4];   // per leg, from the start frames (step_trajectory, :121-122), computed on the host
  double leg_offset[4];
  double step_offset;
  double kp[12], kd[12];
};

struct Vec3 { double x, y, z; };

// kinematics.solve_IK (pose/kinematics.py:68-83) -> theta, alpha, gamma
__device__ inline void solve_ik(const Vec3 c, double hip, double leg, double foot, bool right_side, float *out) {
  double domain = (c.y * c.y + (-c.z) * (-c.z) - hip * hip + (-c.x) * (-c.x) - leg * leg - foot * foot) / (2 * foot * leg);
  if (domain > 1 || domain < -1) domain = domain > 1 ? kDomainClamp : -kDomainClamp;
  const double gamma = atan2(-sqrt(1 - domain * domain), domain);
  double sqrt_value = c.y * c.y + (-c.z) * (-c.z) - hip * hip;
  if (sqrt_value < 0.0) sqrt_value = 0.0;
  const double sq = sqrt(sqrt_value);
  const double alpha = atan2(-c.x, sq) - atan2(foot * sin(gamma), leg + foot * cos(gamma));
  const double hip_val = right_side ? -hip : hip;
  const double theta = -atan2(c.z, c.y) - atan2(sq, hip_val);
  out[0] = (float)theta;
  out[1] = (float)alpha;
  out[2] = (float)gamma;
}

// kinematics.get_RT(orientation, position) = get_Rxyz(roll, pitch, yaw) * translation (pose/kinematics.py:25-46): the
// rotation Rx * Ry * Rz (identity when all three angles are 0) and its product with the translation's last column.
struct RT { double m[3][4]; };

__device__ inline RT make_rt(double roll, double pitch, double yaw, double x0, double y0, double z0) {
  RT o;
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  if (roll != 0 || pitch != 0 || yaw != 0) {
    const double cx = cos(roll), sx = sin(roll), cy = cos(pitch), sy = sin(pitch), cz = cos(yaw), sz = sin(yaw);
    const double Rx[3][3] = {{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}};
    const double Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}};
    const double Rz[3][3] = {{cz, -sz, 0}, {sz, cz, 0}, {0, 0, 1}};
    double A[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) A[i][j] = Rx[i][0] * Ry[0][j] + Rx[i][1] * Ry[1][j] + Rx[i][2] * Ry[2][j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) R[i][j] = A[i][0] * Rz[0][j] + A[i][1] * Rz[1][j] + A[i][2] * Rz[2][j];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) o.m[i][j] = R[i][j];
    o.m[i][3] = R[i][0] * x0 + R[i][1] * y0 + R[i][2] * z0;
  }
  return o;
}

// kinematics.transform (pose/kinematics.py:49-56): RT * [coord, 1]
__device__ inline Vec3 apply_rt(const RT &T, const Vec3 v) {
  return {T.m[0][0] * v.x + T.m[0][1] * v.y + T.m[0][2] * v.z + T.m[0][3],
          T.m[1][0] * v.x + T.m[1][1] * v.y + T.m[1][2] * v.z + T.m[1][3],
          T.m[2][0] * v.x + T.m[2][1] * v.y + T.m[2][2] * v.z + T.m[2][3]};
}

// PoseController.get_action (pose_controller.py:54-99) on foot points feet[leg]: hip vertices moved by the pose, leg
// vectors, the same composition with (-orientation, -position), the four IK solves.  The Bezier get_action
// (bezier_controller.py:191-227) is the zero pose, where both transforms are the identity.
__device__ inline void pose_ik(const PosCfg &c, const Vec3 feet[4], bool zero_pose, double roll, double pitch, double yaw,
                               double x0, double y0, double z0, float *out) {
  RT fwd, inv;
  if (!zero_pose) {
    fwd = make_rt(roll, pitch, yaw, x0, y0, z0);
    inv = make_rt(-roll, -pitch, -yaw, -x0, -y0, -z0);
  }
#pragma unroll
  for (int l = 0; l < 4; l++) {
    Vec3 hv = {c.hip_v[3 * l], c.hip_v[3 * l + 1], c.hip_v[3 * l + 2]};
    if (!zero_pose) hv = apply_rt(fwd, hv);
    Vec3 v = {feet[l].x - hv.x, feet[l].y - hv.y, feet[l].z - hv.z};
    if (!zero_pose) v = apply_rt(inv, v);
    solve_ik(v, c.hip, c.leg, c.foot, (l & 1) == 0 /* FR, RR */, out + 3 * l);
  }
}

// calculate_stance (bezier_controller.py:56-65) with c / s of the angle given
__device__ inline Vec3 stance(double phi_st, double v, double c, double s) {
  const double p = kStanceHalfL * (1 - 2 * phi_st);
  const double av = fabs(v);
  return {c * p * av, -s * p * av, -kStanceA * cos(kStanceW * p)};
}

// calculate_bezier_swing (:67-116) for the long and the rotational term at once: both evaluate the same basis at phi_sw.
// Each term is ((point * binom) * t^k) * (1 - t)^(11 - k), summed in k order as bezier_curve does.
__device__ inline void swing2(double t, double v1, double c1, double s1, double v2, double c2, double s2, Vec3 &o1, Vec3 &o2) {
  const double u = 1 - t;
  double upow[12];
  upow[0] = 1.0;
#pragma unroll
  for (int k = 1; k < 12; k++) upow[k] = upow[k - 1] * u;
  const double a1 = fabs(v1), a2 = fabs(v2);
  const double ac1 = a1 * c1, as1 = a1 * s1, ac2 = a2 * c2, as2 = a2 * s2;
  o1 = {0., 0., 0.};
  o2 = {0., 0., 0.};
  double tk = 1.0;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const double uk = upow[kBezierN - k];
    const double b = kBinom11[k];
    const double X1 = ac1 * kBezierX[k] * kDirection, X2 = ac2 * kBezierX[k] * kDirection;
    const double Y1 = as1 * (-X1), Y2 = as2 * (-X2);
    const double Z1 = a1 * kBezierZ[k], Z2 = a2 * kBezierZ[k];
    o1.x = o1.x + X1 * b * tk * uk; o1.y = o1.y + Y1 * b * tk * uk; o1.z = o1.z + Z1 * b * tk * uk;
    o2.x = o2.x + X2 * b * tk * uk; o2.y = o2.y + Y2 * b * tk * uk; o2.z = o2.z + Z2 * b * tk * uk;
    tk = tk * t;
  }
}

__global__ void __launch_bounds__(kBlock) rg_posctl_bezier_kernel(PosCfg c, int B, double t_all, const double *__restrict__ t_robot,
                                                                  const float *__restrict__ params, double *__restrict__ state,
                                                                  float *__restrict__ angles) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const size_t sB = (size_t)B;
  Vec3 feet[4];
  if (params) {
    const double v = params[b], angle = params[sB + b], w_rot = params[2 * sB + b];
    double period = params[3 * sB + b];
    const double t = t_robot ? t_robot[b] : t_all;
    double phi = state[b], last_time = state[sB + b], alpha = state[2 * sB + b];
    // loop (:154-161)
    if (period <= kPeriodFloor) period = kPeriodFloor;
    if (phi >= kPhaseWrap) last_time = t;
    phi = (t - last_time) / period;
    double cl, sl;
    sincos(angle * kDeg2Rad, &sl, &cl);   // the long term's angle is the same for every leg
    // step_trajectory (:118-152), legs in the order FR, FL, RR, RL: alpha is read before and written after each leg
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double p = phi + c.leg_offset[l];
      if (p >= 1) p = p - 1.;
      const double circle = (w_rot >= 0. ? 90. : 270.) - (c.foot_angle[l] - alpha) * kRad2Deg;
      double cr, sr;
      sincos(circle * kDeg2Rad, &sr, &cr);
      Vec3 lo, ro;
      if (p <= c.step_offset) {
        const double phi_stance = p / c.step_offset;
        lo = stance(phi_stance, v, cl, sl);
        ro = stance(phi_stance, w_rot, cr, sr);
      } else {
        const double phi_swing = (p - c.step_offset) / (1 - c.step_offset);
        swing2(phi_swing, v, cl, sl, w_rot, cr, sr, lo, ro);
      }
      const double mag = atan2(sqrt(ro.x * ro.x + ro.y * ro.y), c.r[l]);
      const bool left = c.start_frames[3 * l + 1] > 0;
      alpha = (left == (ro.x < 0)) ? -mag : mag;
      feet[l] = {c.start_frames[3 * l] + (lo.x + ro.x), c.start_frames[3 * l + 1] + (lo.y + ro.y),
                 c.start_frames[3 * l + 2] + (lo.z + ro.z)};
    }
    state[b] = phi;
    state[sB + b] = last_time;
    state[2 * sB + b] = alpha;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      state[(3 + 3 * k) * sB + b] = feet[k].x;
      state[(4 + 3 * k) * sB + b] = feet[k].y;
      state[(5 + 3 * k) * sB + b] = feet[k].z;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      feet[k] = {state[(3 + 3 * k) * sB + b], state[(4 + 3 * k) * sB + b], state[(5 + 3 * k) * sB + b]};
  }
  float out[12];
  pose_ik(c, feet, true, 0, 0, 0, 0, 0, 0, out);
#pragma unroll
  for (int k = 0; k < 12; k++) angles[(size_t)b * 12 + k] = out[k];
}

__global__ void __launch_bounds__(kBlock) rg_posctl_pose_kernel(PosCfg c, int B, const float *__restrict__ pose, float *__restrict__ angles) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const size_t sB = (size_t)B;
  const double x0 = pose[b], y0 = pose[sB + b], z0 = pose[2 * sB + b];
  const double roll = pose[3 * sB + b], pitch = pose[4 * sB + b], yaw = pose[5 * sB + b];
  Vec3 feet[4];
#pragma unroll
  for (int l = 0; l < 4; l++) feet[l] = {c.pose_frames[3 * l], c.pose_frames[3 * l + 1], c.pose_frames[3 * l + 2]};
  float out[12];
  pose_ik(c, feet, false, roll, pitch, yaw, x0, y0, z0, out);
#pragma unroll
  for (int k = 0; k < 12; k++) angles[(size_t)b * 12 + k] = out[k];
}

// convert_to_torque, POSITION branch (simple_motor.py:122-140) for S sub-steps: one lane per (joint, robot), lane = robot
// so the q / qd loads coalesce; the commanded angle is read once and kept in a register.
__global__ void __launch_bounds__(256) rg_posctl_torque_kernel(PosCfg c, int B, int S, const float *__restrict__ angles,
                                                               const float *__restrict__ q, const float *__restrict__ qd,
                                                               float *__restrict__ tau) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)B * 12) return;
  const int j = (int)(e / B), b = (int)(e - (size_t)j * B);
  const double qs = angles[(size_t)b * 12 + j], kp = c.kp[j], kd = c.kd[j];
  for (int s = 0; s < S; s++) {
    const size_t in = ((size_t)s * 12 + j) * B + b;
    const double t = -1.0 * (kp * ((double)q[in] - qs)) - kd * ((double)qd[in] - 0.0) + 0.0;
    tau[((size_t)s * B + b) * 12 + j] = (float)t;
  }
}

thread_local std::string g_create_err;

}  // namespace

struct rg_posctl_handle {
  PosCfg c;
  int B = 0, device = 0;
  std::string err;
};

namespace {

bool validate(const rg_posctl_config *cfg, int32_t batch, std::string &err) {
  const RealField reals[] = {{"hip", &cfg->hip, 1, kPositive}, {"leg", &cfg->leg, 1, kPositive}, {"foot", &cfg->foot, 1, kPositive},
                             {"hip_v", cfg->hip_v, 12, kFinite}, {"pose_frames", cfg->pose_frames, 12, kFinite},
                             {"start_frames", cfg->start_frames, 12, kFinite}, {"leg_offset", cfg->leg_offset, 4, kFinite},
                             {"step_offset", &cfg->step_offset, 1, kFinite}, {"motor_kp", cfg->motor_kp, 12, kFinite},
                             {"motor_kd", cfg->motor_kd, 12, kFinite}};
  if (!check_abi("config.", cfg->abi_version, RG_POSCTL_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err) ||
      !check_batch(batch, RG_POSCTL_MAX_BATCH, err) || !check_reals("config.", reals, err))
    return false;
  // phi_swing divides by 1 - step_offset and phi_stance by step_offset
  if (!(cfg->step_offset > 0 && cfg->step_offset < 1)) {
    char msg[160];
    snprintf(msg, sizeof(msg), "config.step_offset: %g outside (0, 1)", cfg->step_offset);
    err = msg;
    return false;
  }
  return true;
}

int hip_fail(rg_posctl_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_POSCTL_ERR_HIP, what, e); }
int launch_status(rg_posctl_handle *h, const char *what) { return launch_status(h, RG_POSCTL_ERR_HIP, what); }

}  // namespace

extern "C" {

int32_t rg_posctl_abi_version(void) { return RG_POSCTL_ABI_VERSION; }
int32_t rg_posctl_config_size(void) { return (int32_t)sizeof(rg_posctl_config); }
const char *rg_posctl_last_error(const rg_posctl_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_posctl_create(const rg_posctl_config *cfg, int32_t batch, int32_t device, rg_posctl_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_POSCTL_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!validate(cfg, batch, err)) { g_create_err = err; return RG_POSCTL_ERR_INVALID; }
  // no scope: create runs nothing on the device
  if (const int rc = enter_device(device, nullptr, RG_POSCTL_ERR_NO_DEVICE, RG_POSCTL_ERR_INVALID, RG_POSCTL_ERR_HIP, g_create_err)) return rc;
  rg_posctl_handle *h = new rg_posctl_handle();
  h->B = batch;
  h->device = device;
  PosCfg &c = h->c;
  c.hip = cfg->hip; c.leg = cfg->leg; c.foot = cfg->foot;
  for (int i = 0; i < 12; i++) {
    c.hip_v[i] = cfg->hip_v[i]; c.pose_frames[i] = cfg->pose_frames[i]; c.start_frames[i] = cfg->start_frames[i];
    c.kp[i] = cfg->motor_kp[i]; c.kd[i] = cfg->motor_kd[i];
  }
  for (int l = 0; l < 4; l++) {
    const double x = cfg->start_frames[3 * l], y = cfg->start_frames[3 * l + 1];
    c.r[l] = sqrt(x * x + y * y);   // step_trajectory (bezier_controller.py:121-122)
    c.foot_angle[l] = atan2(y, x);
    c.leg_offset[l] = cfg->leg_offset[l];
  }
  c.step_offset = cfg->step_offset;
  *out = h;
  return RG_POSCTL_OK;
}

void rg_posctl_destroy(rg_posctl_handle *h) { delete h; }

int rg_posctl_bezier_step(rg_posctl_handle *h, double t, const double *t_robot, const float *params, double *state,
                          float *angles, void *stream) {
  if (!h) { g_create_err = "bezier_step: null handle"; return RG_POSCTL_ERR_INVALID; }
  if (!state || !angles) { h->err = "bezier_step: null state or angles"; return RG_POSCTL_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_posctl_bezier_kernel, dim3((h->B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->c, h->B, t,
                     t_robot, params, state, angles);
  return launch_status(h, "rg_posctl_bezier_kernel launch");
}

int rg_posctl_pose(rg_posctl_handle *h, const float *pose, float *angles, void *stream) {
  if (!h) { g_create_err = "pose: null handle"; return RG_POSCTL_ERR_INVALID; }
  if (!pose || !angles) { h->err = "pose: null pose or angles"; return RG_POSCTL_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_posctl_pose_kernel, dim3((h->B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->c, h->B, pose,
                     angles);
  return launch_status(h, "rg_posctl_pose_kernel launch");
}

int rg_posctl_position_to_torque(rg_posctl_handle *h, const float *angles, const float *q, const float *qd, float *tau,
                                 int32_t substeps, void *stream) {
  if (!h) { g_create_err = "position_to_torque: null handle"; return RG_POSCTL_ERR_INVALID; }
  if (!angles || !q || !qd || !tau) { h->err = "position_to_torque: null pointer"; return RG_POSCTL_ERR_INVALID; }
  if (substeps < 1 || substeps > RG_POSCTL_MAX_SUBSTEPS) { h->err = "position_to_torque: substeps outside [1, 1024]"; return RG_POSCTL_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const size_t total = (size_t)h->B * 12;
  hipLaunchKernelGGL(rg_posctl_torque_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->c, h->B,
                     substeps, angles, q, qd, tau);
  return launch_status(h, "rg_posctl_torque_kernel launch");
}

}  // extern "C"
