// rg_est.hip -- the state estimator error model of include/rg_est.h: IMU tilt, gyro, velocity, encoder and foot-switch errors
// between the simulator's exact observation and the controller, per robot and per episode.  Its own translation unit of
// librg_mpc.so; of the controller it includes the leg kinematics (leg_fk of rg_mpc_dev.h), of the simulator the rotation of a
// quaternion and the checks and fills of an rg_srb_config (rg_srb_dev.inc).
//
// Layout.  estimate: a workgroup of 256 lanes is 64 consecutive robots (lane % 64) times 4 legs (lane / 64), so a wave is one
// leg of 64 consecutive robots: the leg is uniform over a wave, every load and store is row * B + b over consecutive b, and the
// body rows (orientation, gyro, velocity, clock, ticks) are the work of whole waves (leg 0), not of every fourth lane.  The tick
// row is read by every lane of a robot and written by its leg-0 lane: every lane reads, the workgroup meets at a barrier, then
// the stores begin.  A run row has one reader and one writer, the leg's own lane.  A robot's lanes share a workgroup by
// construction (the robot is the low part of the lane index); no lane leaves before the barrier.
// reset: one lane per robot.
// No LDS, no atomics, no cross-lane operation.  The amplitudes are read from the kernel argument with constant indices only
// (unrolled loops); the tests on them are uniform over the grid, so a skipped term costs no divergence.  The leg chains are read
// from device memory (the DevCfg the create uploaded), where indexing by the leg is an address, not a register file.
//
// The stream is rg_stream_dev.inc's.
// Parity: tests/est_model.py restates every output in numpy; bit for bit but for the rows that go through sqrt, atan2, asin and
// the kinematics' sincos (quat, rpy, foot_pos, jac).  Floating-point contraction is off for the whole file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rg_est.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_mpc_dev.h"

namespace {

#include "rg_srb_dev.inc"

}  // namespace

struct rg_est_handle {
  rg_est_config cfg;
  int B = 0, device = 0;
  DevCfg *kin = nullptr;   // the kinematic fields of the controller's DevCfg, for leg_fk
  std::string err;
};

namespace {

constexpr int kBlock = 256;
constexpr int kRobots = 64;                          // robots of a workgroup of estimate: one wave per leg
constexpr double kRunMax = (double)RG_EST_RUN_MAX;

struct EstCfg {
  int B, rise;
  unsigned long long seed;
  double imu_bias[3], imu_sigma[3], gyro_bias[3], gyro_sigma[3], vel_bias[3], vel_sigma[3];
  double enc_bias, enc_sigma, enc_quantum, miss, ghost;
};

#include "rg_stream_dev.inc"   // the chain over the four words (key, draw, purpose, index)

static_assert(purposes_in_block(2, RG_EST_PURPOSE_BIAS, RG_EST_PURPOSE_NOISE, RG_EST_PURPOSE_MISS, RG_EST_PURPOSE_GHOST),
              "the estimator model's purposes are block 2 of rg_stream.h's registry, 32..47");

// x + bias(w, row) + noise(s, k, row), each term skipped where its amplitude is 0; hb, hn = the chain with the purpose
__device__ __forceinline__ double perturb(double x, double w, double s, unsigned long long hb, unsigned long long hn, unsigned long long k, int row) {
  if (w != 0.0) x = x + w * (2.0 * unit53(mix_word(hb, (unsigned long long)row)) - 1.0);
  if (s != 0.0) x = x + s * unit_noise(hn, index_word(k, row));
  return x;
}

// three rows of a sensor that adds bias and noise row by row (gyro, velocity)
__device__ __forceinline__ void three_rows(const float *__restrict__ in, float *__restrict__ out, size_t sB, int b, const double *w, const double *s,
                                           unsigned long long hb, unsigned long long hn, unsigned long long k, int row0) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float v = in[i * sB + b];
    out[i * sB + b] = w[i] == 0.0 && s[i] == 0.0 ? v : (float)perturb((double)v, w[i], s[i], hb, hn, k, row0 + i);
  }
}

__global__ void __launch_bounds__(kBlock) rg_est_reset_kernel(int B, const int *__restrict__ mask, double *__restrict__ st) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B || mask[b] == 0) return;
  const size_t sB = (size_t)B;
  st[RG_EST_ROW_DRAWS * sB + b] = st[RG_EST_ROW_DRAWS * sB + b] + 1.0;
  st[RG_EST_ROW_TICKS * sB + b] = 0.0;
#pragma unroll
  for (int l = 0; l < 4; l++) st[(RG_EST_ROW_RUN + l) * sB + b] = kRunMax;
}

__global__ void __launch_bounds__(kBlock) rg_est_estimate_kernel(EstCfg c, const DevCfg *__restrict__ kin, double *__restrict__ st, Obs t, Obs e) {
  const int b = blockIdx.x * kRobots + (int)(threadIdx.x % kRobots), leg = (int)(threadIdx.x / kRobots);
  const size_t sB = (size_t)c.B;
  const bool live = b < c.B;
  double ticks = 0.0, draws = 0.0, key = 0.0;
  if (live) { ticks = st[RG_EST_ROW_TICKS * sB + b]; draws = st[RG_EST_ROW_DRAWS * sB + b]; key = st[RG_EST_ROW_KEY * sB + b]; }
  __syncthreads();   // every lane of a robot has read ticks before its leg-0 lane writes it
  if (!live) return;
  const unsigned long long k = bounded(ticks, kTickBound);
  const unsigned long long hd = mix_word(mix_word(c.seed, word_of(key)), word_of(draws - 1.0));
  const unsigned long long hb = mix_word(hd, RG_EST_PURPOSE_BIAS), hn = mix_word(hd, RG_EST_PURPOSE_NOISE);

  // the leg's encoders, and the kinematics they imply
  if (c.enc_bias == 0.0 && c.enc_sigma == 0.0 && c.enc_quantum == 0.0) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t at = (size_t)(3 * leg + i) * sB + b;
      e.q[at] = t.q[at];
      e.foot_pos[at] = t.foot_pos[at];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const size_t at = (size_t)(9 * leg + i) * sB + b;
      e.jac[at] = t.jac[at];
    }
  } else {
    double qe[3], pf[3], J[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t at = (size_t)(3 * leg + i) * sB + b;
      double x = perturb((double)t.q[at], c.enc_bias, c.enc_sigma, hb, hn, k, RG_EST_OBS_ROW_Q + 3 * leg + i);
      if (c.enc_quantum != 0.0) x = c.enc_quantum * rint(x / c.enc_quantum);
      const float xf = (float)x;
      e.q[at] = xf;
      qe[i] = (double)xf;
    }
    leg_fk(kin, leg, qe, pf, J);
#pragma unroll
    for (int i = 0; i < 3; i++) e.foot_pos[(size_t)(3 * leg + i) * sB + b] = (float)pf[i];
#pragma unroll
    for (int i = 0; i < 9; i++) e.jac[(size_t)(9 * leg + i) * sB + b] = (float)J[i];
  }

  // the leg's foot switch
  {
    const size_t at = (size_t)leg * sB + b, rat = (size_t)(RG_EST_ROW_RUN + leg) * sB + b;
    const int raw = t.contact[at];
    const bool on = raw != 0;
    unsigned long long run = bounded(st[rat], kRunMax);
    run = on ? (run + 1 < (unsigned long long)RG_EST_RUN_MAX ? run + 1 : (unsigned long long)RG_EST_RUN_MAX) : 0ull;
    st[rat] = (double)run;
    if (c.rise == 0 && c.miss == 0.0 && c.ghost == 0.0) {
      e.contact[at] = raw;
    } else {
      const bool seen = on && run > (unsigned long long)c.rise;
      const unsigned long long ix = index_word(k, RG_EST_OBS_ROW_CONTACT + leg);
      int out = seen ? 1 : 0;
      if (seen && c.miss != 0.0 && unit53(mix_word(mix_word(hd, RG_EST_PURPOSE_MISS), ix)) < c.miss) out = 0;
      if (!on && c.ghost != 0.0 && unit53(mix_word(mix_word(hd, RG_EST_PURPOSE_GHOST), ix)) < c.ghost) out = 1;
      e.contact[at] = out;
    }
  }

  if (leg != 0) return;   // uniform over the wave
  three_rows(t.rpy_rate, e.rpy_rate, sB, b, c.gyro_bias, c.gyro_sigma, hb, hn, k, RG_EST_OBS_ROW_RPY_RATE);
  three_rows(t.v_world, e.v_world, sB, b, c.vel_bias, c.vel_sigma, hb, hn, k, RG_EST_OBS_ROW_V_WORLD);
  bool tilt = false;
#pragma unroll
  for (int i = 0; i < 3; i++) tilt = tilt || c.imu_bias[i] != 0.0 || c.imu_sigma[i] != 0.0;
  if (!tilt) {
#pragma unroll
    for (int i = 0; i < 3; i++) e.rpy[i * sB + b] = t.rpy[i * sB + b];
#pragma unroll
    for (int i = 0; i < 4; i++) e.quat[i * sB + b] = t.quat[i * sB + b];
  } else {
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = perturb(0.0, c.imu_bias[i], c.imu_sigma[i], hb, hn, k, RG_EST_OBS_ROW_RPY + i) / 2.0;
    const double qx = (double)t.quat[b], qy = (double)t.quat[sB + b], qz = (double)t.quat[2 * sB + b], qw = (double)t.quat[3 * sB + b];
    double qn[4], R[9];
    qn[0] = ((qw * d[0] + qx) + qy * d[2]) - qz * d[1];
    qn[1] = ((qw * d[1] - qx * d[2]) + qy) + qz * d[0];
    qn[2] = ((qw * d[2] + qx * d[1]) - qy * d[0]) + qz;
    qn[3] = ((qw - qx * d[0]) - qy * d[1]) - qz * d[2];
    const double s = sqrt(((qn[0] * qn[0] + qn[1] * qn[1]) + qn[2] * qn[2]) + qn[3] * qn[3]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      qn[i] = qn[i] / s;
      e.quat[i * sB + b] = (float)qn[i];
    }
    quat_rot(qn, R);
    double sp = R[6];
    sp = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);
    e.rpy[b] = (float)atan2(R[7], R[8]);
    e.rpy[sB + b] = (float)(-asin(sp));
    e.rpy[2 * sB + b] = (float)atan2(R[3], R[0]);
  }
  e.t_robot[b] = t.t_robot[b];
  st[RG_EST_ROW_TICKS * sB + b] = (double)(k + 1);
}

thread_local std::string g_create_err;

bool validate(const rg_est_config *cfg, std::string &err) {
  if (!check_abi("config.", cfg->abi_version, RG_EST_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err) ||
      !check_reserved("config.", "reserved1", cfg->reserved1, err))
    return false;
  const IntField ints[] = {{"contact_rise_ticks", cfg->contact_rise_ticks, 0, RG_EST_MAX_RISE}};
  if (!check_ints("config.", ints, err)) return false;
  // the per-axis amplitudes one by one, so that the text names the axis and the rule
  const struct { const char *name; const double *p; } triples[] = {
      {"imu_bias_half_width", cfg->imu_bias_half_width}, {"imu_noise_sigma", cfg->imu_noise_sigma}, {"gyro_bias_half_width", cfg->gyro_bias_half_width},
      {"gyro_noise_sigma", cfg->gyro_noise_sigma}, {"velocity_bias_half_width", cfg->velocity_bias_half_width}, {"velocity_noise_sigma", cfg->velocity_noise_sigma}};
  for (const auto &tr : triples)
    for (int i = 0; i < 3; i++)
      if (!(std::isfinite(tr.p[i]) && tr.p[i] >= 0.0)) {
        char msg[200];
        snprintf(msg, sizeof(msg), "config.%s[%d]: %g must be finite and >= 0", tr.name, i, tr.p[i]);
        err = msg;
        return false;
      }
  const RealField reals[] = {{"encoder_bias_half_width", &cfg->encoder_bias_half_width, 1, kNonNegative}, {"encoder_noise_sigma", &cfg->encoder_noise_sigma, 1, kNonNegative},
                             {"encoder_quantum", &cfg->encoder_quantum, 1, kNonNegative}, {"contact_miss_probability", &cfg->contact_miss_probability, 1, kUnit},
                             {"contact_ghost_probability", &cfg->contact_ghost_probability, 1, kUnit}};
  return check_reals("config.", reals, err);
}

EstCfg dev_cfg(const rg_est_handle *h) {
  const rg_est_config &f = h->cfg;
  EstCfg c{};
  c.B = h->B; c.rise = f.contact_rise_ticks; c.seed = (unsigned long long)f.seed;
  for (int i = 0; i < 3; i++) {
    c.imu_bias[i] = f.imu_bias_half_width[i]; c.imu_sigma[i] = f.imu_noise_sigma[i];
    c.gyro_bias[i] = f.gyro_bias_half_width[i]; c.gyro_sigma[i] = f.gyro_noise_sigma[i];
    c.vel_bias[i] = f.velocity_bias_half_width[i]; c.vel_sigma[i] = f.velocity_noise_sigma[i];
  }
  c.enc_bias = f.encoder_bias_half_width; c.enc_sigma = f.encoder_noise_sigma; c.enc_quantum = f.encoder_quantum;
  c.miss = f.contact_miss_probability; c.ghost = f.contact_ghost_probability;
  return c;
}

// no pointer of the estimate may be one of the true observation
bool disjoint(const rg_srb_obs_ptrs *a, const rg_srb_obs_ptrs *b) {
  const void *pa[] = {a->rpy, a->rpy_rate, a->v_world, a->quat, a->q, a->foot_pos, a->jac, a->contact, a->t_robot};
  const void *pb[] = {b->rpy, b->rpy_rate, b->v_world, b->quat, b->q, b->foot_pos, b->jac, b->contact, b->t_robot};
  for (const void *x : pa)
    for (const void *y : pb)
      if (x == y) return false;
  return true;
}

int hip_fail(rg_est_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_EST_ERR_HIP, what, e); }
int no_device(rg_est_handle *h) { return no_device(h, RG_EST_ERR_NO_DEVICE, "RG_EST"); }
int launch_status(rg_est_handle *h, const char *what) { return launch_status(h, RG_EST_ERR_HIP, what); }
int null_arg(rg_est_handle *h, const char *call, const char *name) { return null_arg(h, RG_EST_ERR_INVALID, call, name); }

}  // namespace

extern "C" {

int32_t rg_est_abi_version(void) { return RG_EST_ABI_VERSION; }
int32_t rg_est_config_size(void) { return (int32_t)sizeof(rg_est_config); }
int32_t rg_est_state_rows(void) { return RG_EST_ROWS; }
const char *rg_est_last_error(const rg_est_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_est_create(const rg_est_config *cfg, const rg_srb_config *scfg, int32_t batch, int32_t device, rg_est_handle **out) {
  if (!cfg || !scfg || !out) { g_create_err = "create: null config or out"; return RG_EST_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  double Iinv[9];
  if (!check_batch(batch, RG_EST_MAX_BATCH, err) || !validate(cfg, err)) { g_create_err = err; return RG_EST_ERR_INVALID; }
  if (!srb_validate(scfg, batch, Iinv, err)) { g_create_err = "srb " + err; return RG_EST_ERR_INVALID; }
  rg_est_handle *h = new rg_est_handle();
  h->cfg = *cfg;
  h->B = batch;
  h->device = device;
  if (device == RG_EST_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_EST_OK;
  }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_EST_ERR_NO_DEVICE, RG_EST_ERR_INVALID, RG_EST_ERR_HIP, g_create_err)) { delete h; return rc; }
  DevCfg *kin = new DevCfg();
  srb_fill_kinematics(scfg, kin);
  hipError_t e = hipMalloc((void **)&h->kin, sizeof(DevCfg));
  if (e != hipSuccess) {
    g_create_err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
    delete kin;
    rg_est_destroy(h);
    return RG_EST_ERR_ALLOC;
  }
  e = hipMemcpy(h->kin, kin, sizeof(DevCfg), hipMemcpyHostToDevice);
  delete kin;
  if (e != hipSuccess) {
    g_create_err = std::string("hipMemcpy failed: ") + hipGetErrorString(e);
    rg_est_destroy(h);
    return RG_EST_ERR_HIP;
  }
  *out = h;
  return RG_EST_OK;
}

void rg_est_destroy(rg_est_handle *h) {
  if (!h) return;
  if (h->device >= 0 && h->kin) {
    DeviceScope dev(h->device);
    (void)hipFree(h->kin);
  }
  delete h;
}

int rg_est_reset(rg_est_handle *h, const int32_t *mask, double *est_state, void *stream) {
  if (!h) { g_create_err = "reset: null handle"; return RG_EST_ERR_INVALID; }
  RG_NEED("reset", mask, "mask");
  RG_NEED("reset", est_state, "est_state");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_est_reset_kernel, dim3(((unsigned)h->B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->B, mask, est_state);
  return launch_status(h, "rg_est_reset_kernel launch");
}

int rg_est_estimate(rg_est_handle *h, double *est_state, const rg_srb_obs_ptrs *true_obs, const rg_srb_obs_ptrs *est_obs, void *stream) {
  if (!h) { g_create_err = "estimate: null handle"; return RG_EST_ERR_INVALID; }
  RG_NEED("estimate", est_state, "est_state");
  RG_NEED("estimate", obs_ok(true_obs), "true_obs pointer");
  RG_NEED("estimate", obs_ok(est_obs), "est_obs pointer");
  if (!disjoint(true_obs, est_obs)) { h->err = "estimate: est_obs must not alias true_obs"; return RG_EST_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_est_estimate_kernel, dim3(((unsigned)h->B + kRobots - 1) / kRobots), dim3(kBlock), 0, (hipStream_t)stream, dev_cfg(h), h->kin, est_state,
                     to_obs(true_obs), to_obs(est_obs));
  return launch_status(h, "rg_est_estimate_kernel launch");
}

}  // extern "C"
