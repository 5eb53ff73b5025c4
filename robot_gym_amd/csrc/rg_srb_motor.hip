// rg_srb_motor.hip -- the motor model of include/rg_srb.h (rg_srb_motor_apply, rg_srb_motor.h, which states the rule) and the
// per-episode draw of the strengths (rg_srb_motor_draw).  Its own translation unit of librg_mpc.so: no step kernel, and no file
// a step kernel includes, knows of it.  The rule is a pre-pass over the controller's forces, one launch per control tick.
//
// Layout: lane = (robot, leg) as in the step kernels, 16 robots per wave and 64 per workgroup, float64, no LDS, no cross-lane
// operation: lanes past the batch return.  A lane reads the three floats of its leg before it writes them, so grf_out may be
// grf.  The rows [12][B] are read and written with consecutive robots in the lanes of one leg.
//
// Parity: tests/motor_model.py restates the rule in float64 numpy.  Floating-point contraction is off for the whole file, the
// controller's leg_fk included.
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

#include "rg_stream_dev.inc"

static_assert(purposes_in_block(4, RG_SRB_MOTOR_PURPOSE_STRENGTH), "rg_stream.h: the motor unit owns purposes 64..79");

// The rule of rg_srb_motor.h for one (robot, leg) lane.  tau_cmd, tau_out: [12][B] or NULL.
__global__ void __launch_bounds__(kBlock) rg_srb_motor_apply_kernel(const DevCfg *__restrict__ kc, int B, const double *__restrict__ state,
                                                                     const float *grf, const double *__restrict__ strength,
                                                                     const double *__restrict__ limit, float *grf_out, double *__restrict__ tau_cmd,
                                                                     double *__restrict__ tau_out) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const int leg = t & 3, b = t >> 2;
  if (b >= B) return;   // no cross-lane operation in this kernel
  const size_t sB = (size_t)B, at = (size_t)b * 12 + 3 * leg;
  const float gf[3] = {grf[at], grf[at + 1], grf[at + 2]};
  const double g[3] = {(double)gf[0], (double)gf[1], (double)gf[2]};
  double q[3], pf[3], J[9], tau[3], c[3], md[3];
#pragma unroll
  for (int j = 0; j < 3; j++) q[j] = state[(RG_SRB_ROW_Q + 3 * leg + j) * sB + b];
  leg_fk(kc, leg, q, pf, J);
  bool same = true;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const size_t m = (size_t)(3 * leg + j);
    md[j] = kc->mdir[m];
    tau[j] = ((g[0] * J[j] + g[1] * J[3 + j]) + g[2] * J[6 + j]) * md[j];
    const double a = strength[m * sB + b] * tau[j], lim = limit[m * sB + b];
    c[j] = a != a ? a : fmin(fmax(a, -lim), lim);   // a NaN stays a NaN
    same = same && c[j] == tau[j];
    if (tau_cmd) tau_cmd[m * sB + b] = tau[j];
    if (tau_out) tau_out[m * sB + b] = c[j];
  }
  float out[3] = {gf[0], gf[1], gf[2]};   // pass-through: the bits of grf
  if (!same) {
    // J' g' = c o mdir
    const double A[9] = {J[0], J[3], J[6], J[1], J[4], J[7], J[2], J[5], J[8]};
    const double rhs[3] = {c[0] * md[0], c[1] * md[1], c[2] * md[2]};
    double x[3];
    if (!solve3(A, rhs, x)) {
      // a singular leg: the force keeps its direction and is scaled by the joint that delivers the least of what it was asked
      double k = tau[0] != 0.0 ? c[0] / tau[0] : 1.0;
      k = fmin(k, tau[1] != 0.0 ? c[1] / tau[1] : 1.0);
      k = fmin(k, tau[2] != 0.0 ? c[2] / tau[2] : 1.0);
      x[0] = k * g[0]; x[1] = k * g[1]; x[2] = k * g[2];
    }
    out[0] = (float)x[0]; out[1] = (float)x[1]; out[2] = (float)x[2];
  }
  grf_out[at] = out[0]; grf_out[at + 1] = out[1]; grf_out[at + 2] = out[2];
}

// strength[m][b] = lo + (hi - lo) * u(seed; key, draws, RG_SRB_MOTOR_PURPOSE_STRENGTH, m) for the robots of the mask: one lane per
// robot, twelve values each
__global__ void __launch_bounds__(kBlock) rg_srb_motor_draw_kernel(int B, const int *__restrict__ mask, const double *__restrict__ key,
                                                                    const double *__restrict__ draws, unsigned long long seed, double lo, double hi,
                                                                    double *__restrict__ strength) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;   // no cross-lane operation in this kernel
  if (mask[b] == 0) return;
  const unsigned long long hp = mix_word(mix_word(mix_word(seed, word_of(key[b])), word_of(draws[b])), RG_SRB_MOTOR_PURPOSE_STRENGTH);
  for (int m = 0; m < 12; m++) strength[(size_t)m * B + b] = lo + (hi - lo) * unit53(mix_word(hp, (unsigned long long)m));
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

int rg_srb_motor_apply(rg_srb_handle *h, const double *state, const float *grf, const double *strength, const double *torque_limit,
                       float *grf_out, double *tau_cmd, double *tau_out, void *stream) {
  const char *missing = !state ? "state" : !grf ? "grf" : !strength ? "strength" : !torque_limit ? "torque_limit" : !grf_out ? "grf_out" : nullptr;
  if (missing) return refuse(h, std::string("motor_apply: null ") + missing);
  if (!h) return refuse(h, "motor_apply: null handle");
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const unsigned lanes = 4u * (unsigned)h->B;
  hipLaunchKernelGGL(rg_srb_motor_apply_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->dcfg, h->B, state, grf,
                     strength, torque_limit, grf_out, tau_cmd, tau_out);
  return launch_status(h, "rg_srb_motor_apply_kernel launch");
}

int rg_srb_motor_draw(rg_srb_handle *h, const int32_t *mask, const double *key, const double *draws, uint64_t seed, double lo, double hi,
                      double *strength, void *stream) {
  const char *missing = !mask ? "mask" : !key ? "key" : !draws ? "draws" : !strength ? "strength" : nullptr;
  if (missing) return refuse(h, std::string("motor_draw: null ") + missing);
  if (!(std::isfinite(lo) && lo >= 0.0)) return refuse(h, "motor_draw: lo must be finite and >= 0");
  if (!(std::isfinite(hi) && hi >= lo)) return refuse(h, "motor_draw: hi must be finite and >= lo");
  if (!h) return refuse(h, "motor_draw: null handle");
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_srb_motor_draw_kernel, dim3(((unsigned)h->B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->B, mask, key,
                     draws, (unsigned long long)seed, lo, hi, strength);
  return launch_status(h, "rg_srb_motor_draw_kernel launch");
}

}  // extern "C"
