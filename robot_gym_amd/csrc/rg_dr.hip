// rg_dr.hip -- the domain randomisation of include/rg_dr.h: per episode a mass scale, an inertia scale and a world key for
// the robots a device mask names, written into the simulator handle's private body table (rg_srb_handle.h) and the random
// terrain's key row, and the push of a tick for every robot.  Its own translation unit of librg_mpc.so, so that the
// simulator's units keep reporting exactly their kernels.
//
// Layout: lane = robot, float64 and 64-bit integers, no LDS, no cross-lane operation, 256-thread workgroups.  Consecutive
// lanes are consecutive robots and every load and store is row * B + b, so all of them coalesce.  A lane past the batch
// leaves at once; a robot outside the mask leaves after the mask load, so a wave with nobody to draw for costs a load and
// an exit.  The stream is rg_stream_dev.inc's, the one the ground function reads the world key with.
//
// Parity: tests/dr_model.py restates every output in numpy (uint64 and float64), bit for bit.  Floating-point contraction
// is off for the whole file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rg_dr.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_mpc_dev.h"

namespace {

#include "rg_srb_dev.inc"

}  // namespace

#include "rg_srb_handle.h"

static_assert(kSrbBodyRows == RG_DR_BODY_ROWS, "rg_dr.h names the rows of the simulator's body table");

struct rg_dr_handle {
  rg_dr_config cfg;
  int B = 0, device = 0;
  double *base = nullptr;   // [RG_DR_BODY_ROWS][B]: the body the scales multiply (rg_dr_capture_body)
  bool captured = false;
  std::string err;
};

namespace {

constexpr int kBlock = 256;

struct DrCfg {
  int B, worlds, interval, ticks, substeps;
  unsigned long long seed;
  double mass_lo, mass_hi, inertia_lo, inertia_hi, probability;
  double amp[6];
};

#include "rg_stream_dev.inc"   // the chain over the four words (key, draw, purpose, index)

static_assert(purposes_in_block(0, RG_DR_PURPOSE_MASS, RG_DR_PURPOSE_INERTIA, RG_DR_PURPOSE_WORLD, RG_DR_PURPOSE_PUSH_START, RG_DR_PURPOSE_PUSH_COMPONENT,
                                RG_DR_PURPOSE_PUSH_GATE),
              "the randomiser's purposes are block 0 of rg_stream.h's registry, 0..15");

// body of robot b = base scaled: mass by sm, I by si, I^-1 by 1 / si
__device__ __forceinline__ void write_body(const double *__restrict__ base, double *__restrict__ body, size_t sB, int b, double sm, double si) {
  body[b] = base[b] * sm;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    body[(1 + i) * sB + b] = base[(1 + i) * sB + b] * si;
    body[(10 + i) * sB + b] = base[(10 + i) * sB + b] / si;
  }
}

__global__ void __launch_bounds__(kBlock) rg_dr_reset_kernel(DrCfg c, const double *__restrict__ base, double *__restrict__ body,
                                                             const int *__restrict__ mask, double *__restrict__ st, long long *__restrict__ terrain_key) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= c.B || mask[b] == 0) return;
  const size_t sB = (size_t)c.B;
  const double draws = st[RG_DR_ROW_DRAWS * sB + b];
  const unsigned long long hd = mix_word(mix_word(c.seed, word_of(st[RG_DR_ROW_KEY * sB + b])), word_of(draws));
  const double sm = c.mass_lo + (c.mass_hi - c.mass_lo) * unit53(mix_word(mix_word(hd, RG_DR_PURPOSE_MASS), 0));
  const double si = c.inertia_lo + (c.inertia_hi - c.inertia_lo) * unit53(mix_word(mix_word(hd, RG_DR_PURPOSE_INERTIA), 0));
  write_body(base, body, sB, b, sm, si);
  if (c.worlds) {
    const unsigned long long w = mix_word(mix_word(hd, RG_DR_PURPOSE_WORLD), 0) >> 33;
    terrain_key[b] = (long long)w;
    st[RG_DR_ROW_WORLD * sB + b] = (double)w;
  }
  st[RG_DR_ROW_MASS_SCALE * sB + b] = sm;
  st[RG_DR_ROW_INERTIA_SCALE * sB + b] = si;
  st[RG_DR_ROW_DRAWS * sB + b] = draws + 1.0;
}

__global__ void __launch_bounds__(kBlock) rg_dr_apply_kernel(int B, const double *__restrict__ base, double *__restrict__ body,
                                                             const int *__restrict__ mask, const double *__restrict__ st) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B || (mask && mask[b] == 0)) return;
  const size_t sB = (size_t)B;
  const double sm = st[RG_DR_ROW_MASS_SCALE * sB + b], si = st[RG_DR_ROW_INERTIA_SCALE * sB + b];
  const double inf = __builtin_huge_val();
  if (!(sm > 0.0 && sm < inf && si > 0.0 && si < inf)) return;   // false for a NaN
  write_body(base, body, sB, b, sm, si);
}

__global__ void __launch_bounds__(kBlock) rg_dr_push_kernel(DrCfg c, const double *__restrict__ sim_state, const double *__restrict__ st,
                                                            double *__restrict__ ext) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= c.B) return;
  const size_t sB = (size_t)c.B;
  const double steps = sim_state[RG_SRB_ROW_STEPS * sB + b];
  const unsigned long long k = bounded(steps, kTickBound) / (unsigned long long)c.substeps;   // steps are clamped like a tick row
  const unsigned long long interval = (unsigned long long)c.interval, ticks = (unsigned long long)c.ticks;
  const unsigned long long win = k / interval, r = k % interval;
  const unsigned long long hd = mix_word(mix_word(c.seed, word_of(st[RG_DR_ROW_KEY * sB + b])), word_of(st[RG_DR_ROW_DRAWS * sB + b]));
  const unsigned long long n = interval - ticks + 1;
  unsigned long long start = (unsigned long long)((double)n * unit53(mix_word(mix_word(hd, RG_DR_PURPOSE_PUSH_START), win)));
  start = start < n - 1 ? start : n - 1;
  const bool active = start <= r && r < start + ticks && unit53(mix_word(mix_word(hd, RG_DR_PURPOSE_PUSH_GATE), win)) < c.probability;
  const unsigned long long hc = mix_word(hd, RG_DR_PURPOSE_PUSH_COMPONENT);
#pragma unroll
  for (int a = 0; a < 6; a++)
    ext[(size_t)a * sB + b] = active ? c.amp[a] * (2.0 * unit53(mix_word(hc, 8 * win + (unsigned long long)a)) - 1.0) : 0.0;
}

thread_local std::string g_create_err;

bool validate(const rg_dr_config *cfg, std::string &err) {
  if (!check_abi("config.", cfg->abi_version, RG_DR_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err)) return false;
  const IntField ints[] = {{"worlds", cfg->worlds, 0, 1}, {"push_interval", cfg->push_interval, 0, INT32_MAX},
                           {"substeps", cfg->substeps, 1, RG_SRB_MAX_SUBSTEPS}};
  const RealField reals[] = {{"mass_lo", &cfg->mass_lo, 1, kPositive}, {"mass_hi", &cfg->mass_hi, 1, kPositive},
                             {"inertia_lo", &cfg->inertia_lo, 1, kPositive}, {"inertia_hi", &cfg->inertia_hi, 1, kPositive},
                             {"push_probability", &cfg->push_probability, 1, kUnit}, {"push_force_xy", &cfg->push_force_xy, 1, kNonNegative},
                             {"push_force_z", &cfg->push_force_z, 1, kNonNegative}, {"push_torque_xy", &cfg->push_torque_xy, 1, kNonNegative},
                             {"push_torque_z", &cfg->push_torque_z, 1, kNonNegative}};
  if (!check_ints("config.", ints, err) || !check_reals("config.", reals, err)) return false;
  char msg[200];
  if (cfg->mass_lo > cfg->mass_hi) { snprintf(msg, sizeof(msg), "config.mass_hi: %g below mass_lo %g", cfg->mass_hi, cfg->mass_lo); err = msg; return false; }
  if (cfg->inertia_lo > cfg->inertia_hi) { snprintf(msg, sizeof(msg), "config.inertia_hi: %g below inertia_lo %g", cfg->inertia_hi, cfg->inertia_lo); err = msg; return false; }
  const int lo = cfg->push_interval ? 1 : 0;
  if (cfg->push_ticks < lo || cfg->push_ticks > cfg->push_interval) {
    snprintf(msg, sizeof(msg), "config.push_ticks: %d outside [%d, %d] (push_interval)", cfg->push_ticks, lo, cfg->push_interval);
    err = msg;
    return false;
  }
  return true;
}

DrCfg dev_cfg(const rg_dr_handle *h) {
  const rg_dr_config &f = h->cfg;
  return DrCfg{h->B, f.worlds, f.push_interval, f.push_ticks, f.substeps, (unsigned long long)f.seed, f.mass_lo, f.mass_hi, f.inertia_lo, f.inertia_hi,
               f.push_probability, {f.push_force_xy, f.push_force_xy, f.push_force_z, f.push_torque_xy, f.push_torque_xy, f.push_torque_z}};
}

int hip_fail(rg_dr_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_DR_ERR_HIP, what, e); }
int no_device(rg_dr_handle *h) { return no_device(h, RG_DR_ERR_NO_DEVICE, "RG_DR"); }
int launch_status(rg_dr_handle *h, const char *what) { return launch_status(h, RG_DR_ERR_HIP, what); }
int null_arg(rg_dr_handle *h, const char *call, const char *name) { return null_arg(h, RG_DR_ERR_INVALID, call, name); }

// the simulator handle of an entry: the same batch, and (with a device) the same device.  0 where it fits.
int srb_fits(rg_dr_handle *h, const char *call, const rg_srb_handle *srb) {
  char msg[200];
  if (srb->B != h->B) {
    snprintf(msg, sizeof(msg), "%s: srb has batch %d, this handle %d", call, srb->B, h->B);
    h->err = msg;
    return RG_DR_ERR_INVALID;
  }
  if (h->device >= 0 && srb->device != h->device) {
    snprintf(msg, sizeof(msg), "%s: srb is on device %d, this handle on %d", call, srb->device, h->device);
    h->err = msg;
    return RG_DR_ERR_INVALID;
  }
  return 0;
}

int need_capture(rg_dr_handle *h, const char *call) {
  if (h->captured) return 0;
  h->err = std::string(call) + ": no base body yet (rg_dr_capture_body first)";
  return RG_DR_ERR_INVALID;
}

unsigned blocks(int B) { return ((unsigned)B + kBlock - 1) / kBlock; }

}  // namespace

extern "C" {

int32_t rg_dr_abi_version(void) { return RG_DR_ABI_VERSION; }
int32_t rg_dr_config_size(void) { return (int32_t)sizeof(rg_dr_config); }
int32_t rg_dr_state_rows(void) { return RG_DR_ROWS; }
const char *rg_dr_last_error(const rg_dr_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_dr_create(const rg_dr_config *cfg, int32_t batch, int32_t device, rg_dr_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_DR_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!check_batch(batch, RG_DR_MAX_BATCH, err) || !validate(cfg, err)) { g_create_err = err; return RG_DR_ERR_INVALID; }
  double *base = nullptr;
  if (device != RG_DR_DEVICE_NONE) {
    std::optional<DeviceScope> dev;
    if (const int rc = enter_device(device, &dev, RG_DR_ERR_NO_DEVICE, RG_DR_ERR_INVALID, RG_DR_ERR_HIP, g_create_err)) return rc;
    const hipError_t e = hipMalloc((void **)&base, (size_t)RG_DR_BODY_ROWS * (size_t)batch * sizeof(double));
    if (e != hipSuccess) { g_create_err = std::string("hipMalloc failed: ") + hipGetErrorString(e); return RG_DR_ERR_ALLOC; }
  }
  rg_dr_handle *h = new rg_dr_handle();
  h->cfg = *cfg;
  h->B = batch;
  h->device = device;
  h->base = base;
  *out = h;
  return RG_DR_OK;
}

void rg_dr_destroy(rg_dr_handle *h) {
  if (!h) return;
  if (h->base) {
    DeviceScope dev(h->device);
    (void)hipFree(h->base);
  }
  delete h;
}

int rg_dr_capture_body(rg_dr_handle *h, rg_srb_handle *srb) {
  if (!h) { g_create_err = "capture_body: null handle"; return RG_DR_ERR_INVALID; }
  RG_NEED("capture_body", srb, "srb");
  if (const int rc = srb_fits(h, "capture_body", srb)) return rc;
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const hipError_t e = hipMemcpy(h->base, srb->body_host.data(), (size_t)RG_DR_BODY_ROWS * (size_t)h->B * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(h, "capture_body copy", e);
  h->captured = true;
  return RG_DR_OK;
}

int rg_dr_reset(rg_dr_handle *h, rg_srb_handle *srb, const int32_t *mask, double *dr_state, int64_t *terrain_key, void *stream) {
  if (!h) { g_create_err = "reset: null handle"; return RG_DR_ERR_INVALID; }
  RG_NEED("reset", srb, "srb");
  RG_NEED("reset", mask, "mask");
  RG_NEED("reset", dr_state, "dr_state");
  if (h->cfg.worlds && !terrain_key) { h->err = "reset: null terrain_key (config.worlds is 1: the random terrain's key row is required)"; return RG_DR_ERR_INVALID; }
  if (!h->cfg.worlds && terrain_key) { h->err = "reset: terrain_key must be null (config.worlds is 0: no world is drawn)"; return RG_DR_ERR_INVALID; }
  if (const int rc = srb_fits(h, "reset", srb)) return rc;
  if (h->device < 0) return no_device(h);
  if (const int rc = need_capture(h, "reset")) return rc;
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_dr_reset_kernel, dim3(blocks(h->B)), dim3(kBlock), 0, (hipStream_t)stream, dev_cfg(h), h->base, srb->body, mask, dr_state,
                     (long long *)terrain_key);
  return launch_status(h, "rg_dr_reset_kernel launch");
}

int rg_dr_apply(rg_dr_handle *h, rg_srb_handle *srb, const int32_t *mask, const double *dr_state, void *stream) {
  if (!h) { g_create_err = "apply: null handle"; return RG_DR_ERR_INVALID; }
  RG_NEED("apply", srb, "srb");
  RG_NEED("apply", dr_state, "dr_state");
  if (const int rc = srb_fits(h, "apply", srb)) return rc;
  if (h->device < 0) return no_device(h);
  if (const int rc = need_capture(h, "apply")) return rc;
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_dr_apply_kernel, dim3(blocks(h->B)), dim3(kBlock), 0, (hipStream_t)stream, h->B, h->base, srb->body, mask, dr_state);
  return launch_status(h, "rg_dr_apply_kernel launch");
}

int rg_dr_push(rg_dr_handle *h, const double *sim_state, const double *dr_state, double *ext, void *stream) {
  if (!h) { g_create_err = "push: null handle"; return RG_DR_ERR_INVALID; }
  RG_NEED("push", sim_state, "sim_state");
  RG_NEED("push", dr_state, "dr_state");
  RG_NEED("push", ext, "ext");
  if (h->cfg.push_interval == 0) { h->err = "push: config.push_interval is 0, there is no push (pass the simulator a null ext)"; return RG_DR_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_dr_push_kernel, dim3(blocks(h->B)), dim3(kBlock), 0, (hipStream_t)stream, dev_cfg(h), sim_state, dr_state, ext);
  return launch_status(h, "rg_dr_push_kernel launch");
}

int rg_dr_get_body(rg_dr_handle *h, rg_srb_handle *srb, double *out, void *stream) {
  if (!h) { g_create_err = "get_body: null handle"; return RG_DR_ERR_INVALID; }
  RG_NEED("get_body", srb, "srb");
  RG_NEED("get_body", out, "out");
  if (const int rc = srb_fits(h, "get_body", srb)) return rc;
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const hipError_t e = hipMemcpyAsync(out, srb->body, (size_t)RG_DR_BODY_ROWS * (size_t)h->B * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e != hipSuccess ? hip_fail(h, "get_body copy", e) : RG_DR_OK;
}

}  // extern "C"
