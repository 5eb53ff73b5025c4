// rg_sensor.hip -- the sensor and actuator model of include/rg_sensor.h: bias, white noise, quantisation, dropout and latency
// on float32 observation rows, noise and latency on actions, per robot and per episode.  Its own translation unit of
// librg_mpc.so; it includes nothing of the controller's or the simulator's.
//
// Layout.  reset and observe: a workgroup of 256 lanes is 32 consecutive robots (lane % 32) times 8 row slices (lane / 32);
// slice s takes the rows s, s + 8, ...  A wave is two slices of the same 32 robots, every load and store is row * B + b, so a
// slice moves one 128-byte run per row.  At D = 64 a lane hashes 8 rows instead of 64, and batch 64 is 8 waves on two compute
// units instead of one wave on one.  The state rows a robot's lanes all read (draws, ticks) have one writer, slice 0: every
// lane reads, the workgroup meets at a barrier, then slice 0 writes.  A robot's lanes share a workgroup by construction
// (the robot is the low part of the lane index), so the barrier orders them; no lane leaves before it.
// act: one lane per robot, at most 8 components of 4 hashes each.
// No LDS, no atomics, no cross-lane operation.  The groups and the per-component settings are read from the kernel argument
// with constant indices only (unrolled loops and selects), so nothing is indexed dynamically and nothing goes to scratch.
//
// The stream is rg_stream_dev.inc's.
// Parity: tests/sensor_model.py restates every output in numpy (uint64 and float64), bit for bit.  Floating-point
// contraction is off for the whole file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rg_sensor.h"
#include "rg_host.h"

#pragma clang fp contract(off)

struct rg_sensor_handle {
  rg_sensor_config cfg;
  int B = 0, device = 0;
  std::string err;
};

namespace {

constexpr int kBlock = 256;
constexpr int kRobots = 32;                  // robots of a workgroup of reset and observe
constexpr int kSlices = kBlock / kRobots;    // lanes of a robot: row slices

struct SensorCfg {
  int B, D, A, Lo, La;
  int od_min, od_max, ad_min, ad_max;
  unsigned long long seed;
  int begin[RG_SENSOR_MAX_GROUPS], end[RG_SENSOR_MAX_GROUPS];   // begin == end: unused
  double sigma[RG_SENSOR_MAX_GROUPS], bias[RG_SENSOR_MAX_GROUPS], prob[RG_SENSOR_MAX_GROUPS], dropv[RG_SENSOR_MAX_GROUPS], quantum[RG_SENSOR_MAX_GROUPS];
  double act_sigma[RG_SENSOR_MAX_ACT], act_fill[RG_SENSOR_MAX_ACT];
};

#include "rg_stream_dev.inc"   // the chain over the four words (key, draw, purpose, index)

static_assert(purposes_in_block(1, RG_SENSOR_PURPOSE_OBS_DELAY, RG_SENSOR_PURPOSE_ACT_DELAY, RG_SENSOR_PURPOSE_BIAS, RG_SENSOR_PURPOSE_NOISE,
                                RG_SENSOR_PURPOSE_DROPOUT, RG_SENSOR_PURPOSE_ACT_NOISE),
              "the sensor model's purposes are block 1 of rg_stream.h's registry, 16..31");

// the delay of an episode in lo .. hi
__device__ __forceinline__ unsigned long long draw_delay(unsigned long long hd, unsigned long long purpose, int lo, int hi) {
  const unsigned long long span = (unsigned long long)(hi - lo);
  const unsigned long long v = (unsigned long long)((double)(span + 1) * unit53(mix_word(mix_word(hd, purpose), 0)));
  return (unsigned long long)lo + (v < span ? v : span);
}

// the measurement of row r at tick k; hd = the chain over (seed, key, d)
__device__ __forceinline__ float measure(const SensorCfg &c, unsigned long long hd, unsigned long long k, int r, float clean) {
  double sigma = 0.0, bias = 0.0, prob = 0.0, dropv = 0.0, quantum = 0.0;
#pragma unroll
  for (int g = 0; g < RG_SENSOR_MAX_GROUPS; g++)
    if (r >= c.begin[g] && r < c.end[g]) { sigma = c.sigma[g]; bias = c.bias[g]; prob = c.prob[g]; dropv = c.dropv[g]; quantum = c.quantum[g]; }
  if (sigma == 0.0 && bias == 0.0 && prob == 0.0 && quantum == 0.0) return clean;   // bits
  const unsigned long long ix = index_word(k, r);
  double x = (double)clean;
  if (bias != 0.0) x = x + bias * (2.0 * unit53(mix_word(mix_word(hd, RG_SENSOR_PURPOSE_BIAS), (unsigned long long)r)) - 1.0);
  if (sigma != 0.0) x = x + sigma * unit_noise(mix_word(hd, RG_SENSOR_PURPOSE_NOISE), ix);
  if (quantum != 0.0) x = quantum * rint(x / quantum);
  if (prob != 0.0 && unit53(mix_word(mix_word(hd, RG_SENSOR_PURPOSE_DROPOUT), ix)) < prob) x = dropv;
  return (float)x;
}

__global__ void __launch_bounds__(kBlock) rg_sensor_reset_kernel(SensorCfg c, const int *__restrict__ mask, double *__restrict__ st,
                                                                 const float *__restrict__ clean, float *__restrict__ ring, float *__restrict__ out,
                                                                 float *__restrict__ prev, float *__restrict__ act_ring) {
  const int b = blockIdx.x * kRobots + (int)(threadIdx.x % kRobots), s = (int)(threadIdx.x / kRobots);
  const size_t sB = (size_t)c.B;
  const bool live = b < c.B && mask[b] != 0;
  double draws = 0.0, key = 0.0;
  if (live) { draws = st[RG_SENSOR_ROW_DRAWS * sB + b]; key = st[RG_SENSOR_ROW_KEY * sB + b]; }
  __syncthreads();   // every lane of a robot has read draws before slice 0 writes it
  if (!live) return;
  const unsigned long long hd = mix_word(mix_word(c.seed, word_of(key)), word_of(draws));
  // the state and the action ring first: their settings are dead before the groups' are live
  if (s == 0) {
    st[RG_SENSOR_ROW_OBS_DELAY * sB + b] = (double)draw_delay(hd, RG_SENSOR_PURPOSE_OBS_DELAY, c.od_min, c.od_max);
    st[RG_SENSOR_ROW_ACT_DELAY * sB + b] = (double)draw_delay(hd, RG_SENSOR_PURPOSE_ACT_DELAY, c.ad_min, c.ad_max);
    st[RG_SENSOR_ROW_OBS_TICKS * sB + b] = 1.0;
    st[RG_SENSOR_ROW_ACT_TICKS * sB + b] = 0.0;
    st[RG_SENSOR_ROW_DRAWS * sB + b] = draws + 1.0;
  }
  for (int l = s; l < c.La; l += kSlices) {
#pragma unroll
    for (int a = 0; a < RG_SENSOR_MAX_ACT; a++)
      if (a < c.A) act_ring[((size_t)l * c.A + a) * sB + b] = (float)c.act_fill[a];
  }
  const size_t slot = (size_t)c.D * sB;
  if (prev)
    for (int r = s; r < c.D; r += kSlices) prev[(size_t)r * sB + b] = out[(size_t)r * sB + b];
  for (int r = s; r < c.D; r += kSlices) {
    const size_t at = (size_t)r * sB + b;
    const float m = measure(c, hd, 0, r, clean[at]);
    float *p = ring + at;
    for (int l = 0; l < c.Lo; l++, p += slot) *p = m;
    out[at] = m;
  }
}

__global__ void __launch_bounds__(kBlock) rg_sensor_observe_kernel(SensorCfg c, double *__restrict__ st, const float *__restrict__ clean,
                                                                   float *__restrict__ ring, float *__restrict__ out) {
  const int b = blockIdx.x * kRobots + (int)(threadIdx.x % kRobots), s = (int)(threadIdx.x / kRobots);
  const size_t sB = (size_t)c.B;
  const bool live = b < c.B;
  double ticks = 0.0, draws = 0.0, key = 0.0, delay = 0.0;
  if (live) {
    ticks = st[RG_SENSOR_ROW_OBS_TICKS * sB + b]; draws = st[RG_SENSOR_ROW_DRAWS * sB + b];
    key = st[RG_SENSOR_ROW_KEY * sB + b]; delay = st[RG_SENSOR_ROW_OBS_DELAY * sB + b];
  }
  __syncthreads();   // every lane of a robot has read obs_ticks before slice 0 writes it
  if (!live) return;
  const unsigned long long k = bounded(ticks, kTickBound), Lo = (unsigned long long)c.Lo, dl = bounded(delay, (double)c.od_max);
  const unsigned long long hd = mix_word(mix_word(c.seed, word_of(key)), word_of(draws - 1.0));
  const size_t slot = (size_t)c.D * sB;
  const size_t wr = (size_t)(k % Lo) * slot, rd = (size_t)((k + Lo - dl) % Lo) * slot;
  for (int r = s; r < c.D; r += kSlices) {
    const size_t at = (size_t)r * sB + b;
    const float m = measure(c, hd, k, r, clean[at]);
    ring[wr + at] = m;
    out[at] = rd == wr ? m : ring[rd + at];   // another slot: this lane wrote it on an earlier tick
  }
  if (s == 0) st[RG_SENSOR_ROW_OBS_TICKS * sB + b] = (double)(k + 1);
}

__global__ void __launch_bounds__(kBlock) rg_sensor_act_kernel(SensorCfg c, double *__restrict__ st, const float *act_in, float *__restrict__ ring,
                                                               float *act_out) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= c.B) return;
  const size_t sB = (size_t)c.B;
  const unsigned long long k = bounded(st[RG_SENSOR_ROW_ACT_TICKS * sB + b], kTickBound), La = (unsigned long long)c.La;
  const unsigned long long dl = bounded(st[RG_SENSOR_ROW_ACT_DELAY * sB + b], (double)c.ad_max);
  const unsigned long long hd = mix_word(mix_word(c.seed, word_of(st[RG_SENSOR_ROW_KEY * sB + b])), word_of(st[RG_SENSOR_ROW_DRAWS * sB + b] - 1.0));
  const unsigned long long hp = mix_word(hd, RG_SENSOR_PURPOSE_ACT_NOISE);
  const size_t slot = (size_t)c.A * sB;
  const size_t wr = (size_t)(k % La) * slot, rd = (size_t)((k + La - dl) % La) * slot;
#pragma unroll
  for (int a = 0; a < RG_SENSOR_MAX_ACT; a++) {
    if (a < c.A) {
      float v = act_in[(size_t)b * c.A + a];
      const double sigma = c.act_sigma[a];
      if (sigma != 0.0) v = (float)((double)v + sigma * unit_noise(hp, index_word(k, a)));
      const size_t at = (size_t)a * sB + b;
      ring[wr + at] = v;
      act_out[(size_t)b * c.A + a] = rd == wr ? v : ring[rd + at];
    }
  }
  st[RG_SENSOR_ROW_ACT_TICKS * sB + b] = (double)(k + 1);
}

thread_local std::string g_create_err;

bool group_error(std::string &err, int g, const char *field, const char *what) {
  char msg[200];
  snprintf(msg, sizeof(msg), "config.groups[%d].%s: %s", g, field, what);
  err = msg;
  return false;
}

bool validate(const rg_sensor_config *cfg, std::string &err) {
  if (!check_abi("config.", cfg->abi_version, RG_SENSOR_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err) ||
      !check_reserved("config.", "reserved1", cfg->reserved1, err))
    return false;
  const IntField dims[] = {{"obs_dim", cfg->obs_dim, 1, RG_SENSOR_MAX_OBS}, {"act_dim", cfg->act_dim, 1, RG_SENSOR_MAX_ACT},
                           {"n_groups", cfg->n_groups, 0, RG_SENSOR_MAX_GROUPS}};
  if (!check_ints("config.", dims, err)) return false;
  const IntField delays[] = {{"obs_delay_min", cfg->obs_delay_min, 0, RG_SENSOR_MAX_DELAY}, {"obs_delay_max", cfg->obs_delay_max, cfg->obs_delay_min, RG_SENSOR_MAX_DELAY},
                             {"act_delay_min", cfg->act_delay_min, 0, RG_SENSOR_MAX_DELAY}, {"act_delay_max", cfg->act_delay_max, cfg->act_delay_min, RG_SENSOR_MAX_DELAY}};
  if (!check_ints("config.", delays, err)) return false;
  char msg[200];
  for (int g = 0; g < RG_SENSOR_MAX_GROUPS; g++) {
    const rg_sensor_group &q = cfg->groups[g];
    char prefix[40];
    snprintf(prefix, sizeof(prefix), "config.groups[%d].", g);
    if (g >= cfg->n_groups) {
      if (q.begin != 0) return group_error(err, g, "begin", "must be 0 past the groups in use");
      if (q.end != 0) return group_error(err, g, "end", "must be 0 past the groups in use");
      const double *reals[] = {&q.noise_sigma, &q.bias_half_width, &q.dropout_probability, &q.dropout_value, &q.quantum};
      const char *names[] = {"noise_sigma", "bias_half_width", "dropout_probability", "dropout_value", "quantum"};
      for (int i = 0; i < 5; i++)
        if (!(*reals[i] == 0.0)) return group_error(err, g, names[i], "must be 0 past the groups in use");
      continue;
    }
    const IntField rows[] = {{"begin", q.begin, 0, cfg->obs_dim - 1}, {"end", q.end, q.begin + 1, cfg->obs_dim}};
    const RealField reals[] = {{"noise_sigma", &q.noise_sigma, 1, kNonNegative}, {"bias_half_width", &q.bias_half_width, 1, kNonNegative},
                               {"dropout_probability", &q.dropout_probability, 1, kUnit}, {"dropout_value", &q.dropout_value, 1, kFinite},
                               {"quantum", &q.quantum, 1, kNonNegative}};
    if (!check_ints(prefix, rows, err) || !check_reals(prefix, reals, err)) return false;
    for (int o = 0; o < g; o++)
      if (q.begin < cfg->groups[o].end && cfg->groups[o].begin < q.end) {
        snprintf(msg, sizeof(msg), "config.groups[%d].begin: rows [%d, %d) overlap groups[%d] [%d, %d)", g, q.begin, q.end, o, cfg->groups[o].begin, cfg->groups[o].end);
        err = msg;
        return false;
      }
  }
  for (int a = 0; a < RG_SENSOR_MAX_ACT; a++) {
    const double sg = cfg->act_noise_sigma[a], fill = cfg->act_fill[a];
    const bool used = a < cfg->act_dim;
    if (!(used ? std::isfinite(sg) && sg >= 0.0 : sg == 0.0)) {
      snprintf(msg, sizeof(msg), "config.act_noise_sigma[%d]: %g must be %s", a, sg, used ? "finite and >= 0" : "0 past act_dim");
      err = msg;
      return false;
    }
    if (!(used ? std::isfinite(fill) : fill == 0.0)) {
      snprintf(msg, sizeof(msg), "config.act_fill[%d]: %g must be %s", a, fill, used ? "finite" : "0 past act_dim");
      err = msg;
      return false;
    }
  }
  return true;
}

SensorCfg dev_cfg(const rg_sensor_handle *h) {
  const rg_sensor_config &f = h->cfg;
  SensorCfg c{};
  c.B = h->B; c.D = f.obs_dim; c.A = f.act_dim; c.Lo = f.obs_delay_max + 1; c.La = f.act_delay_max + 1;
  c.od_min = f.obs_delay_min; c.od_max = f.obs_delay_max; c.ad_min = f.act_delay_min; c.ad_max = f.act_delay_max;
  c.seed = (unsigned long long)f.seed;
  for (int g = 0; g < f.n_groups; g++) {
    const rg_sensor_group &q = f.groups[g];
    c.begin[g] = q.begin; c.end[g] = q.end;
    c.sigma[g] = q.noise_sigma; c.bias[g] = q.bias_half_width; c.prob[g] = q.dropout_probability; c.dropv[g] = q.dropout_value; c.quantum[g] = q.quantum;
  }
  for (int a = 0; a < RG_SENSOR_MAX_ACT; a++) { c.act_sigma[a] = f.act_noise_sigma[a]; c.act_fill[a] = f.act_fill[a]; }
  return c;
}

int hip_fail(rg_sensor_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_SENSOR_ERR_HIP, what, e); }
int no_device(rg_sensor_handle *h) { return no_device(h, RG_SENSOR_ERR_NO_DEVICE, "RG_SENSOR"); }
int launch_status(rg_sensor_handle *h, const char *what) { return launch_status(h, RG_SENSOR_ERR_HIP, what); }
int null_arg(rg_sensor_handle *h, const char *call, const char *name) { return null_arg(h, RG_SENSOR_ERR_INVALID, call, name); }

unsigned robot_blocks(int B) { return ((unsigned)B + kRobots - 1) / kRobots; }

}  // namespace

extern "C" {

int32_t rg_sensor_abi_version(void) { return RG_SENSOR_ABI_VERSION; }
int32_t rg_sensor_config_size(void) { return (int32_t)sizeof(rg_sensor_config); }
int32_t rg_sensor_state_rows(void) { return RG_SENSOR_ROWS; }
const char *rg_sensor_last_error(const rg_sensor_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_sensor_create(const rg_sensor_config *cfg, int32_t batch, int32_t device, rg_sensor_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_SENSOR_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!check_batch(batch, RG_SENSOR_MAX_BATCH, err) || !validate(cfg, err)) { g_create_err = err; return RG_SENSOR_ERR_INVALID; }
  if (device != RG_SENSOR_DEVICE_NONE)
    if (const int rc = enter_device(device, nullptr, RG_SENSOR_ERR_NO_DEVICE, RG_SENSOR_ERR_INVALID, RG_SENSOR_ERR_HIP, g_create_err)) return rc;
  rg_sensor_handle *h = new rg_sensor_handle();
  h->cfg = *cfg;
  h->B = batch;
  h->device = device;
  *out = h;
  return RG_SENSOR_OK;
}

void rg_sensor_destroy(rg_sensor_handle *h) { delete h; }

int rg_sensor_reset(rg_sensor_handle *h, const int32_t *mask, double *sensor_state, const float *obs_clean, float *obs_ring, float *obs_out, float *obs_prev,
                    float *act_ring, void *stream) {
  if (!h) { g_create_err = "reset: null handle"; return RG_SENSOR_ERR_INVALID; }
  RG_NEED("reset", mask, "mask");
  RG_NEED("reset", sensor_state, "sensor_state");
  RG_NEED("reset", obs_clean, "obs_clean");
  RG_NEED("reset", obs_ring, "obs_ring");
  RG_NEED("reset", obs_out, "obs_out");
  RG_NEED("reset", act_ring, "act_ring");
  if (obs_prev == obs_out) { h->err = "reset: obs_prev must not be obs_out"; return RG_SENSOR_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_sensor_reset_kernel, dim3(robot_blocks(h->B)), dim3(kBlock), 0, (hipStream_t)stream, dev_cfg(h), mask, sensor_state, obs_clean, obs_ring,
                     obs_out, obs_prev, act_ring);
  return launch_status(h, "rg_sensor_reset_kernel launch");
}

int rg_sensor_observe(rg_sensor_handle *h, double *sensor_state, const float *obs_clean, float *obs_ring, float *obs_out, void *stream) {
  if (!h) { g_create_err = "observe: null handle"; return RG_SENSOR_ERR_INVALID; }
  RG_NEED("observe", sensor_state, "sensor_state");
  RG_NEED("observe", obs_clean, "obs_clean");
  RG_NEED("observe", obs_ring, "obs_ring");
  RG_NEED("observe", obs_out, "obs_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_sensor_observe_kernel, dim3(robot_blocks(h->B)), dim3(kBlock), 0, (hipStream_t)stream, dev_cfg(h), sensor_state, obs_clean, obs_ring,
                     obs_out);
  return launch_status(h, "rg_sensor_observe_kernel launch");
}

int rg_sensor_act(rg_sensor_handle *h, double *sensor_state, const float *act_in, float *act_ring, float *act_out, void *stream) {
  if (!h) { g_create_err = "act: null handle"; return RG_SENSOR_ERR_INVALID; }
  RG_NEED("act", sensor_state, "sensor_state");
  RG_NEED("act", act_in, "act_in");
  RG_NEED("act", act_ring, "act_ring");
  RG_NEED("act", act_out, "act_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_sensor_act_kernel, dim3(((unsigned)h->B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, dev_cfg(h), sensor_state, act_in,
                     act_ring, act_out);
  return launch_status(h, "rg_sensor_act_kernel launch");
}

}  // extern "C"
