// rg_policy.hip -- the acting and collecting side of the PPO agent of include/rg_policy.h.  Its own translation unit of
// librg_mpc.so.  The noise stream, the normaliser's arithmetic, the workgroup sum and the layer descriptor are those of
// rg_agent_dev.inc, which the agents' update files include too, and the host helpers those of rg_host.h; rg_mpc.hip
// includes neither, so the source hash behind profiles/ is unaffected.  The act kernel's neuron (8 samples wide, where the
// shared layer is 16) stays here.
//
// rg_policy_act_kernel: kTile robots per workgroup of 512 threads.  Threads 0..255 (waves 0..3) run the policy network,
// threads 256..511 (waves 4..7) the value network: every branch on the network is uniform over a wave, and both halves meet
// at the same __syncthreads.  One output neuron per thread, kTile accumulators in registers; the activations of a layer lie
// in LDS as x[i][robot] (a thread reads the kTile values of input i as two 16-byte broadcasts) and ping-pong between two
// buffers per network; the weight W[i][j] is read once per (workgroup, neuron), coalesced along j, and used kTile times.
// A batch of one still spreads its 200 + 200 neurons over the lanes.  The sum over i runs in order with explicit fmaf, so it
// depends on the configuration alone.  The layer descriptors are read from device memory (dynamic indexing of a by-value
// kernel argument could end on the stack).
// LDS: 2 networks * 2 buffers * 256 * kTile floats + kTile * 4 floats = 32896 bytes.
//
// rg_policy_record: grid (G, obs_dim + 1), G = min(ceil(B / 256), 256) workgroups per column striding over the robots.
// first: copies, and partial n / sum(v - mean) / sum(v) per workgroup; second: every workgroup finishes those partials in
// the same fixed order, forms new_mean and sums (v - mean)(v - new_mean); finish: one workgroup per column writes the state.
// Sums inside a workgroup are a shuffle tree and an in-order sum over the four waves; nothing is accumulated in place
// across workgroups.
// rg_policy_returns_kernel: one thread per robot, backwards over T.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rg_policy.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_agent_dev.inc"

namespace {

constexpr int kTile = RG_POLICY_TILE;
constexpr int kMaxW = RG_POLICY_MAX_WIDTH;
constexpr int kMaxAct = RG_POLICY_MAX_ACT;
constexpr int kHalf = 256;
constexpr int kActThreads = 2 * kHalf;
constexpr int kRed = kAgentThreads;   // threads of a record / returns workgroup: block_sum's four waves
constexpr int kMaxGroups = 256;    // workgroups per column of rg_policy_record
constexpr int kCols = RG_POLICY_NORM_COLS;
constexpr int kRewardCol = RG_POLICY_NORM_REWARD;
constexpr int kParts = 4;          // n, sum(v - mean), sum(v), sum((v - mean)(v - new_mean))

static_assert(kTile == 8, "the act kernel reads the activations of an input as two float4");
static_assert(kTile * RG_POLICY_MAX_OBS <= kActThreads && kTile * kMaxAct <= 64, "act kernel thread maps");
static_assert(RG_POLICY_NORM_ROWS == 3 * kCols && kRewardCol == RG_POLICY_MAX_OBS, "norm_state layout");

struct ActDev {
  int B, obs_dim, act_dim, logstd_off;
  double obs_clip;
  unsigned long long seed;
  NetDesc pol, val;
};

__global__ void __launch_bounds__(kActThreads) rg_policy_act_kernel(const ActDev *__restrict__ d, const float *__restrict__ obs,
                                                                    const double *__restrict__ norm, const float *__restrict__ pp,
                                                                    const float *__restrict__ vp, long long *__restrict__ act_state, const int mode,
                                                                    float *__restrict__ action, float *__restrict__ mean, float *__restrict__ value,
                                                                    float *__restrict__ logprob) {
  __shared__ __attribute__((aligned(16))) float xs[2][2][kMaxW * kTile];   // [network][buffer][input * kTile + robot]
  __shared__ float eps_s[kTile * kMaxAct];
  const int tid = threadIdx.x;
  const int net = tid >> 8;          // uniform over a wave
  const int j = tid & (kHalf - 1);
  const int B = d->B, obs_dim = d->obs_dim, act_dim = d->act_dim;
  const int b0 = blockIdx.x * kTile;
  // the observation through the normaliser, once, into the first buffer of both networks
  if (tid < obs_dim * kTile) {
    const int i = tid / kTile, r = tid % kTile, b = b0 + r;
    float xn = 0.0f;
    if (b < B) {
      double v = (double)obs[(size_t)i * B + b] - norm[kCols + i];
      v = v / norm_scale(norm[i], norm[2 * kCols + i]);
      xn = (float)clip_sym(v, d->obs_clip);
    }
    xs[0][0][tid] = xn;
    xs[1][0][tid] = xn;
  }
  const NetDesc &nd = net ? d->val : d->pol;
  const float *__restrict__ P = net ? vp : pp;
  const int n_mine = nd.n;
  const int n_max = d->pol.n > d->val.n ? d->pol.n : d->val.n;
  int cur = 0;
  for (int l = 0; l < n_max; l++) {
    __syncthreads();
    if (l < n_mine) {   // uniform over a wave
      const int nin = nd.in[l], nout = nd.out[l];
      if (j < nout) {
        const float *__restrict__ W = P + nd.w[l] + j;
        const float *x = xs[net][cur];
        float acc[kTile];
#pragma unroll
        for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
#pragma unroll 8
        for (int i = 0; i < nin; i++) {
          const float w = W[(size_t)i * nout];
          const float4 xa = *reinterpret_cast<const float4 *>(x + i * kTile);
          const float4 xb = *reinterpret_cast<const float4 *>(x + i * kTile + 4);
          acc[0] = __builtin_fmaf(w, xa.x, acc[0]); acc[1] = __builtin_fmaf(w, xa.y, acc[1]);
          acc[2] = __builtin_fmaf(w, xa.z, acc[2]); acc[3] = __builtin_fmaf(w, xa.w, acc[3]);
          acc[4] = __builtin_fmaf(w, xb.x, acc[4]); acc[5] = __builtin_fmaf(w, xb.y, acc[5]);
          acc[6] = __builtin_fmaf(w, xb.z, acc[6]); acc[7] = __builtin_fmaf(w, xb.w, acc[7]);
        }
        const float bias = P[nd.b[l] + j];
        const bool head = l == n_mine - 1;
        float *y = xs[net][cur ^ 1] + j * kTile;
#pragma unroll
        for (int r = 0; r < kTile; r++) {
          float v = acc[r] + bias;
          if (!head) v = v > 0.0f ? v : 0.0f;
          else if (net == 0) v = tanhf(v);
          y[r] = v;
        }
      }
    }
    cur ^= 1;
  }
  __syncthreads();
  const float *mean_s = xs[0][d->pol.n & 1];    // [component * kTile + robot]
  const float *value_s = xs[1][d->val.n & 1];   // [robot]
  // sample: thread r * act_dim + a, so that a tile's actions are one contiguous store
  if (tid < kTile * act_dim) {
    const int r = tid / act_dim, a = tid % act_dim, b = b0 + r;
    float e = 0.0f;
    if (b < B) {
      const float m = mean_s[a * kTile + r];
      float act = m;
      if (mode == RG_POLICY_MODE_SAMPLE) {
        e = noise_eps(d->seed, (unsigned long long)act_state[b], (unsigned long long)act_state[(size_t)B + b], (unsigned long long)a);
        const float se = expf(pp[d->logstd_off + a]) * e;
        act = m + se;
      }
      action[(size_t)b * act_dim + a] = act;
      if (mean) mean[(size_t)b * act_dim + a] = m;
    }
    eps_s[r * kMaxAct + a] = e;
  }
  __syncthreads();   // every counter has been read
  if (tid < kTile && b0 + tid < B) {
    const int b = b0 + tid;
    if (logprob) {
      double s = 0.0, sl = 0.0;
      for (int a = 0; a < act_dim; a++) {
        const double e = (double)eps_s[tid * kMaxAct + a];
        s = s + e * e;
        sl = sl + (double)pp[d->logstd_off + a];
      }
      logprob[b] = (float)(-0.5 * s - sl - 0.5 * (double)act_dim * 1.8378770664093453);   // ln(2 pi)
    }
    if (value) value[b] = value_s[tid];
    if (mode == RG_POLICY_MODE_SAMPLE) act_state[(size_t)B + b] = act_state[(size_t)B + b] + 1;
  }
}

// ---- record ---------------------------------------------------------------------------------------------------------

struct RecCfg {
  int B, obs_dim, G;
};

// part[col][g][kParts]: the sum over g of entry k, thread g holding workgroup g's partial
__device__ __forceinline__ double finish_sum(const double *__restrict__ part, int col, int G, int k, double *sh) {
  const int t = threadIdx.x;
  return block_sum(t < G ? part[((size_t)col * G + t) * kParts + k] : 0.0, sh);
}

__device__ __forceinline__ double new_mean_of(double count_after, double mu, double s1, double sv) {
  return count_after > 1.0 ? mu + s1 / count_after : sv;   // count has become 1: the one value itself
}

__global__ void __launch_bounds__(kRed) rg_policy_record_first_kernel(const RecCfg c, const float *__restrict__ obs, const float *__restrict__ reward,
                                                                      const int *__restrict__ done, const int *__restrict__ mask,
                                                                      const double *__restrict__ norm, float *__restrict__ ro_obs,
                                                                      float *__restrict__ ro_reward, int *__restrict__ ro_done,
                                                                      double *__restrict__ part) {
  __shared__ double sh[4];
  const int col = blockIdx.y, g = blockIdx.x;
  const bool is_reward = col == c.obs_dim;   // uniform over the workgroup
  const float *__restrict__ src = is_reward ? reward : obs + (size_t)col * c.B;
  float *__restrict__ dst = is_reward ? ro_reward : (ro_obs ? ro_obs + (size_t)col * c.B : nullptr);
  const double mu = norm[kCols + (is_reward ? kRewardCol : col)];
  double n = 0.0, s1 = 0.0, sv = 0.0;
  for (int b = g * kRed + (int)threadIdx.x; b < c.B; b += c.G * kRed) {
    const float x = src[b];
    if (dst) dst[b] = x;
    if (is_reward && ro_done) ro_done[b] = done[b];
    if (mask == nullptr || mask[b] != 0) {
      const double v = (double)x;
      n = n + 1.0;
      s1 = s1 + (v - mu);
      sv = sv + v;
    }
  }
  n = block_sum(n, sh);
  s1 = block_sum(s1, sh);
  sv = block_sum(sv, sh);
  if (threadIdx.x == 0) {
    double *p = part + ((size_t)col * c.G + g) * kParts;
    p[0] = n; p[1] = s1; p[2] = sv;
  }
}

__global__ void __launch_bounds__(kRed) rg_policy_record_second_kernel(const RecCfg c, const float *__restrict__ obs, const float *__restrict__ reward,
                                                                       const int *__restrict__ mask, const double *__restrict__ norm,
                                                                       double *__restrict__ part) {
  __shared__ double sh[4];
  const int col = blockIdx.y, g = blockIdx.x;
  const bool is_reward = col == c.obs_dim;
  const int ncol = is_reward ? kRewardCol : col;
  const float *__restrict__ src = is_reward ? reward : obs + (size_t)col * c.B;
  const double n = finish_sum(part, col, c.G, 0, sh);
  const double s1 = finish_sum(part, col, c.G, 1, sh);
  const double sv = finish_sum(part, col, c.G, 2, sh);
  const double mu = norm[kCols + ncol];
  const double nm = new_mean_of(norm[ncol] + n, mu, s1, sv);
  double s2 = 0.0;
  if (n > 0.0) {   // uniform over the workgroup
    for (int b = g * kRed + (int)threadIdx.x; b < c.B; b += c.G * kRed) {
      if (mask == nullptr || mask[b] != 0) {
        const double v = (double)src[b];
        s2 = s2 + (v - mu) * (v - nm);
      }
    }
  }
  s2 = block_sum(s2, sh);
  if (threadIdx.x == 0) part[((size_t)col * c.G + g) * kParts + 3] = s2;
}

__global__ void __launch_bounds__(kRed) rg_policy_record_finish_kernel(const RecCfg c, double *__restrict__ norm, const double *__restrict__ part) {
  __shared__ double sh[4];
  const int col = blockIdx.x;
  const int ncol = col == c.obs_dim ? kRewardCol : col;
  const double n = finish_sum(part, col, c.G, 0, sh);
  const double s1 = finish_sum(part, col, c.G, 1, sh);
  const double sv = finish_sum(part, col, c.G, 2, sh);
  const double s2 = finish_sum(part, col, c.G, 3, sh);
  if (threadIdx.x == 0 && n > 0.0) {
    const double count = norm[ncol] + n;
    norm[kCols + ncol] = new_mean_of(count, norm[kCols + ncol], s1, sv);
    norm[2 * kCols + ncol] = norm[2 * kCols + ncol] + s2;
    norm[ncol] = count;
  }
}

// ---- returns --------------------------------------------------------------------------------------------------------

struct RetCfg {
  int B, T, bootstrap;
  double discount, lambda, reward_clip;
};

__global__ void __launch_bounds__(kRed) rg_policy_returns_kernel(const RetCfg c, const float *__restrict__ reward, const float *__restrict__ value,
                                                                 const int *__restrict__ done, const float *__restrict__ last_value,
                                                                 const double *__restrict__ norm, float *__restrict__ ret, float *__restrict__ adv) {
  const int b = blockIdx.x * kRed + threadIdx.x;
  if (b >= c.B) return;
  const double scale = norm_scale(norm[kRewardCol], norm[2 * kCols + kRewardCol]);
  double vnext = c.bootstrap ? (double)last_value[b] : 0.0, anext = 0.0;
  for (int t = c.T - 1; t >= 0; t--) {
    const size_t k = (size_t)t * c.B + b;
    const double rp = clip_sym((double)reward[k] / scale, c.reward_clip);
    const double nd = done[k] != 0 ? 0.0 : 1.0;
    const double v = (double)value[k];
    const double delta = rp + c.discount * nd * vnext - v;
    const double a = delta + c.discount * c.lambda * nd * anext;
    adv[k] = (float)a;
    ret[k] = (float)(a + v);
    vnext = v;
    anext = a;
  }
}

thread_local std::string g_create_err;

}  // namespace

struct rg_policy_handle {
  rg_policy_config cfg{};
  rg_policy_layout lay{};
  ActDev dv{};
  int B = 0, device = 0, G = 0;
  ActDev *dev_cfg = nullptr;
  double *part = nullptr;   // [obs_dim + 1][G][kParts]
  std::string err;
};

namespace {

bool validate(const rg_policy_config *cfg, std::string &err) {
  const RealField reals[] = {{"reward_clip", &cfg->reward_clip, 1, kNonNegative}, {"discount", &cfg->discount, 1, kUnit}, {"gae_lambda", &cfg->gae_lambda, 1, kUnit}};
  return check_policy_config("config.", cfg, err) && check_reals("config.", reals, err);
}

void fill_layout(const rg_policy_config *cfg, rg_policy_layout &L) {
  std::memset(&L, 0, sizeof(L));
  L.n_policy = cfg->n_policy_layers + 1;
  L.logstd_offset = layer_layout(cfg->obs_dim, cfg->policy_layers, cfg->n_policy_layers, cfg->act_dim, L.policy_in, L.policy_out, L.policy_w, L.policy_b);
  L.policy_count = L.logstd_offset + cfg->act_dim;
  L.n_value = cfg->n_value_layers + 1;
  L.value_count = layer_layout(cfg->obs_dim, cfg->value_layers, cfg->n_value_layers, 1, L.value_in, L.value_out, L.value_w, L.value_b);
}

int hip_fail(rg_policy_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_POLICY_ERR_HIP, what, e); }
int no_device(rg_policy_handle *h) { return no_device(h, RG_POLICY_ERR_NO_DEVICE, "RG_POLICY"); }
int launch_status(rg_policy_handle *h, const char *what) { return launch_status(h, RG_POLICY_ERR_HIP, what); }

}  // namespace

extern "C" {

int32_t rg_policy_abi_version(void) { return RG_POLICY_ABI_VERSION; }
int32_t rg_policy_config_size(void) { return (int32_t)sizeof(rg_policy_config); }
int32_t rg_policy_layout_size(void) { return (int32_t)sizeof(rg_policy_layout); }
int32_t rg_policy_norm_rows(void) { return RG_POLICY_NORM_ROWS; }
int32_t rg_policy_tile(void) { return RG_POLICY_TILE; }
const char *rg_policy_last_error(const rg_policy_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_policy_param_layout(const rg_policy_config *cfg, rg_policy_layout *out) {
  if (!cfg || !out) { g_create_err = "param_layout: null config or out"; return RG_POLICY_ERR_INVALID; }
  std::string err;
  if (!validate(cfg, err)) { g_create_err = err; return RG_POLICY_ERR_INVALID; }
  fill_layout(cfg, *out);
  return RG_POLICY_OK;
}

int rg_policy_create(const rg_policy_config *cfg, int32_t batch, int32_t device, rg_policy_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_POLICY_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!check_batch(batch, RG_POLICY_MAX_BATCH, err) || !validate(cfg, err)) { g_create_err = err; return RG_POLICY_ERR_INVALID; }
  rg_policy_handle *h = new rg_policy_handle();
  h->cfg = *cfg;
  h->B = batch;
  h->device = device;
  h->G = (batch + kRed - 1) / kRed;
  if (h->G > kMaxGroups) h->G = kMaxGroups;
  fill_layout(cfg, h->lay);
  ActDev &d = h->dv;
  d.B = batch; d.obs_dim = cfg->obs_dim; d.act_dim = cfg->act_dim; d.logstd_off = h->lay.logstd_offset;
  d.obs_clip = cfg->obs_clip; d.seed = cfg->seed;
  d.pol.n = h->lay.n_policy; d.val.n = h->lay.n_value;
  for (int l = 0; l < 4; l++) {
    d.pol.in[l] = h->lay.policy_in[l]; d.pol.out[l] = h->lay.policy_out[l]; d.pol.w[l] = h->lay.policy_w[l]; d.pol.b[l] = h->lay.policy_b[l];
    d.val.in[l] = h->lay.value_in[l]; d.val.out[l] = h->lay.value_out[l]; d.val.w[l] = h->lay.value_w[l]; d.val.b[l] = h->lay.value_b[l];
  }
  if (device == RG_POLICY_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_POLICY_OK;
  }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_POLICY_ERR_NO_DEVICE, RG_POLICY_ERR_INVALID, RG_POLICY_ERR_HIP, g_create_err)) { delete h; return rc; }
  hipError_t e = hipMalloc((void **)&h->dev_cfg, sizeof(ActDev));
  if (e == hipSuccess) e = hipMalloc((void **)&h->part, sizeof(double) * (size_t)(cfg->obs_dim + 1) * h->G * kParts);
  if (e != hipSuccess) {
    g_create_err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
    rg_policy_destroy(h);
    return RG_POLICY_ERR_ALLOC;
  }
  e = hipMemcpy(h->dev_cfg, &h->dv, sizeof(ActDev), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    g_create_err = std::string("hipMemcpy failed: ") + hipGetErrorString(e);
    rg_policy_destroy(h);
    return RG_POLICY_ERR_HIP;
  }
  *out = h;
  return RG_POLICY_OK;
}

void rg_policy_destroy(rg_policy_handle *h) {
  if (!h) return;
  if (h->device >= 0) {
    DeviceScope dev(h->device);
    if (h->dev_cfg) (void)hipFree(h->dev_cfg);
    if (h->part) (void)hipFree(h->part);
  }
  delete h;
}

int rg_policy_act(rg_policy_handle *h, const float *obs, const double *norm_state, const float *policy_params, const float *value_params,
                  int64_t *act_state, int32_t mode, float *action, float *mean, float *value, float *logprob, void *stream) {
  if (!h) { g_create_err = "act: null handle"; return RG_POLICY_ERR_INVALID; }
  if (!obs) { h->err = "act: null obs"; return RG_POLICY_ERR_INVALID; }
  if (!norm_state) { h->err = "act: null norm_state"; return RG_POLICY_ERR_INVALID; }
  if (!policy_params) { h->err = "act: null policy_params"; return RG_POLICY_ERR_INVALID; }
  if (!value_params) { h->err = "act: null value_params"; return RG_POLICY_ERR_INVALID; }
  if (mode != RG_POLICY_MODE_SAMPLE && mode != RG_POLICY_MODE_MEAN) { h->err = "act: mode is neither RG_POLICY_MODE_SAMPLE nor RG_POLICY_MODE_MEAN"; return RG_POLICY_ERR_INVALID; }
  if (!act_state && mode == RG_POLICY_MODE_SAMPLE) { h->err = "act: null act_state"; return RG_POLICY_ERR_INVALID; }
  if (!action) { h->err = "act: null action"; return RG_POLICY_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_policy_act_kernel, dim3(((unsigned)h->B + kTile - 1) / kTile), dim3(kActThreads), 0, (hipStream_t)stream, h->dev_cfg, obs,
                     norm_state, policy_params, value_params, (long long *)act_state, mode, action, mean, value, logprob);
  return launch_status(h, "rg_policy_act_kernel launch");
}

int rg_policy_record(rg_policy_handle *h, const float *obs, const float *reward, const int32_t *done, const int32_t *mask, double *norm_state,
                     float *ro_obs, float *ro_reward, int32_t *ro_done, void *stream) {
  if (!h) { g_create_err = "record: null handle"; return RG_POLICY_ERR_INVALID; }
  if (!obs) { h->err = "record: null obs"; return RG_POLICY_ERR_INVALID; }
  if (!reward) { h->err = "record: null reward"; return RG_POLICY_ERR_INVALID; }
  if (!done) { h->err = "record: null done"; return RG_POLICY_ERR_INVALID; }
  if (!norm_state) { h->err = "record: null norm_state"; return RG_POLICY_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  const RecCfg c{h->B, h->cfg.obs_dim, h->G};
  const dim3 grid((unsigned)h->G, (unsigned)(h->cfg.obs_dim + 1));
  hipLaunchKernelGGL(rg_policy_record_first_kernel, grid, dim3(kRed), 0, s, c, obs, reward, done, mask, norm_state, ro_obs, ro_reward, ro_done, h->part);
  int rc = launch_status(h, "rg_policy_record_first_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_policy_record_second_kernel, grid, dim3(kRed), 0, s, c, obs, reward, mask, norm_state, h->part);
  rc = launch_status(h, "rg_policy_record_second_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_policy_record_finish_kernel, dim3((unsigned)(h->cfg.obs_dim + 1)), dim3(kRed), 0, s, c, norm_state, h->part);
  return launch_status(h, "rg_policy_record_finish_kernel launch");
}

int rg_policy_returns(rg_policy_handle *h, const float *reward, const float *value, const int32_t *done, const float *last_value,
                      const double *norm_state, int32_t T, int32_t bootstrap, float *ret, float *adv, void *stream) {
  if (!h) { g_create_err = "returns: null handle"; return RG_POLICY_ERR_INVALID; }
  if (!reward) { h->err = "returns: null reward"; return RG_POLICY_ERR_INVALID; }
  if (!value) { h->err = "returns: null value"; return RG_POLICY_ERR_INVALID; }
  if (!done) { h->err = "returns: null done"; return RG_POLICY_ERR_INVALID; }
  if (!last_value && bootstrap) { h->err = "returns: null last_value"; return RG_POLICY_ERR_INVALID; }
  if (!norm_state) { h->err = "returns: null norm_state"; return RG_POLICY_ERR_INVALID; }
  if (T < 1 || T > RG_POLICY_MAX_T) {
    char msg[96];
    snprintf(msg, sizeof(msg), "returns: T %d outside [1, %d]", T, RG_POLICY_MAX_T);
    h->err = msg;
    return RG_POLICY_ERR_INVALID;
  }
  if (!ret) { h->err = "returns: null ret"; return RG_POLICY_ERR_INVALID; }
  if (!adv) { h->err = "returns: null adv"; return RG_POLICY_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const RetCfg c{h->B, T, bootstrap ? 1 : 0, h->cfg.discount, h->cfg.gae_lambda, h->cfg.reward_clip};
  hipLaunchKernelGGL(rg_policy_returns_kernel, dim3(((unsigned)h->B + kRed - 1) / kRed), dim3(kRed), 0, (hipStream_t)stream, c, reward, value, done,
                     last_value, norm_state, ret, adv);
  return launch_status(h, "rg_policy_returns_kernel launch");
}

}  // extern "C"
