// rg_rnn.hip -- the recurrent Gaussian policy of include/rg_rnn.h: one tick (rg_rnn_act) and T ticks with the state kept on
// the chip (rg_rnn_unroll).  Its own translation unit of librg_mpc.so.  The noise stream, the normaliser's arithmetic and the
// layer descriptor are those of rg_agent_dev.inc, the tick (its tiling, its stages, the fmaf chain) that of rg_gru_dev.inc and
// the host helpers those of rg_host.h; rg_mpc.hip includes neither this file nor them, so the source hash behind profiles/ is
// unaffected.
//
// rg_rnn_act_kernel: 512 threads, threads 0..255 (waves 0..3) the policy's stages, threads 256..511 (waves 4..7) the value
// network's layers (rg_policy_act_kernel's neuron, so the value is that kernel's to the bit); every branch on the network is
// uniform over a wave and both halves meet at the same barriers.  A workgroup reads its robots' rows of hidden_in before
// the first barrier and writes hidden_out after it: hidden_out may be hidden_in.
// rg_rnn_unroll_kernel: 256 threads, the same gru_stage calls T times; h stays in LDS between ticks.
// LDS, floats: act (4 * RG_RNN_MAX_WIDTH + 3 * RG_RNN_MAX_UNITS + RG_RNN_MAX_ACT) * RG_RNN_TILE = 45184 bytes;
//              unroll (2 * RG_RNN_MAX_WIDTH + 3 * RG_RNN_MAX_UNITS) * RG_RNN_TILE = 28672 bytes, and its copy of the descriptor
//              (at most 256 bytes).
// The descriptor is read from device memory (dynamic indexing of a by-value kernel argument could end on the stack); the
// unroll kernel copies it to LDS first.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rg_policy.h"
#include "../../include/rg_rnn.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_agent_dev.inc"
#include "rg_gru_dev.inc"

namespace {

constexpr int kHalf = 256;
constexpr int kActThreads = 2 * kHalf;

static_assert(kHalf == kAgentThreads, "the workgroup that copies the descriptor");
static_assert(2 * kMaxH <= kHalf && kMaxW <= kHalf, "one output neuron per thread of the policy's half");
static_assert(kTile * kMaxAct <= 64 && kMaxAct <= kMaxW, "sampling thread map; the head's output fits an x buffer");
static_assert(RG_RNN_MODE_SAMPLE == RG_POLICY_MODE_SAMPLE && RG_RNN_MODE_MEAN == RG_POLICY_MODE_MEAN, "modes");

struct RnnDev {
  int B, obs_dim, act_dim, H, n_dense, n_x;
  int dense_in[2], dense_out[2], dense_w[2], dense_b[2];
  int w_ru, b_ru, w_c, b_c, head_w, head_b, logstd_off, pad0;
  double obs_clip;
  unsigned long long seed;
  NetDesc val;
};

// what the acting kernels keep of a tick: h' of the tile's robots from b0 on, in memory at hout_a and hout_b ([B][H] each,
// either may be null)
struct HiddenSink {
  const RnnDev *d;
  int b0;
  float *hout_a, *hout_b;
  __device__ __forceinline__ void dense(int, int, int, int, float) const {}
  __device__ __forceinline__ void reset_gate(int, int, int, float, float) const {}
  __device__ __forceinline__ void update_gate(int, int, int, float) const {}
  __device__ __forceinline__ void cell(const int H, const int j, const int r, float, const float hn) const {
    const int b = b0 + r;
    if (b < d->B) {
      if (hout_a) hout_a[(size_t)b * H + j] = hn;
      if (hout_b) hout_b[(size_t)b * H + j] = hn;
    }
  }
};

__global__ void __launch_bounds__(kActThreads) rg_rnn_act_kernel(const RnnDev *__restrict__ d, const float *__restrict__ obs,
                                                                 const double *__restrict__ norm, const float *__restrict__ pp,
                                                                 const float *__restrict__ vp, long long *__restrict__ act_state,
                                                                 const int *__restrict__ reset, const float *hidden_in, float *hidden_out,
                                                                 const int mode, float *__restrict__ action, float *__restrict__ mean,
                                                                 float *__restrict__ value, float *__restrict__ logprob) {
  __shared__ __attribute__((aligned(16))) float xp[2][kMaxW * kTile];   // the policy's x buffers, [input * kTile + robot]
  __shared__ __attribute__((aligned(16))) float xv[2][kMaxW * kTile];   // the value network's
  __shared__ __attribute__((aligned(16))) float hs[kMaxH * kTile];
  __shared__ __attribute__((aligned(16))) float rh[kMaxH * kTile];
  __shared__ __attribute__((aligned(16))) float us[kMaxH * kTile];
  __shared__ float eps_s[kTile * kMaxAct];
  const int tid = threadIdx.x;
  const int net = tid >> 8;          // uniform over a wave
  const int j = tid & (kHalf - 1);
  const int B = d->B, obs_dim = d->obs_dim, act_dim = d->act_dim, H = d->H;
  const int b0 = blockIdx.x * kTile;
  if (tid < obs_dim * kTile) {
    const int i = tid / kTile, r = tid % kTile, b = b0 + r;
    const float xn = b < B ? normalised(obs, norm, i, b, B, d->obs_clip) : 0.0f;
    xp[0][tid] = xn;
    xv[0][tid] = xn;
  }
  for (int idx = tid; idx < H * kTile; idx += kActThreads) {   // along j: a robot's row is read contiguously
    const int r = idx / H, k = idx - r * H, b = b0 + r;
    float h = 0.0f;
    if (b < B && !(reset && reset[b] != 0)) h = hidden_in[(size_t)b * H + k];
    hs[k * kTile + r] = h;
  }
  const int n_pol = d->n_dense + 3, n_val = d->val.n;
  const int n_max = n_pol > n_val ? n_pol : n_val;
  for (int s = 0; s < n_max; s++) {
    __syncthreads();
    if (net == 0) {
      if (s < n_pol) gru_stage(d, pp, s, j, xp, hs, rh, us, HiddenSink{d, b0, hidden_out, nullptr});
    } else if (s < n_val) {
      const int nin = d->val.in[s], nout = d->val.out[s];
      if (j < nout) {
        float acc[kTile];
#pragma unroll
        for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
        chain8(vp + d->val.w[s] + j, nout, xv[s & 1], nin, acc);
        const float bias = vp[d->val.b[s] + j];
        float *y = xv[(s & 1) ^ 1] + j * kTile;
#pragma unroll
        for (int r = 0; r < kTile; r++) {
          float v = acc[r] + bias;
          if (s < n_val - 1) v = v > 0.0f ? v : 0.0f;
          y[r] = v;
        }
      }
    }
  }
  __syncthreads();
  const float *mean_s = xp[(d->n_dense & 1) ^ 1];   // [component * kTile + robot]
  const float *value_s = xv[n_val & 1];             // [robot]
  // sample: thread r * act_dim + a, so that a tile's actions are one contiguous store (rg_policy_act_kernel's epilogue)
  if (tid < kTile * act_dim) {
    const int r = tid / act_dim, a = tid % act_dim, b = b0 + r;
    float e = 0.0f;
    if (b < B) {
      const float m = mean_s[a * kTile + r];
      float act = m;
      if (mode == RG_RNN_MODE_SAMPLE) {
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
    if (mode == RG_RNN_MODE_SAMPLE) act_state[(size_t)B + b] = act_state[(size_t)B + b] + 1;
  }
}

__global__ void __launch_bounds__(kHalf) rg_rnn_unroll_kernel(const RnnDev *__restrict__ dg, const float *__restrict__ obs,
                                                              const int *__restrict__ reset, const float *h0, const double *__restrict__ norm,
                                                              const float *__restrict__ pp, const int T, float *__restrict__ mean_out,
                                                              float *__restrict__ hidden_seq, float *hidden_last) {
  // the descriptor from LDS: as scalar registers its fields, live through the loop over t, do not fit beside the pointers
  __shared__ RnnDev dsh;
  const RnnDev *d = descriptor_to_lds(dg, &dsh);
  __shared__ __attribute__((aligned(16))) float xs[2][kMaxW * kTile];
  __shared__ __attribute__((aligned(16))) float hs[kMaxH * kTile];
  __shared__ __attribute__((aligned(16))) float rh[kMaxH * kTile];
  __shared__ __attribute__((aligned(16))) float us[kMaxH * kTile];
  const int tid = threadIdx.x;
  const int B = d->B, obs_dim = d->obs_dim, act_dim = d->act_dim, H = d->H;
  const int b0 = blockIdx.x * kTile;
  const int n_pol = d->n_dense + 3;
  const float *mean_s = xs[(d->n_dense & 1) ^ 1];
  for (int idx = tid; idx < H * kTile; idx += kHalf) {
    const int r = idx / H, k = idx - r * H, b = b0 + r;
    hs[k * kTile + r] = b < B ? h0[(size_t)b * H + k] : 0.0f;
  }
  for (int t = 0; t < T; t++) {
    const float *__restrict__ obs_t = obs + (size_t)t * obs_dim * B;
    const int *__restrict__ reset_t = reset + (size_t)t * B;
    for (int idx = tid; idx < obs_dim * kTile; idx += kHalf) {
      const int i = idx / kTile, r = idx % kTile, b = b0 + r;
      xs[0][idx] = b < B ? normalised(obs_t, norm, i, b, B, d->obs_clip) : 0.0f;
    }
    for (int idx = tid; idx < H * kTile; idx += kHalf) {   // the thread that wrote h0's element zeroes it
      const int r = idx / H, k = idx - r * H, b = b0 + r;
      if (b < B && reset_t[b] != 0) hs[k * kTile + r] = 0.0f;
    }
    float *hseq_t = hidden_seq ? hidden_seq + (size_t)t * B * H : nullptr;
    float *hlast = t == T - 1 ? hidden_last : nullptr;
    for (int s = 0; s < n_pol; s++) {
      __syncthreads();
      gru_stage(d, pp, s, tid, xs, hs, rh, us, HiddenSink{d, b0, hseq_t, hlast});
    }
    __syncthreads();
    if (tid < kTile * act_dim) {
      const int r = tid / act_dim, a = tid % act_dim, b = b0 + r;
      if (b < B) mean_out[((size_t)t * B + b) * act_dim + a] = mean_s[a * kTile + r];
    }
    __syncthreads();   // the next tick's observation may land in the buffer the mean was read from
  }
}

thread_local std::string g_create_err;

}  // namespace

struct rg_rnn_handle {
  rg_rnn_config cfg{};
  rg_rnn_layout lay{};
  RnnDev dv{};
  int B = 0, device = 0;
  RnnDev *dev_cfg = nullptr;
  std::string err;
};

namespace {

int hip_fail(rg_rnn_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_RNN_ERR_HIP, what, e); }
int no_device(rg_rnn_handle *h) { return no_device(h, RG_RNN_ERR_NO_DEVICE, "RG_RNN"); }
int launch_status(rg_rnn_handle *h, const char *what) { return launch_status(h, RG_RNN_ERR_HIP, what); }
int null_arg(rg_rnn_handle *h, const char *call, const char *name) { return null_arg(h, RG_RNN_ERR_INVALID, call, name); }

}  // namespace

extern "C" {

int32_t rg_rnn_abi_version(void) { return RG_RNN_ABI_VERSION; }
int32_t rg_rnn_config_size(void) { return (int32_t)sizeof(rg_rnn_config); }
int32_t rg_rnn_layout_size(void) { return (int32_t)sizeof(rg_rnn_layout); }
int32_t rg_rnn_tile(void) { return RG_RNN_TILE; }
const char *rg_rnn_last_error(const rg_rnn_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_rnn_param_layout(const rg_rnn_config *cfg, rg_rnn_layout *out) {
  if (!cfg || !out) { g_create_err = "param_layout: null config or out"; return RG_RNN_ERR_INVALID; }
  std::string err;
  if (!check_rnn_config("config.", cfg, err)) { g_create_err = err; return RG_RNN_ERR_INVALID; }
  fill_layout(cfg, *out);
  return RG_RNN_OK;
}

int rg_rnn_create(const rg_rnn_config *cfg, int32_t batch, int32_t device, rg_rnn_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_RNN_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!check_batch(batch, RG_RNN_MAX_BATCH, err) || !check_rnn_config("config.", cfg, err)) { g_create_err = err; return RG_RNN_ERR_INVALID; }
  rg_rnn_handle *h = new rg_rnn_handle();
  h->cfg = *cfg;
  h->B = batch;
  h->device = device;
  fill_layout(cfg, h->lay);
  const rg_rnn_layout &L = h->lay;
  RnnDev &d = h->dv;
  d.B = batch; d.obs_dim = cfg->obs_dim; d.act_dim = cfg->act_dim;
  layout_to_dev(L, d);
  d.obs_clip = cfg->obs_clip; d.seed = cfg->seed;
  d.val.n = L.n_value;
  for (int l = 0; l < 4; l++) { d.val.in[l] = L.value_in[l]; d.val.out[l] = L.value_out[l]; d.val.w[l] = L.value_w[l]; d.val.b[l] = L.value_b[l]; }
  if (device == RG_RNN_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_RNN_OK;
  }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_RNN_ERR_NO_DEVICE, RG_RNN_ERR_INVALID, RG_RNN_ERR_HIP, g_create_err)) { delete h; return rc; }
  hipError_t e = hipMalloc((void **)&h->dev_cfg, sizeof(RnnDev));
  if (e != hipSuccess) {
    g_create_err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
    rg_rnn_destroy(h);
    return RG_RNN_ERR_ALLOC;
  }
  e = hipMemcpy(h->dev_cfg, &h->dv, sizeof(RnnDev), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    g_create_err = std::string("hipMemcpy failed: ") + hipGetErrorString(e);
    rg_rnn_destroy(h);
    return RG_RNN_ERR_HIP;
  }
  *out = h;
  return RG_RNN_OK;
}

void rg_rnn_destroy(rg_rnn_handle *h) {
  if (!h) return;
  if (h->device >= 0) {
    DeviceScope dev(h->device);
    if (h->dev_cfg) (void)hipFree(h->dev_cfg);
  }
  delete h;
}

int rg_rnn_act(rg_rnn_handle *h, const float *obs, const double *norm_state, const float *policy_params, const float *value_params,
               int64_t *act_state, const int32_t *reset, const float *hidden_in, float *hidden_out, int32_t mode, float *action, float *mean,
               float *value, float *logprob, void *stream) {
  if (!h) { g_create_err = "act: null handle"; return RG_RNN_ERR_INVALID; }
  RG_NEED("act", obs, "obs");
  RG_NEED("act", norm_state, "norm_state");
  RG_NEED("act", policy_params, "policy_params");
  RG_NEED("act", value_params, "value_params");
  if (mode != RG_RNN_MODE_SAMPLE && mode != RG_RNN_MODE_MEAN) { h->err = "act: mode is neither RG_RNN_MODE_SAMPLE nor RG_RNN_MODE_MEAN"; return RG_RNN_ERR_INVALID; }
  if (!act_state && mode == RG_RNN_MODE_SAMPLE) return null_arg(h, "act", "act_state");
  RG_NEED("act", hidden_in, "hidden_in");
  RG_NEED("act", hidden_out, "hidden_out");
  RG_NEED("act", action, "action");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_rnn_act_kernel, dim3(((unsigned)h->B + kTile - 1) / kTile), dim3(kActThreads), 0, (hipStream_t)stream, h->dev_cfg, obs,
                     norm_state, policy_params, value_params, (long long *)act_state, reset, hidden_in, hidden_out, mode, action, mean, value,
                     logprob);
  return launch_status(h, "rg_rnn_act_kernel launch");
}

int rg_rnn_unroll(rg_rnn_handle *h, const float *obs, const int32_t *reset, const float *h0, const double *norm_state, const float *policy_params,
                  int32_t T, float *mean_out, float *hidden_seq, float *hidden_last, void *stream) {
  if (!h) { g_create_err = "unroll: null handle"; return RG_RNN_ERR_INVALID; }
  RG_NEED("unroll", obs, "obs");
  RG_NEED("unroll", reset, "reset");
  RG_NEED("unroll", h0, "h0");
  RG_NEED("unroll", norm_state, "norm_state");
  RG_NEED("unroll", policy_params, "policy_params");
  if (T < 1 || T > RG_RNN_MAX_T) {
    char msg[96];
    snprintf(msg, sizeof(msg), "unroll: T %d outside [1, %d]", T, RG_RNN_MAX_T);
    h->err = msg;
    return RG_RNN_ERR_INVALID;
  }
  RG_NEED("unroll", mean_out, "mean_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_rnn_unroll_kernel, dim3(((unsigned)h->B + kTile - 1) / kTile), dim3(kHalf), 0, (hipStream_t)stream, h->dev_cfg, obs, reset,
                     h0, norm_state, policy_params, T, mean_out, hidden_seq, hidden_last);
  return launch_status(h, "rg_rnn_unroll_kernel launch");
}

}  // extern "C"
