// rg_ppo.hip -- the PPO update of include/rg_ppo.h.  Its own translation unit of librg_mpc.so.  A layer's forward and backward
// pass over a tile, the normaliser's arithmetic, the workgroup sums and the bodies of the transpose and slab-finish
// kernels and Adam's arithmetic are those of rg_agent_dev.inc, which the acting side includes too (so the forward pass gives
// rg_policy_act's mean to the bit from one text); the Gaussian head of a sample, the robot-KL element, the loss finish and
// the penalty rule are those of rg_ppo_dev.inc, which the recurrent update includes too; the host helpers are those of
// rg_host.h.  rg_mpc.hip includes none of them, so the source hash behind profiles/ is unaffected.
//
// Sweeps (rg_ppo_policy_forward_kernel, rg_ppo_policy_backward_kernel, rg_ppo_value_backward_kernel): G workgroups of 256
// threads, workgroup g walks the tiles g, g + G, ... of kTile samples.  LDS (dynamic): the tile's activations of every layer
// as a[layer][neuron * kTile + sample] (the normalised observation first) and two delta buffers of the widest layer, i.e.
// (obs_dim + sum(out) + 2 max(out)) * kTile floats: 45 KB at the defaults, 86 KB at the limits (64 -> 3 x 256 -> 4).
//   forward   thread j owns output neuron j: kTile accumulators, acc = fma(W[i][j], x[i][s], acc) for i in order; W read once
//             per (tile, neuron) coalesced along j, x as float4 broadcasts.
//   head      thread s < kTile owns sample s: float64 over the float32 mean (rg_ppo.h), delta rounded to float32;
//             gaussian_head of rg_ppo_dev.inc through TileHead, this file's view of a tile's sample.
//   backward  per layer, last to first: thread j folds sum_s x[i][s] delta[j][s] (an fma chain over s) into
//             slab[g][W[i][j]] for every i, coalesced along j -- the slab is the workgroup's own and each of its elements belongs
//             to one thread (which clears it first), so the running sum over the workgroup's tiles is plain loads and stores; thread i forms
//             dx[i][s] = sum_j Wt[j][i] delta[j][s] from the transposed copy, coalesced along i, and masks it by x[i][s] > 0.
// rg_ppo_grad_finish_kernel adds the G slabs per element in index order in float64; rg_ppo_loss_finish_kernel the float64
// partials of the loss and of the logstd gradient (a strided sum per thread, a shuffle tree, the four waves in order).
// The descriptors live in the workspace (rg_ppo_describe_kernel, first in every entry that sweeps) and are read with scalar loads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rg_ppo.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_agent_dev.inc"
#include "rg_ppo_dev.inc"

namespace {

constexpr int kTile = RG_PPO_TILE;
constexpr int kThreads = kAgentThreads;
constexpr int kMaxGroups = RG_PPO_MAX_GROUPS;
constexpr int kMaxAct = kHeadAct;
constexpr int kCols = RG_POLICY_NORM_COLS;
constexpr int kPart = kHeadPart;     // per (workgroup, lane): the loss sum, then the logstd gradient
constexpr int kPrep = 3;             // per workgroup of prepare: n, sum(adv), sum((adv - m)^2)
// dynamic LDS of a sweep at the widest configuration: (obs + three hidden layers + head + two delta buffers) * kTile floats
constexpr int kMaxLds = (RG_POLICY_MAX_OBS + RG_POLICY_MAX_LAYERS * RG_POLICY_MAX_WIDTH + RG_POLICY_MAX_ACT + 2 * RG_POLICY_MAX_WIDTH) * kTile * 4;
static_assert(kMaxLds == 86272 && kMaxLds <= 160 * 1024, "a sweep's tile fits a compute unit's LDS at every configuration");
constexpr int kScal = 8;             // workspace scalars: n (clamped), m, sd, n

static_assert(kTile == kAgentTile, "the sweeps run the shared layers, whose tile is four float4");
static_assert(RG_POLICY_MAX_WIDTH <= kThreads && RG_POLICY_MAX_OBS <= kThreads, "one neuron per thread");
static_assert(kMaxGroups <= kThreads, "finish_sum holds one workgroup's partial per thread");

struct SweepCfg {
  int T, B, N, G, ntiles;
  int obs_dim, act_dim, logstd_off, count;
  int asum, dmax;              // LDS: floats per sample of the activations, of one delta buffer
  double obs_clip, c, thr, coef;
  NetDesc nd;
};

struct RoDev {
  const float *obs, *action, *mean, *logstd, *adv, *ret;
  const int *mask;
};

struct Desc {                  // in the workspace: what a sweep reads of its call
  SweepCfg net[2];             // policy, value
  RoDev ro;
  const double *norm, *penalty;   // norm_state; the penalty of opt_state (NULL where the entry takes none)
  double *scal, *klr, *kls, *part;   // the workspace's regions
  float *wt, *slabs;
};

// ---- prepare --------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_ppo_prepare_first_kernel(const int N, const int GP, const float *__restrict__ adv,
                                                                        const int *__restrict__ mask, double *__restrict__ prep) {
  __shared__ double sh[4];
  double n = 0.0, s = 0.0;
  for (int k = blockIdx.x * kThreads + (int)threadIdx.x; k < N; k += GP * kThreads)
    if (mask[k] != 0) { n = n + 1.0; s = s + (double)adv[k]; }
  n = block_sum(n, sh);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) { prep[blockIdx.x * kPrep + 0] = n; prep[blockIdx.x * kPrep + 1] = s; }
}

__global__ void __launch_bounds__(kThreads) rg_ppo_prepare_second_kernel(const int N, const int GP, const float *__restrict__ adv,
                                                                         const int *__restrict__ mask, double *__restrict__ prep) {
  __shared__ double sh[4];
  const double n = strided_sum(prep + 0, GP, kPrep, sh);
  const double s = strided_sum(prep + 1, GP, kPrep, sh);
  const double m = s / (n > 1.0 ? n : 1.0);
  double q = 0.0;
  for (int k = blockIdx.x * kThreads + (int)threadIdx.x; k < N; k += GP * kThreads)
    if (mask[k] != 0) { const double d = (double)adv[k] - m; q = q + d * d; }
  q = block_sum(q, sh);
  if (threadIdx.x == 0) prep[blockIdx.x * kPrep + 2] = q;
}

__global__ void __launch_bounds__(kThreads) rg_ppo_prepare_finish_kernel(const int GP, const double *__restrict__ prep, double *__restrict__ scal) {
  __shared__ double sh[4];
  const double n = strided_sum(prep + 0, GP, kPrep, sh);
  const double s = strided_sum(prep + 1, GP, kPrep, sh);
  const double q = strided_sum(prep + 2, GP, kPrep, sh);
  if (threadIdx.x == 0) {
    const double nc = n > 1.0 ? n : 1.0;
    scal[0] = nc;
    scal[1] = s / nc;
    scal[2] = sqrt(q / nc) + 1e-8;
    scal[3] = n;
  }
}

// ---- the transposed copy of the weights -------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_ppo_transpose_kernel(const NetDesc nd, const float *__restrict__ P, float *__restrict__ Wt) {
  transpose_element(nd, P, Wt, blockIdx.x * kThreads + (int)threadIdx.x);
}

// the two descriptors and the rollout's pointers into the workspace, where the sweeps index them (dynamic indexing of a by-value kernel argument
// ends on the stack)
struct Regions {
  const double *norm, *penalty;
  double *scal, *klr, *kls, *part;
  float *wt, *slabs;
};

__global__ void rg_ppo_describe_kernel(const SweepCfg pol, const SweepCfg val, const RoDev ro, const Regions r, Desc *__restrict__ dst) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dst->net[0] = pol;
    dst->net[1] = val;
    dst->ro = ro;
    dst->norm = r.norm; dst->penalty = r.penalty;
    dst->scal = r.scal; dst->klr = r.klr; dst->kls = r.kls; dst->part = r.part;
    dst->wt = r.wt; dst->slabs = r.slabs;
  }
}

// ---- the sweeps -------------------------------------------------------------------------------------------------------

// gaussian_head's view of a sample of a tile: the new mean from the head's activations in LDS, out[k * kTile] (this thread's
// column), the delta into its column of the first delta buffer, the rest from the descriptor
struct TileHead {
  const Desc *dp;
  const SweepCfg &c;
  const float *out;
  float *d0;
  __device__ __forceinline__ const SweepCfg &cfg() const { return c; }
  __device__ __forceinline__ int mask(const int n) const { return dp->ro.mask[n]; }
  __device__ __forceinline__ float logstd0(const int k) const { return dp->ro.logstd[k]; }
  __device__ __forceinline__ float mean(const int, const int k) const { return out[k * kTile]; }
  __device__ __forceinline__ float mean0(const int n, const int k) const { return dp->ro.mean[(size_t)n * c.act_dim + k]; }
  __device__ __forceinline__ float action(const int n, const int k) const { return dp->ro.action[(size_t)n * c.act_dim + k]; }
  __device__ __forceinline__ float adv(const int n) const { return dp->ro.adv[n]; }
  __device__ __forceinline__ const double *scal() const { return dp->scal; }
  __device__ __forceinline__ double robot_kl(const int b) const { return dp->klr[b]; }
  __device__ __forceinline__ double penalty() const { return *dp->penalty; }
  __device__ __forceinline__ void keep_kl(const int n, const double v) const { dp->kls[n] = v; }
  __device__ __forceinline__ void keep_delta(const int, const int k, const float v) const { d0[k * kTile] = v; }
};

template <bool kPolicy, bool kBackward>
__device__ __forceinline__ void sweep(const Desc *__restrict__ dp, const float *__restrict__ P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, g = blockIdx.x;
  const SweepCfg &c = dp->net[kPolicy ? 0 : 1];
  const RoDev &ro = dp->ro;
  const double *__restrict__ norm = dp->norm;
  const float *__restrict__ Wt = dp->wt;
  const NetDesc &nd = c.nd;
  float *d0 = lds + c.asum * kTile, *d1 = d0 + c.dmax * kTile;
  float *slab = dp->slabs + (size_t)g * c.count;
  const double inv = 1.0 / ((double)c.T * (double)c.B);
  double loss = 0.0, gls[kMaxAct] = {0.0, 0.0, 0.0, 0.0};
  if (kBackward) {   // every element of the slab belongs to the thread that accumulates it: that thread clears it
    for (int l = 0; l < nd.n; l++) {
      if (tid < nd.out[l]) {
        slab[nd.b[l] + tid] = 0.0f;
        for (int i = 0; i < nd.in[l]; i++) slab[nd.w[l] + (size_t)i * nd.out[l] + tid] = 0.0f;
      }
    }
  }
  for (int tile = g; tile < c.ntiles; tile += c.G) {
    __syncthreads();   // the tile before has been read
    // the observation through the normaliser, as rg_policy_act forms it
    for (int idx = tid; idx < c.obs_dim * kTile; idx += kThreads) {
      const int i = idx / kTile, n = tile * kTile + idx % kTile;
      float xn = 0.0f;
      if (n < c.N) {
        const int t = n / c.B, b = n - t * c.B;
        double v = (double)ro.obs[((size_t)t * c.obs_dim + i) * c.B + b] - norm[kCols + i];
        v = v / norm_scale(norm[i], norm[2 * kCols + i]);
        xn = (float)clip_sym(v, c.obs_clip);
      }
      lds[idx] = xn;
    }
    int ao = 0;   // where the input of layer l lies
    for (int l = 0; l < nd.n; l++) {
      __syncthreads();
      const int an = ao + nd.in[l] * kTile;
      forward_layer(P, nd.in[l], nd.out[l], nd.w[l], nd.b[l], lds + ao, lds + an, l < nd.n - 1 ? 0 : (kPolicy ? 1 : 2));
      ao = an;
    }
    __syncthreads();
    // the head: one sample per thread
    if (tid < kTile) {
      const int n = tile * kTile + tid;
      const float *out = lds + c.asum * kTile - (kPolicy ? c.act_dim : 1) * kTile + tid;   // the head's activations, [k * kTile]
      const bool live = n < c.N;
      if (kPolicy) {
        gaussian_head<kBackward>(TileHead{dp, c, out, d0 + tid}, P, n, live, inv, loss, gls);
      } else {
        float dlt = 0.0f;
        if (live && ro.mask[n] != 0) {
          const double e = (double)ro.ret[n] - (double)out[0];
          loss = loss + 0.5 * (e * e);
          dlt = (float)(-e * inv);
        }
        d0[tid] = dlt;
      }
    }
    if (kBackward) {
      int cur = 0;
      for (int l = nd.n - 1; l >= 0; l--) {
        __syncthreads();
        ao -= nd.in[l] * kTile;
        const float *dl = cur ? d1 : d0;
        float *dn = cur ? d0 : d1;
        backward_weights(slab, nd.in[l], nd.out[l], nd.w[l], nd.b[l], lds + ao, dl);
        if (l > 0) backward_inputs(Wt, nd.in[l], nd.out[l], nd.w[l], lds + ao, dl, dn);
        cur ^= 1;
      }
    }
  }
  if (kBackward && tid < kTile) {
    double *p = dp->part + ((size_t)g * kTile + tid) * kPart;
    p[0] = loss;
#pragma unroll
    for (int k = 0; k < kMaxAct; k++) p[1 + k] = gls[k];
  }
}

__global__ void __launch_bounds__(kThreads) rg_ppo_policy_forward_kernel(const Desc *__restrict__ d, const float *__restrict__ P) {
  sweep<true, false>(d, P);
}

__global__ void __launch_bounds__(kThreads) rg_ppo_policy_backward_kernel(const Desc *__restrict__ d, const float *__restrict__ P) {
  sweep<true, true>(d, P);
}

__global__ void __launch_bounds__(kThreads) rg_ppo_value_backward_kernel(const Desc *__restrict__ d, const float *__restrict__ P) {
  sweep<false, true>(d, P);
}

// KL_b = (sum_t kls[t][b]) / T, t in order
__global__ void __launch_bounds__(kThreads) rg_ppo_robot_kl_kernel(const int T, const int B, const double *__restrict__ kls, double *__restrict__ out) {
  robot_kl_element(T, B, kls, out, blockIdx.x * kThreads + (int)threadIdx.x);
}

// grad[e] = (float) sum_g slab[g][e], g in order, for the first n elements (the networks; logstd is the loss kernel's)
__global__ void __launch_bounds__(kThreads) rg_ppo_grad_finish_kernel(const int n, const int count, const int G, const float *__restrict__ slabs,
                                                                      float *__restrict__ grad) {
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= n) return;
  grad[e] = slab_sum(slabs, count, G, e);
}

__global__ void __launch_bounds__(kThreads) rg_ppo_loss_finish_kernel(const LossCfg c, const double *__restrict__ part, const double *__restrict__ klr,
                                                                      const double *__restrict__ penalty, float *__restrict__ grad,
                                                                      double *__restrict__ loss_out, double *__restrict__ loss_out2) {
  __shared__ double sh[4];
  loss_finish(c, c.parts, c.policy != 0, part, klr, penalty, grad, loss_out, loss_out2, sh);
}

// ---- Adam -----------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_ppo_adam_kernel(const AdamCfg c, float *__restrict__ p, const float *__restrict__ grad,
                                                               float *__restrict__ m, float *__restrict__ v, const long long *__restrict__ step) {
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= c.count) return;
  const AdamBias bias = adam_bias(c, *step);
  adam_element(c, bias, grad[e], p, m, v, e);
}

__global__ void rg_ppo_adam_count_kernel(long long *__restrict__ step) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *step = *step + 1;
}

// ---- the penalty ------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_ppo_penalty_kernel(const int B, const double target, const int epochs_policy, const int epochs_value,
                                                                  const double *__restrict__ klr, double *__restrict__ penalty,
                                                                  double *__restrict__ stats) {
  __shared__ double sh[4];
  const double s = strided_sum(klr, B, 1, sh);
  if (threadIdx.x == 0) {
    const PenaltyMove mv = move_penalty(s, B, target, penalty);
    *penalty = mv.penalty;
    stats[4] = mv.change;
    stats[5] = mv.penalty;
    if (epochs_policy == 0) stats[0] = stats[1] = nan("");
    if (epochs_value == 0) stats[2] = stats[3] = nan("");
  }
}

thread_local std::string g_create_err;

}  // namespace

struct rg_ppo_handle {
  rg_policy_config pcfg{};
  rg_ppo_config cfg{};
  SweepCfg pol{}, val{};
  int T = 0, B = 0, N = 0, G = 0, GP = 0, device = 0, maxc = 0;
  size_t lds_pol = 0, lds_val = 0;
  // byte offsets into the workspace
  size_t o_desc = 0, o_scal = 0, o_prep = 0, o_klr = 0, o_kls = 0, o_part = 0, o_grad = 0, o_wt = 0, o_slab = 0, ws_bytes = 0, opt_bytes = 0;
  std::string err;
};

namespace {

int hip_fail(rg_ppo_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_PPO_ERR_HIP, what, e); }
int no_device(rg_ppo_handle *h) { return no_device(h, RG_PPO_ERR_NO_DEVICE, "RG_PPO"); }
int launch_status(rg_ppo_handle *h, const char *what) { return launch_status(h, RG_PPO_ERR_HIP, what); }
int null_arg(rg_ppo_handle *h, const char *call, const char *name) { return null_arg(h, RG_PPO_ERR_INVALID, call, name); }

RoDev ro_dev(const rg_ppo_rollout *ro) { return RoDev{ro->obs, ro->action, ro->mean, ro->logstd, ro->adv, ro->ret, (const int *)ro->mask}; }

double *penalty_of(void *opt_state) { return reinterpret_cast<double *>(static_cast<char *>(opt_state) + 16); }
const double *penalty_of(const void *opt_state) { return reinterpret_cast<const double *>(static_cast<const char *>(opt_state) + 16); }

unsigned blocks_of(int n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// ---- the launches of each entry, arguments checked and the device set by the caller ------------------------------------

int run_describe(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm, const void *opt, void *ws, hipStream_t s) {
  const Regions r{norm, opt ? penalty_of(opt) : nullptr, ws_at<double>(ws, h->o_scal), ws_at<double>(ws, h->o_klr), ws_at<double>(ws, h->o_kls),
                  ws_at<double>(ws, h->o_part), ws_at<float>(ws, h->o_wt), ws_at<float>(ws, h->o_slab)};
  hipLaunchKernelGGL(rg_ppo_describe_kernel, dim3(1), dim3(64), 0, s, h->pol, h->val, ro_dev(ro), r, ws_at<Desc>(ws, h->o_desc));
  return launch_status(h, "rg_ppo_describe_kernel launch");
}

int run_prepare(rg_ppo_handle *h, const rg_ppo_rollout *ro, void *ws, hipStream_t s) {
  double *prep = ws_at<double>(ws, h->o_prep), *scal = ws_at<double>(ws, h->o_scal);
  hipLaunchKernelGGL(rg_ppo_prepare_first_kernel, dim3((unsigned)h->GP), dim3(kThreads), 0, s, h->N, h->GP, ro->adv, (const int *)ro->mask, prep);
  int rc = launch_status(h, "rg_ppo_prepare_first_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ppo_prepare_second_kernel, dim3((unsigned)h->GP), dim3(kThreads), 0, s, h->N, h->GP, ro->adv, (const int *)ro->mask, prep);
  rc = launch_status(h, "rg_ppo_prepare_second_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ppo_prepare_finish_kernel, dim3(1), dim3(kThreads), 0, s, h->GP, prep, scal);
  return launch_status(h, "rg_ppo_prepare_finish_kernel launch");
}

int run_robot_kl(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm, const float *pp, void *ws, double *kl_out, hipStream_t s) {
  double *kls = ws_at<double>(ws, h->o_kls);
  hipLaunchKernelGGL(rg_ppo_policy_forward_kernel, dim3((unsigned)h->G), dim3(kThreads), h->lds_pol, s, ws_at<const Desc>(ws, h->o_desc), pp);
  int rc = launch_status(h, "rg_ppo_policy_forward_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ppo_robot_kl_kernel, dim3(blocks_of(h->B)), dim3(kThreads), 0, s, h->T, h->B, kls, kl_out);
  return launch_status(h, "rg_ppo_robot_kl_kernel launch");
}

int run_finish(rg_ppo_handle *h, bool policy, const double *penalty, void *ws, float *grad, double *loss_out, double *loss_out2, hipStream_t s) {
  const SweepCfg &c = policy ? h->pol : h->val;
  const int n = policy ? c.logstd_off : c.count;
  hipLaunchKernelGGL(rg_ppo_grad_finish_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, n, c.count, h->G, ws_at<float>(ws, h->o_slab), grad);
  int rc = launch_status(h, "rg_ppo_grad_finish_kernel launch");
  if (rc) return rc;
  const LossCfg lc{h->T, h->B, h->G * kTile, c.act_dim, c.logstd_off, policy ? 1 : 0, c.thr, c.coef};
  hipLaunchKernelGGL(rg_ppo_loss_finish_kernel, dim3(1), dim3(kThreads), 0, s, lc, ws_at<double>(ws, h->o_part), ws_at<double>(ws, h->o_klr), penalty,
                     grad, loss_out, loss_out2);
  return launch_status(h, "rg_ppo_loss_finish_kernel launch");
}

int run_policy_grad(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm, const float *pp, const void *opt, void *ws, float *grad,
                    double *loss_out, double *loss_out2, hipStream_t s) {
  float *wt = ws_at<float>(ws, h->o_wt);
  hipLaunchKernelGGL(rg_ppo_transpose_kernel, dim3(blocks_of(h->pol.count)), dim3(kThreads), 0, s, h->pol.nd, pp, wt);
  int rc = launch_status(h, "rg_ppo_transpose_kernel launch");
  if (rc) return rc;
  double *klr = ws_at<double>(ws, h->o_klr);
  rc = run_robot_kl(h, ro, norm, pp, ws, klr, s);
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ppo_policy_backward_kernel, dim3((unsigned)h->G), dim3(kThreads), h->lds_pol, s, ws_at<const Desc>(ws, h->o_desc), pp);
  rc = launch_status(h, "rg_ppo_policy_backward_kernel launch");
  if (rc) return rc;
  return run_finish(h, true, penalty_of(opt), ws, grad, loss_out, loss_out2, s);
}

int run_value_grad(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm, const float *vp, void *ws, float *grad, double *loss_out,
                   double *loss_out2, hipStream_t s) {
  float *wt = ws_at<float>(ws, h->o_wt);
  hipLaunchKernelGGL(rg_ppo_transpose_kernel, dim3(blocks_of(h->val.count)), dim3(kThreads), 0, s, h->val.nd, vp, wt);
  int rc = launch_status(h, "rg_ppo_transpose_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ppo_value_backward_kernel, dim3((unsigned)h->G), dim3(kThreads), h->lds_val, s, ws_at<const Desc>(ws, h->o_desc), vp);
  rc = launch_status(h, "rg_ppo_value_backward_kernel launch");
  if (rc) return rc;
  return run_finish(h, false, nullptr, ws, grad, loss_out, loss_out2, s);
}

int run_adam(rg_ppo_handle *h, int which, float *params, const float *grad, void *opt, hipStream_t s) {
  const int pc = h->pol.count, vc = h->val.count;
  const int count = which == RG_PPO_POLICY ? pc : vc;
  float *mom = reinterpret_cast<float *>(static_cast<char *>(opt) + RG_PPO_OPT_HEADER_BYTES);
  float *m = which == RG_PPO_POLICY ? mom : mom + 2 * (size_t)pc;
  long long *step = reinterpret_cast<long long *>(opt) + which;
  const AdamCfg c{count, 0, which == RG_PPO_POLICY ? h->cfg.policy_lr : h->cfg.value_lr, h->cfg.beta1, h->cfg.beta2, h->cfg.adam_eps};
  hipLaunchKernelGGL(rg_ppo_adam_kernel, dim3(blocks_of(count)), dim3(kThreads), 0, s, c, params, grad, m, m + count, (const long long *)step);
  int rc = launch_status(h, "rg_ppo_adam_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ppo_adam_count_kernel, dim3(1), dim3(64), 0, s, step);
  return launch_status(h, "rg_ppo_adam_count_kernel launch");
}

int check_rollout(rg_ppo_handle *h, const char *call, const rg_ppo_rollout *ro, bool obs, bool action, bool mean, bool adv, bool ret) {
  RG_NEED(call, ro, "rollout");
  if (obs) RG_NEED(call, ro->obs, "rollout.obs");
  if (action) RG_NEED(call, ro->action, "rollout.action");
  if (mean) { RG_NEED(call, ro->mean, "rollout.mean"); RG_NEED(call, ro->logstd, "rollout.logstd"); }
  if (adv) RG_NEED(call, ro->adv, "rollout.adv");
  if (ret) RG_NEED(call, ro->ret, "rollout.ret");
  RG_NEED(call, ro->mask, "rollout.mask");
  return RG_PPO_OK;
}

}  // namespace

extern "C" {

int32_t rg_ppo_abi_version(void) { return RG_PPO_ABI_VERSION; }
int32_t rg_ppo_config_size(void) { return (int32_t)sizeof(rg_ppo_config); }
int32_t rg_ppo_rollout_size(void) { return (int32_t)sizeof(rg_ppo_rollout); }
int32_t rg_ppo_tile(void) { return RG_PPO_TILE; }
const char *rg_ppo_last_error(const rg_ppo_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }
int64_t rg_ppo_workspace_bytes(const rg_ppo_handle *h) { return h ? (int64_t)h->ws_bytes : -1; }
int64_t rg_ppo_opt_state_bytes(const rg_ppo_handle *h) { return h ? (int64_t)h->opt_bytes : -1; }
int32_t rg_ppo_groups(const rg_ppo_handle *h) { return h ? h->G : -1; }
int64_t rg_ppo_scalars_offset(const rg_ppo_handle *h) { return h ? (int64_t)h->o_scal : -1; }

int rg_ppo_create(const rg_policy_config *policy_cfg, const rg_ppo_config *ppo_cfg, int32_t T, int32_t B, int32_t device, rg_ppo_handle **out) {
  if (!policy_cfg || !ppo_cfg || !out) { g_create_err = "create: null policy_cfg, ppo_cfg or out"; return RG_PPO_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  const IntField sizes[] = {{"T", T, 1, RG_POLICY_MAX_T}, {"B", B, 1, RG_POLICY_MAX_BATCH}};
  if (!check_policy_config("policy_cfg.", policy_cfg, err) || !check_ppo_config(ppo_cfg, err) || !check_ints("", sizes, err) || !check_samples(T, B, err)) {
    g_create_err = err;
    return RG_PPO_ERR_INVALID;
  }
  rg_ppo_handle *h = new rg_ppo_handle();
  h->pcfg = *policy_cfg;
  h->cfg = *ppo_cfg;
  h->T = T; h->B = B; h->N = T * B; h->device = device;
  const int ntiles = (h->N + kTile - 1) / kTile;
  h->G = ntiles < kMaxGroups ? ntiles : kMaxGroups;
  h->GP = (h->N + kThreads - 1) / kThreads;
  if (h->GP > kMaxGroups) h->GP = kMaxGroups;
  for (int net = 0; net < 2; net++) {
    SweepCfg &c = net ? h->val : h->pol;
    c.nd.n = (net ? policy_cfg->n_value_layers : policy_cfg->n_policy_layers) + 1;
    c.count = layer_layout(policy_cfg->obs_dim, net ? policy_cfg->value_layers : policy_cfg->policy_layers, c.nd.n - 1, net ? 1 : policy_cfg->act_dim,
                           c.nd.in, c.nd.out, c.nd.w, c.nd.b);
    c.T = T; c.B = B; c.N = h->N; c.G = h->G; c.ntiles = ntiles;
    c.obs_dim = policy_cfg->obs_dim; c.act_dim = policy_cfg->act_dim;
    c.logstd_off = c.count;
    if (!net) c.count += policy_cfg->act_dim;
    c.asum = policy_cfg->obs_dim;
    c.dmax = 0;
    for (int l = 0; l < c.nd.n; l++) {
      c.asum += c.nd.out[l];
      if (c.nd.out[l] > c.dmax) c.dmax = c.nd.out[l];
    }
    c.obs_clip = policy_cfg->obs_clip;
    c.c = ppo_cfg->conv_logpdf == RG_PPO_LOGPDF_EXACT ? 1.0 : 0.5;
    c.thr = ppo_cfg->kl_target * ppo_cfg->kl_cutoff_factor;
    c.coef = ppo_cfg->kl_cutoff_coef;
    (net ? h->lds_val : h->lds_pol) = sizeof(float) * (size_t)kTile * (size_t)(c.asum + 2 * c.dmax);
  }
  h->maxc = h->pol.count > h->val.count ? h->pol.count : h->val.count;
  size_t off = 0;
  h->o_desc = off; off += round8(sizeof(Desc));
  h->o_scal = off; off += sizeof(double) * kScal;
  h->o_prep = off; off += sizeof(double) * (size_t)h->GP * kPrep;
  h->o_klr = off; off += sizeof(double) * (size_t)B;
  h->o_kls = off; off += sizeof(double) * (size_t)h->N;
  h->o_part = off; off += sizeof(double) * (size_t)h->G * kTile * kPart;
  h->o_grad = off; off += round8(sizeof(float) * (size_t)h->maxc);
  h->o_wt = off; off += round8(sizeof(float) * (size_t)h->maxc);
  h->o_slab = off; off += round8(sizeof(float) * (size_t)h->G * (size_t)h->maxc);
  h->ws_bytes = off;
  h->opt_bytes = round8(RG_PPO_OPT_HEADER_BYTES + sizeof(float) * 2 * ((size_t)h->pol.count + (size_t)h->val.count));
  if (device == RG_PPO_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_PPO_OK;
  }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_PPO_ERR_NO_DEVICE, RG_PPO_ERR_INVALID, RG_PPO_ERR_HIP, g_create_err)) { delete h; return rc; }
  // the sweeps' tiles may need more dynamic LDS than the default limit of a launch.  The attribute belongs to the function and
  // the device, not to the handle: it is set to the most any configuration of the ABI needs, so handles do not undo each other
  hipError_t e = hipFuncSetAttribute((const void *)rg_ppo_policy_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)rg_ppo_policy_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)rg_ppo_value_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
  if (e != hipSuccess) {
    g_create_err = std::string("hipFuncSetAttribute failed: ") + hipGetErrorString(e);
    delete h;
    return RG_PPO_ERR_HIP;
  }
  *out = h;
  return RG_PPO_OK;
}

void rg_ppo_destroy(rg_ppo_handle *h) { delete h; }

int rg_ppo_prepare(rg_ppo_handle *h, const rg_ppo_rollout *ro, void *workspace, void *stream) {
  if (!h) { g_create_err = "prepare: null handle"; return RG_PPO_ERR_INVALID; }
  int rc = check_rollout(h, "prepare", ro, false, false, false, true, false);
  if (rc) return rc;
  RG_NEED("prepare", workspace, "workspace");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_prepare(h, ro, workspace, (hipStream_t)stream);
}

int rg_ppo_policy_grad(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm_state, const float *policy_params, const void *opt_state,
                       void *workspace, float *grad_out, double *loss_out, void *stream) {
  if (!h) { g_create_err = "policy_grad: null handle"; return RG_PPO_ERR_INVALID; }
  int rc = check_rollout(h, "policy_grad", ro, true, true, true, true, false);
  if (rc) return rc;
  RG_NEED("policy_grad", norm_state, "norm_state");
  RG_NEED("policy_grad", policy_params, "policy_params");
  RG_NEED("policy_grad", opt_state, "opt_state");
  RG_NEED("policy_grad", workspace, "workspace");
  RG_NEED("policy_grad", grad_out, "grad_out");
  RG_NEED("policy_grad", loss_out, "loss_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  rc = run_describe(h, ro, norm_state, opt_state, workspace, (hipStream_t)stream);
  if (rc) return rc;
  return run_policy_grad(h, ro, norm_state, policy_params, opt_state, workspace, grad_out, loss_out, nullptr, (hipStream_t)stream);
}

int rg_ppo_value_grad(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm_state, const float *value_params, void *workspace,
                      float *grad_out, double *loss_out, void *stream) {
  if (!h) { g_create_err = "value_grad: null handle"; return RG_PPO_ERR_INVALID; }
  int rc = check_rollout(h, "value_grad", ro, true, false, false, false, true);
  if (rc) return rc;
  RG_NEED("value_grad", norm_state, "norm_state");
  RG_NEED("value_grad", value_params, "value_params");
  RG_NEED("value_grad", workspace, "workspace");
  RG_NEED("value_grad", grad_out, "grad_out");
  RG_NEED("value_grad", loss_out, "loss_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  rc = run_describe(h, ro, norm_state, nullptr, workspace, (hipStream_t)stream);
  if (rc) return rc;
  return run_value_grad(h, ro, norm_state, value_params, workspace, grad_out, loss_out, nullptr, (hipStream_t)stream);
}

int rg_ppo_adam(rg_ppo_handle *h, int32_t which, float *params, const float *grad, void *opt_state, void *stream) {
  if (!h) { g_create_err = "adam: null handle"; return RG_PPO_ERR_INVALID; }
  if (which != RG_PPO_POLICY && which != RG_PPO_VALUE) { h->err = "adam: which is neither RG_PPO_POLICY nor RG_PPO_VALUE"; return RG_PPO_ERR_INVALID; }
  RG_NEED("adam", params, "params");
  RG_NEED("adam", grad, "grad");
  RG_NEED("adam", opt_state, "opt_state");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_adam(h, which, params, grad, opt_state, (hipStream_t)stream);
}

int rg_ppo_kl(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm_state, const float *policy_params, void *workspace, double *kl_out,
              void *stream) {
  if (!h) { g_create_err = "kl: null handle"; return RG_PPO_ERR_INVALID; }
  int rc = check_rollout(h, "kl", ro, true, false, true, false, false);
  if (rc) return rc;
  RG_NEED("kl", norm_state, "norm_state");
  RG_NEED("kl", policy_params, "policy_params");
  RG_NEED("kl", workspace, "workspace");
  RG_NEED("kl", kl_out, "kl_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  rc = run_describe(h, ro, norm_state, nullptr, workspace, (hipStream_t)stream);
  if (rc) return rc;
  return run_robot_kl(h, ro, norm_state, policy_params, workspace, kl_out, (hipStream_t)stream);
}

int rg_ppo_update(rg_ppo_handle *h, const rg_ppo_rollout *ro, const double *norm_state, float *policy_params, float *value_params, void *opt_state,
                  void *workspace, double *stats, void *stream) {
  if (!h) { g_create_err = "update: null handle"; return RG_PPO_ERR_INVALID; }
  int rc = check_rollout(h, "update", ro, true, true, true, true, true);
  if (rc) return rc;
  RG_NEED("update", norm_state, "norm_state");
  RG_NEED("update", policy_params, "policy_params");
  RG_NEED("update", value_params, "value_params");
  RG_NEED("update", opt_state, "opt_state");
  RG_NEED("update", workspace, "workspace");
  RG_NEED("update", stats, "stats");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  float *grad = ws_at<float>(workspace, h->o_grad);
  rc = run_describe(h, ro, norm_state, opt_state, workspace, s);
  if (!rc) rc = run_prepare(h, ro, workspace, s);
  for (int e = 0; e < h->cfg.epochs_policy && !rc; e++) {
    rc = run_policy_grad(h, ro, norm_state, policy_params, opt_state, workspace, grad, e == 0 ? stats + 0 : stats + 1, e == 0 ? stats + 1 : nullptr, s);
    if (!rc) rc = run_adam(h, RG_PPO_POLICY, policy_params, grad, opt_state, s);
  }
  for (int e = 0; e < h->cfg.epochs_value && !rc; e++) {
    rc = run_value_grad(h, ro, norm_state, value_params, workspace, grad, e == 0 ? stats + 2 : stats + 3, e == 0 ? stats + 3 : nullptr, s);
    if (!rc) rc = run_adam(h, RG_PPO_VALUE, value_params, grad, opt_state, s);
  }
  if (rc) return rc;
  double *klr = ws_at<double>(workspace, h->o_klr);
  rc = run_robot_kl(h, ro, norm_state, policy_params, workspace, klr, s);
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ppo_penalty_kernel, dim3(1), dim3(kThreads), 0, s, h->B, h->cfg.kl_target, h->cfg.epochs_policy, h->cfg.epochs_value,
                     (const double *)klr, penalty_of(opt_state), stats);
  return launch_status(h, "rg_ppo_penalty_kernel launch");
}

}  // extern "C"
