// rg_bptt.hip -- the recurrent PPO policy update of include/rg_bptt.h: back-propagation through time through the GRU cell of
// rg_rnn.h, with the head, Adam and the penalty rule of rg_ppo.h.  Its own translation unit of librg_mpc.so.  The normaliser's
// arithmetic, the workgroup sums, the transpose body and Adam's arithmetic are those of rg_agent_dev.inc; the Gaussian head of
// a sample, the robot-KL element, the loss finish and the penalty rule are those of rg_ppo_dev.inc, the text rg_ppo.hip runs
// (StoredHead is this file's view of a sample); the host helpers are those of rg_host.h.  rg_mpc.hip includes neither this
// file nor them, so the source hash behind profiles/ is unaffected.  The tick lives in
// rg_gru_dev.inc, which the acting kernels run too: the forward pass here is that code with a sink that keeps everything, so
// its means are the rollout's to the bit.
//
// One gradient is four kinds of launch (rg_bptt.h):
//   F  rg_bptt_forward_kernel: kTile robots per 256-thread workgroup through all T ticks, one output neuron per thread with
//      kTile accumulators, x, h, r*h and u in LDS as [input * kTile + robot]; every intermediate of every sample goes to the
//      workspace as [sample][neuron], coalesced along the neuron.
//   H  rg_bptt_sample_kl_kernel (a thread per sample), rg_bptt_robot_kl_kernel (a thread per robot), rg_bptt_head_kernel
//      (delta_mean per sample, the float64 partials of the loss and of the logstd gradient), rg_bptt_loss_finish_kernel.
//   B  rg_bptt_delta_kernel: the same tile of robots with t from T - 1 down to 0.  Thread i < H owns hidden unit i: its dh for
//      the kTile robots stays in registers, it reads r, u, c and h of its unit from the workspace, and the deltas of the tick
//      (delta_mean, delta_c, delta_ru, the dense deltas) lie in LDS for the chains, which read the transposed weights
//      coalesced along i.  Four barriers a tick, one more with two dense layers.
//   W  rg_bptt_weight_kernel: grid (row tiles of kRows input rows over all blocks, G groups of chunks); thread j owns column j
//      of the block, holds the chunk's kChunk deltas of its column in registers and kRows float64 sums; the chunk's kChunk x
//      kRows inputs are staged in LDS (the row past a block's inputs is the constant 1: the bias).  rg_bptt_grad_finish_kernel
//      adds the G float64 partials per element in index order.
// LDS (static), floats of the header limits W = RG_RNN_MAX_WIDTH, H = RG_RNN_MAX_UNITS, A = RG_RNN_MAX_ACT, tile RG_RNN_TILE:
//   F  (2 W + 3 H) * tile * 4 = 28672 bytes;  B  (2 W + 3 H + A) * tile * 4 = 28800 bytes; each with its copy of the descriptor
//      (at most 768 bytes);  W  RG_BPTT_CHUNK * RG_BPTT_ROWS * 4 = 1024 bytes;  the sums 32 bytes.
// The descriptor (layouts, the call's pointers, the workspace's regions) is written into the head of the workspace by a
// one-thread kernel first in every entry that launches; F and B copy it to LDS (as scalar registers its fields, live through
// the loop over t, do not fit beside the pointers).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rg_policy.h"
#include "../../include/rg_ppo.h"
#include "../../include/rg_rnn.h"
#include "../../include/rg_bptt.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_agent_dev.inc"
#include "rg_gru_dev.inc"
#include "rg_ppo_dev.inc"

namespace {

constexpr int kThreads = kAgentThreads;
constexpr int kChunk = RG_BPTT_CHUNK;
constexpr int kRows = RG_BPTT_ROWS;
constexpr int kMaxGroups = RG_BPTT_MAX_GROUPS;
constexpr int kMaxParts = 256;       // workgroups of the head kernel, at most
constexpr int kPart = kHeadPart;     // per workgroup of the head kernel: the loss sum, then the logstd gradient
constexpr int kBlocks = RG_RNN_MAX_DENSE + 3;

static_assert(2 * kMaxH <= kThreads && kMaxW <= kThreads, "one output neuron, one column of a block per thread");
static_assert(kTile * kMaxAct <= kThreads && kMaxAct <= kMaxW, "the mean's thread map; the head's output fits an x buffer");
static_assert(kChunk * kRows == kThreads && kRows % 4 == 0, "a thread stages one input of a chunk; rows are read as float4");
static_assert(kMaxParts <= kThreads && kMaxAct == kHeadAct, "strided sums; the head's arrays");
static_assert(RG_RNN_MAX_DENSE == 2, "the delta pass has two dense delta buffers and the transpose four blocks");

struct WBlock {                // one block of policy_params for the W phase
  const float *in0, *in1, *delta;   // the inputs [N][n0] and then [N][n1] (in1 may be null with n1 = 0), the deltas [N][out]
  int n0, n1, out, w_off, b_off, tile0;   // tile0: the first row tile of this block in the grid
};

struct BpttDev {               // in the workspace: what the kernels read of a call
  int T, B, N, obs_dim, act_dim, H, n_dense, n_x;
  int dense_in[2], dense_out[2], dense_w[2], dense_b[2];
  int w_ru, b_ru, w_c, b_c, head_w, head_b, logstd_off, count;
  int G, per, nchunks, P, nblk, pad0;
  double obs_clip, c, thr, coef;
  const float *obs, *action, *mean0, *logstd0, *adv, *h0;
  const int *mask, *reset;
  const double *norm, *scal, *penalty;
  float *a[3], *hin, *r, *u, *cc, *rh, *hn, *mean, *dmean, *dru, *dcs, *dd[2], *wt;
  double *kls, *klr, *part, *gpart;
  WBlock blk[kBlocks];
};
static_assert(sizeof(BpttDev) % sizeof(int) == 0 && sizeof(BpttDev) <= 768, "copied to LDS word by word");

__global__ void rg_bptt_describe_kernel(const BpttDev src, BpttDev *__restrict__ dst) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *dst = src;
}

// ---- F: the forward pass, every intermediate kept --------------------------------------------------------------------------

// what the update keeps of a tick: everything, in the workspace's regions at sample t0 + b0 + r, t0 = t * B
struct KeepSink {
  const BpttDev *d;
  int b0;
  size_t t0;
  __device__ __forceinline__ void dense(const int s, const int nout, const int j, const int r, const float a) const {
    if (b0 + r < d->B) d->a[s + 1][(t0 + b0 + r) * nout + j] = a;
  }
  __device__ __forceinline__ void reset_gate(const int H, const int j, const int r, const float g, const float p) const {
    if (b0 + r < d->B) { d->r[(t0 + b0 + r) * H + j] = g; d->rh[(t0 + b0 + r) * H + j] = p; }
  }
  __device__ __forceinline__ void update_gate(const int H, const int j, const int r, const float u) const {
    if (b0 + r < d->B) d->u[(t0 + b0 + r) * H + j] = u;
  }
  __device__ __forceinline__ void cell(const int H, const int j, const int r, const float c, const float hn) const {
    if (b0 + r < d->B) { d->cc[(t0 + b0 + r) * H + j] = c; d->hn[(t0 + b0 + r) * H + j] = hn; }
  }
};

__global__ void __launch_bounds__(kThreads) rg_bptt_forward_kernel(const BpttDev *__restrict__ dg, const float *__restrict__ pp) {
  __shared__ BpttDev dsh;
  __shared__ __attribute__((aligned(16))) float xs[2][kMaxW * kTile];
  __shared__ __attribute__((aligned(16))) float hs[kMaxH * kTile];
  __shared__ __attribute__((aligned(16))) float rh[kMaxH * kTile];
  __shared__ __attribute__((aligned(16))) float us[kMaxH * kTile];
  const BpttDev *d = descriptor_to_lds(dg, &dsh);
  const int tid = threadIdx.x;
  const int B = d->B, T = d->T, obs_dim = d->obs_dim, act_dim = d->act_dim, H = d->H;
  const int b0 = blockIdx.x * kTile;
  const int n_pol = d->n_dense + 3;
  const float *mean_s = xs[(d->n_dense & 1) ^ 1];
  const double *__restrict__ norm = d->norm;
  for (int idx = tid; idx < H * kTile; idx += kThreads) {
    const int r = idx / H, k = idx - r * H, b = b0 + r;
    hs[k * kTile + r] = b < B ? d->h0[(size_t)b * H + k] : 0.0f;
  }
  for (int t = 0; t < T; t++) {
    const size_t t0 = (size_t)t * B;
    const float *__restrict__ obs_t = d->obs + t0 * obs_dim;
    const int *__restrict__ reset_t = d->reset + t0;
    for (int idx = tid; idx < obs_dim * kTile; idx += kThreads) {
      const int r = idx / obs_dim, i = idx - r * obs_dim, b = b0 + r;
      float xn = 0.0f;
      if (b < B) {
        xn = normalised(obs_t, norm, i, b, B, d->obs_clip);
        d->a[0][(t0 + b) * obs_dim + i] = xn;
      }
      xs[0][i * kTile + r] = xn;
    }
    for (int idx = tid; idx < H * kTile; idx += kThreads) {   // the state this tick reads
      const int r = idx / H, k = idx - r * H, b = b0 + r;
      if (b < B) {
        if (reset_t[b] != 0) hs[k * kTile + r] = 0.0f;
        d->hin[(t0 + b) * H + k] = hs[k * kTile + r];
      }
    }
    for (int s = 0; s < n_pol; s++) {
      __syncthreads();
      gru_stage(d, pp, s, tid, xs, hs, rh, us, KeepSink{d, b0, t0});
    }
    __syncthreads();
    if (tid < kTile * act_dim) {
      const int r = tid / act_dim, a = tid % act_dim, b = b0 + r;
      if (b < B) d->mean[(t0 + b) * act_dim + a] = mean_s[a * kTile + r];
    }
    __syncthreads();   // the next tick's observation may land in the buffer the mean was read from
  }
}

// ---- H: the head, float64 --------------------------------------------------------------------------------------------------

// gaussian_head's view of sample n: the new mean from the workspace, where the forward pass left it, the delta beside it
struct StoredHead {
  const BpttDev *d;
  __device__ __forceinline__ const BpttDev &cfg() const { return *d; }
  __device__ __forceinline__ int mask(const int n) const { return d->mask[n]; }
  __device__ __forceinline__ float logstd0(const int k) const { return d->logstd0[k]; }
  __device__ __forceinline__ float mean(const int n, const int k) const { return d->mean[(size_t)n * d->act_dim + k]; }
  __device__ __forceinline__ float mean0(const int n, const int k) const { return d->mean0[(size_t)n * d->act_dim + k]; }
  __device__ __forceinline__ float action(const int n, const int k) const { return d->action[(size_t)n * d->act_dim + k]; }
  __device__ __forceinline__ float adv(const int n) const { return d->adv[n]; }
  __device__ __forceinline__ const double *scal() const { return d->scal; }
  __device__ __forceinline__ double robot_kl(const int b) const { return d->klr[b]; }
  __device__ __forceinline__ double penalty() const { return *d->penalty; }
  __device__ __forceinline__ void keep_kl(const int n, const double v) const { d->kls[n] = v; }
  __device__ __forceinline__ void keep_delta(const int n, const int k, const float v) const { d->dmean[(size_t)n * d->act_dim + k] = v; }
};

template <bool kBackward>
__device__ __forceinline__ void head_sample(const BpttDev *__restrict__ d, const float *__restrict__ P, const int n, double &loss, double (&gls)[kMaxAct]) {
  gaussian_head<kBackward>(StoredHead{d}, P, n, true, 1.0 / ((double)d->T * (double)d->B), loss, gls);
}

__global__ void __launch_bounds__(kThreads) rg_bptt_sample_kl_kernel(const BpttDev *__restrict__ d, const float *__restrict__ P) {
  const long long n = (long long)blockIdx.x * kThreads + (int)threadIdx.x;
  if (n >= d->N) return;
  double loss = 0.0, gls[kMaxAct] = {0.0, 0.0, 0.0, 0.0};
  head_sample<false>(d, P, (int)n, loss, gls);
}

// KL_b = (sum_t kls[t][b]) / T, t in order
__global__ void __launch_bounds__(kThreads) rg_bptt_robot_kl_kernel(const int T, const int B, const double *__restrict__ kls, double *__restrict__ out) {
  robot_kl_element(T, B, kls, out, blockIdx.x * kThreads + (int)threadIdx.x);
}

__global__ void __launch_bounds__(kThreads) rg_bptt_head_kernel(const BpttDev *__restrict__ d, const float *__restrict__ P) {
  __shared__ double sh[4];
  double loss = 0.0, gls[kMaxAct] = {0.0, 0.0, 0.0, 0.0};
  const long long step = (long long)d->P * kThreads;
  for (long long n = (long long)blockIdx.x * kThreads + (int)threadIdx.x; n < d->N; n += step) head_sample<true>(d, P, (int)n, loss, gls);
  double *p = d->part + (size_t)blockIdx.x * kPart;
  loss = block_sum(loss, sh);
  if (threadIdx.x == 0) p[0] = loss;
#pragma unroll
  for (int k = 0; k < kMaxAct; k++) {
    const double g = block_sum(gls[k], sh);
    if (threadIdx.x == 0) p[1 + k] = g;
  }
}

__global__ void __launch_bounds__(kThreads) rg_bptt_loss_finish_kernel(const LossCfg c, const double *__restrict__ part, const double *__restrict__ klr,
                                                                       const double *__restrict__ penalty, float *__restrict__ grad,
                                                                       double *__restrict__ loss_out, double *__restrict__ loss_out2) {
  __shared__ double sh[4];
  loss_finish(c, c.parts, true, part, klr, penalty, grad, loss_out, loss_out2, sh);
}

// ---- B: the delta pass -----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_bptt_transpose_kernel(const NetDesc nd, const int count, const float *__restrict__ P, float *__restrict__ Wt) {
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e < count) transpose_element(nd, P, Wt, e);
}

__global__ void __launch_bounds__(kThreads) rg_bptt_delta_kernel(const BpttDev *__restrict__ dg) {
  __shared__ BpttDev dsh;
  __shared__ __attribute__((aligned(16))) float dm[kMaxAct * kTile];        // delta_mean of the tick, [component * kTile + robot]
  __shared__ __attribute__((aligned(16))) float dcs[kMaxH * kTile];         // delta_c
  __shared__ __attribute__((aligned(16))) float dru[2 * kMaxH * kTile];     // delta_r, then delta_u
  __shared__ __attribute__((aligned(16))) float dbuf[2][kMaxW * kTile];     // the dense deltas, ping-pong
  const BpttDev *d = descriptor_to_lds(dg, &dsh);
  const int tid = threadIdx.x;
  const int B = d->B, act_dim = d->act_dim, H = d->H, n_dense = d->n_dense, n_x = d->n_x;
  const int b0 = blockIdx.x * kTile;
  const int bl = B - 1;                // a slot past the batch mirrors the last robot: the same loads, the same values, the same stores
  const int rows = n_x + H;            // rows of W_ru and of W_c: the stride of their transposed copies
  const float *__restrict__ Wt = d->wt;
  float dh[kTile], dhp[kTile], hin[kTile], rr[kTile], acc[kTile];
#pragma unroll
  for (int r = 0; r < kTile; r++) dh[r] = dhp[r] = hin[r] = rr[r] = 0.0f;
  for (int t = d->T - 1; t >= 0; t--) {
    const size_t t0 = (size_t)t * B;
    if (tid < act_dim * kTile) {
      const int a = tid / kTile, r = tid % kTile, b = b0 + r < bl ? b0 + r : bl;
      dm[tid] = d->dmean[(t0 + b) * act_dim + a];
    }
    __syncthreads();   // and every chain of the tick before has read dcs, dru and dbuf
    if (tid < H) {
#pragma unroll
      for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
      chain8(Wt + d->head_w + tid, H, dm, act_dim, acc);
#pragma unroll
      for (int r = 0; r < kTile; r++) {
        const int b = b0 + r < bl ? b0 + r : bl;
        const size_t o = (t0 + b) * H + tid;
        const float u = d->u[o], c = d->cc[o];
        hin[r] = d->hin[o];
        rr[r] = d->r[o];
        const float g = dh[r] + acc[r];
        const float dc = g * (1.0f - u), du = g * (hin[r] - c);
        dhp[r] = g * u;
        const float dcv = dc * (1.0f - c * c), duv = du * (u * (1.0f - u));
        dcs[tid * kTile + r] = dcv;
        dru[(H + tid) * kTile + r] = duv;
        d->dcs[o] = dcv;
        d->dru[(t0 + b) * 2 * H + H + tid] = duv;
      }
    }
    __syncthreads();
    if (tid < H) {
#pragma unroll
      for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
      chain8(Wt + d->w_c + n_x + tid, rows, dcs, H, acc);   // Wt_c[j][n_x + i]
#pragma unroll
      for (int r = 0; r < kTile; r++) {
        const int b = b0 + r < bl ? b0 + r : bl;
        const float drh = acc[r];
        const float dr = drh * hin[r];
        dhp[r] = dhp[r] + drh * rr[r];
        const float drv = dr * (rr[r] * (1.0f - rr[r]));
        dru[tid * kTile + r] = drv;
        d->dru[(t0 + b) * 2 * H + tid] = drv;
      }
    }
    __syncthreads();
    if (tid < H) {
#pragma unroll
      for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
      chain8(Wt + d->w_ru + n_x + tid, rows, dru, 2 * H, acc);   // Wt_ru[j][n_x + i]
#pragma unroll
      for (int r = 0; r < kTile; r++) {
        const int b = b0 + r < bl ? b0 + r : bl;
        const float v = dhp[r] + acc[r];
        dh[r] = d->reset[t0 + b] == 0 ? v : 0.0f;   // nothing crosses a reset
      }
    }
    if (n_dense > 0 && tid < n_x) {
#pragma unroll
      for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
      chain8(Wt + d->w_ru + tid, rows, dru, 2 * H, acc);
      chain8(Wt + d->w_c + tid, rows, dcs, H, acc);
      const float *act = d->a[n_dense];
      float *out = d->dd[n_dense - 1];
#pragma unroll
      for (int r = 0; r < kTile; r++) {
        const int b = b0 + r < bl ? b0 + r : bl;
        const float v = act[(t0 + b) * n_x + tid] > 0.0f ? acc[r] : 0.0f;
        out[(t0 + b) * n_x + tid] = v;
        dbuf[0][tid * kTile + r] = v;
      }
    }
    int cur = 0;
    for (int l = n_dense - 1; l >= 1; l--) {
      __syncthreads();
      const int nin = d->dense_in[l], nout = d->dense_out[l];
      if (tid < nin) {
#pragma unroll
        for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
        chain8(Wt + d->dense_w[l] + tid, nin, dbuf[cur], nout, acc);   // Wt_l[j][k]
        const float *act = d->a[l];
        float *out = d->dd[l - 1];
#pragma unroll
        for (int r = 0; r < kTile; r++) {
          const int b = b0 + r < bl ? b0 + r : bl;
          const float v = act[(t0 + b) * nin + tid] > 0.0f ? acc[r] : 0.0f;
          out[(t0 + b) * nin + tid] = v;
          dbuf[cur ^ 1][tid * kTile + r] = v;
        }
      }
      cur ^= 1;
    }
  }
}

// ---- W: the weight gradients -------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_bptt_weight_kernel(const BpttDev *__restrict__ d) {
  __shared__ __attribute__((aligned(16))) float xin[kChunk * kRows];   // [sample of the chunk][row of the tile]
  const int tid = threadIdx.x, g = blockIdx.y;
  int k = 0;
  for (int q = 1; q < kBlocks; q++)
    if (q < d->nblk && (int)blockIdx.x >= d->blk[q].tile0) k = q;
  const WBlock &blk = d->blk[k];
  const int n0 = blk.n0, nin = blk.n0 + blk.n1, out = blk.out, N = d->N;
  const int row0 = ((int)blockIdx.x - blk.tile0) * kRows;
  const int ss = tid / kRows, si = tid % kRows, srow = row0 + si;   // what this thread stages of a chunk
  const float *__restrict__ delta = blk.delta;
  double sum[kRows];
#pragma unroll
  for (int i = 0; i < kRows; i++) sum[i] = 0.0;
  const int first = g * d->per;
  const int last = first + d->per < d->nchunks ? first + d->per : d->nchunks;
  for (int ch = first; ch < last; ch++) {
    const long long nb = (long long)ch * kChunk;
    __syncthreads();   // the chunk before has been read
    {
      const long long n = nb + ss;
      float v = 0.0f;
      if (n < N) {
        if (srow < n0) v = blk.in0[(size_t)n * n0 + srow];
        else if (srow < nin) v = blk.in1[(size_t)n * blk.n1 + (srow - n0)];
        else if (srow == nin) v = 1.0f;
      }
      xin[ss * kRows + si] = v;
    }
    float dl[kChunk];
#pragma unroll
    for (int s = 0; s < kChunk; s++) {
      const long long n = nb + s;
      dl[s] = (tid < out && n < N) ? delta[(size_t)n * out + tid] : 0.0f;
    }
    __syncthreads();
    float v[kRows];
#pragma unroll
    for (int i = 0; i < kRows; i++) v[i] = 0.0f;
#pragma unroll
    for (int s = 0; s < kChunk; s++) {
#pragma unroll
      for (int q = 0; q < kRows / 4; q++) {
        const float4 x = *reinterpret_cast<const float4 *>(xin + s * kRows + 4 * q);
        v[4 * q] = __builtin_fmaf(x.x, dl[s], v[4 * q]);
        v[4 * q + 1] = __builtin_fmaf(x.y, dl[s], v[4 * q + 1]);
        v[4 * q + 2] = __builtin_fmaf(x.z, dl[s], v[4 * q + 2]);
        v[4 * q + 3] = __builtin_fmaf(x.w, dl[s], v[4 * q + 3]);
      }
    }
#pragma unroll
    for (int i = 0; i < kRows; i++) sum[i] = sum[i] + (double)v[i];
  }
  if (tid < out) {
    double *__restrict__ part = d->gpart + (size_t)g * d->count;
#pragma unroll
    for (int i = 0; i < kRows; i++) {
      const int row = row0 + i;
      if (row < nin) part[blk.w_off + (size_t)row * out + tid] = sum[i];
      else if (row == nin) part[blk.b_off + tid] = sum[i];
    }
  }
}

// grad[e] = (float) sum_g gpart[g][e], g in order, for the first n elements (the networks; logstd is the loss kernel's)
__global__ void __launch_bounds__(kThreads) rg_bptt_grad_finish_kernel(const int n, const int count, const int G, const double *__restrict__ gpart,
                                                                       float *__restrict__ grad) {
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int g = 0; g < G; g++) s = s + gpart[(size_t)g * count + e];
  grad[e] = (float)s;
}

// ---- Adam and the penalty ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_bptt_adam_kernel(const AdamCfg c, float *__restrict__ p, const float *__restrict__ grad,
                                                                float *__restrict__ m, float *__restrict__ v, const long long *__restrict__ step) {
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= c.count) return;
  const AdamBias bias = adam_bias(c, *step);
  adam_element(c, bias, grad[e], p, m, v, e);
}

__global__ void rg_bptt_adam_count_kernel(long long *__restrict__ step) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *step = *step + 1;
}

// stats: kl_change, penalty; nan_out (or null): two losses that no epoch wrote
__global__ void __launch_bounds__(kThreads) rg_bptt_penalty_kernel(const int B, const double target, const double *__restrict__ klr,
                                                                   double *__restrict__ penalty, double *__restrict__ stats, double *__restrict__ nan_out) {
  __shared__ double sh[4];
  const double s = strided_sum(klr, B, 1, sh);
  if (threadIdx.x == 0) {
    const PenaltyMove mv = move_penalty(s, B, target, penalty);
    *penalty = mv.penalty;
    stats[0] = mv.change;
    stats[1] = mv.penalty;
    if (nan_out) nan_out[0] = nan_out[1] = nan("");
  }
}

thread_local std::string g_create_err;

}  // namespace

struct rg_bptt_handle {
  rg_rnn_config rcfg{};
  rg_ppo_config cfg{};
  BpttDev dv{};                // everything but the call's pointers and the workspace's regions
  NetDesc tr{};                // the blocks whose transposed copy the delta pass reads
  int T = 0, B = 0, N = 0, device = 0, tiles = 0;
  // byte offsets into the workspace
  size_t o_desc = 0, o_part = 0, o_klr = 0, o_kls = 0, o_grad = 0, o_wt = 0, o_gpart = 0, o_a[3] = {0, 0, 0}, o_hin = 0, o_r = 0, o_u = 0, o_c = 0, o_rh = 0,
         o_hn = 0, o_mean = 0, o_dmean = 0, o_dru = 0, o_dcs = 0, o_dd[2] = {0, 0}, ws_bytes = 0, opt_bytes = 0;
  std::string err;
};

namespace {

int hip_fail(rg_bptt_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_BPTT_ERR_HIP, what, e); }
int no_device(rg_bptt_handle *h) { return no_device(h, RG_BPTT_ERR_NO_DEVICE, "RG_BPTT"); }
int launch_status(rg_bptt_handle *h, const char *what) { return launch_status(h, RG_BPTT_ERR_HIP, what); }
int null_arg(rg_bptt_handle *h, const char *call, const char *name) { return null_arg(h, RG_BPTT_ERR_INVALID, call, name); }

unsigned blocks_of(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

long long *step_of(void *opt) { return reinterpret_cast<long long *>(opt); }
double *penalty_of(void *opt) { return reinterpret_cast<double *>(static_cast<char *>(opt) + 8); }
const double *penalty_of(const void *opt) { return reinterpret_cast<const double *>(static_cast<const char *>(opt) + 8); }

// what the kernels of a call read: the handle's part, the call's pointers, the workspace's regions
struct Call {
  const rg_ppo_rollout *ro;
  const int32_t *reset;
  const float *h0;
  const double *adv_stats, *norm, *penalty;
};

int run_describe(rg_bptt_handle *h, const Call &c, void *ws, hipStream_t s) {
  BpttDev d = h->dv;
  d.obs = c.ro->obs; d.action = c.ro->action; d.mean0 = c.ro->mean; d.logstd0 = c.ro->logstd; d.adv = c.ro->adv; d.mask = (const int *)c.ro->mask;
  d.reset = (const int *)c.reset; d.h0 = c.h0; d.norm = c.norm; d.scal = c.adv_stats; d.penalty = c.penalty;
  for (int l = 0; l < 3; l++) d.a[l] = ws_at<float>(ws, h->o_a[l]);
  d.hin = ws_at<float>(ws, h->o_hin); d.r = ws_at<float>(ws, h->o_r); d.u = ws_at<float>(ws, h->o_u); d.cc = ws_at<float>(ws, h->o_c);
  d.rh = ws_at<float>(ws, h->o_rh); d.hn = ws_at<float>(ws, h->o_hn); d.mean = ws_at<float>(ws, h->o_mean); d.dmean = ws_at<float>(ws, h->o_dmean);
  d.dru = ws_at<float>(ws, h->o_dru); d.dcs = ws_at<float>(ws, h->o_dcs);
  for (int l = 0; l < 2; l++) d.dd[l] = ws_at<float>(ws, h->o_dd[l]);
  d.wt = ws_at<float>(ws, h->o_wt);
  d.kls = ws_at<double>(ws, h->o_kls); d.klr = ws_at<double>(ws, h->o_klr); d.part = ws_at<double>(ws, h->o_part); d.gpart = ws_at<double>(ws, h->o_gpart);
  // the blocks of the W phase, in the buffer's order
  const int nd = d.n_dense;
  int k = 0, tile = 0;
  auto add = [&](const float *in0, int n0, const float *in1, int n1, const float *delta, int out, int w_off, int b_off) {
    d.blk[k] = WBlock{in0, in1, delta, n0, n1, out, w_off, b_off, tile};
    tile += (n0 + n1 + 1 + kRows - 1) / kRows;
    k++;
  };
  for (int l = 0; l < nd; l++) add(d.a[l], d.dense_in[l], nullptr, 0, d.dd[l], d.dense_out[l], d.dense_w[l], d.dense_b[l]);
  add(d.a[nd], d.n_x, d.hin, d.H, d.dru, 2 * d.H, d.w_ru, d.b_ru);
  add(d.a[nd], d.n_x, d.rh, d.H, d.dcs, d.H, d.w_c, d.b_c);
  add(d.hn, d.H, nullptr, 0, d.dmean, d.act_dim, d.head_w, d.head_b);
  d.nblk = k;
  h->tiles = tile;
  hipLaunchKernelGGL(rg_bptt_describe_kernel, dim3(1), dim3(64), 0, s, d, ws_at<BpttDev>(ws, h->o_desc));
  return launch_status(h, "rg_bptt_describe_kernel launch");
}

int run_forward(rg_bptt_handle *h, const float *pp, void *ws, hipStream_t s) {
  hipLaunchKernelGGL(rg_bptt_forward_kernel, dim3(((unsigned)h->B + kTile - 1) / kTile), dim3(kThreads), 0, s, ws_at<const BpttDev>(ws, h->o_desc), pp);
  return launch_status(h, "rg_bptt_forward_kernel launch");
}

// F, then KL_b per robot into kl_out
int run_robot_kl(rg_bptt_handle *h, const float *pp, void *ws, double *kl_out, hipStream_t s) {
  int rc = run_forward(h, pp, ws, s);
  if (rc) return rc;
  hipLaunchKernelGGL(rg_bptt_sample_kl_kernel, dim3(blocks_of(h->N)), dim3(kThreads), 0, s, ws_at<const BpttDev>(ws, h->o_desc), pp);
  rc = launch_status(h, "rg_bptt_sample_kl_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_bptt_robot_kl_kernel, dim3(blocks_of(h->B)), dim3(kThreads), 0, s, h->T, h->B, ws_at<const double>(ws, h->o_kls), kl_out);
  return launch_status(h, "rg_bptt_robot_kl_kernel launch");
}

int run_policy_grad(rg_bptt_handle *h, const float *pp, const void *opt, void *ws, float *grad, double *loss_out, double *loss_out2, hipStream_t s) {
  const BpttDev &d = h->dv;
  const BpttDev *desc = ws_at<const BpttDev>(ws, h->o_desc);
  hipLaunchKernelGGL(rg_bptt_transpose_kernel, dim3(blocks_of(d.count)), dim3(kThreads), 0, s, h->tr, d.count, pp, ws_at<float>(ws, h->o_wt));
  int rc = launch_status(h, "rg_bptt_transpose_kernel launch");
  if (rc) return rc;
  rc = run_robot_kl(h, pp, ws, ws_at<double>(ws, h->o_klr), s);
  if (rc) return rc;
  hipLaunchKernelGGL(rg_bptt_head_kernel, dim3((unsigned)d.P), dim3(kThreads), 0, s, desc, pp);
  rc = launch_status(h, "rg_bptt_head_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_bptt_delta_kernel, dim3(((unsigned)h->B + kTile - 1) / kTile), dim3(kThreads), 0, s, desc);
  rc = launch_status(h, "rg_bptt_delta_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_bptt_weight_kernel, dim3((unsigned)h->tiles, (unsigned)d.G), dim3(kThreads), 0, s, desc);
  rc = launch_status(h, "rg_bptt_weight_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_bptt_grad_finish_kernel, dim3(blocks_of(d.logstd_off)), dim3(kThreads), 0, s, d.logstd_off, d.count, d.G,
                     ws_at<const double>(ws, h->o_gpart), grad);
  rc = launch_status(h, "rg_bptt_grad_finish_kernel launch");
  if (rc) return rc;
  const LossCfg lc{h->T, h->B, d.P, d.act_dim, d.logstd_off, 1, d.thr, d.coef};
  hipLaunchKernelGGL(rg_bptt_loss_finish_kernel, dim3(1), dim3(kThreads), 0, s, lc, ws_at<const double>(ws, h->o_part), ws_at<const double>(ws, h->o_klr),
                     penalty_of(opt), grad, loss_out, loss_out2);
  return launch_status(h, "rg_bptt_loss_finish_kernel launch");
}

int run_adam(rg_bptt_handle *h, float *params, const float *grad, void *opt, hipStream_t s) {
  const int count = h->dv.count;
  float *m = reinterpret_cast<float *>(static_cast<char *>(opt) + RG_BPTT_OPT_HEADER_BYTES);
  const AdamCfg c{count, 0, h->cfg.policy_lr, h->cfg.beta1, h->cfg.beta2, h->cfg.adam_eps};
  hipLaunchKernelGGL(rg_bptt_adam_kernel, dim3(blocks_of(count)), dim3(kThreads), 0, s, c, params, grad, m, m + count, (const long long *)step_of(opt));
  int rc = launch_status(h, "rg_bptt_adam_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_bptt_adam_count_kernel, dim3(1), dim3(64), 0, s, step_of(opt));
  return launch_status(h, "rg_bptt_adam_count_kernel launch");
}

int run_penalty(rg_bptt_handle *h, const double *kl, void *opt, double *stats, double *nan_out, hipStream_t s) {
  hipLaunchKernelGGL(rg_bptt_penalty_kernel, dim3(1), dim3(kThreads), 0, s, h->B, h->cfg.kl_target, kl, penalty_of(opt), stats, nan_out);
  return launch_status(h, "rg_bptt_penalty_kernel launch");
}

int check_rollout(rg_bptt_handle *h, const char *call, const rg_ppo_rollout *ro, bool grad) {
  RG_NEED(call, ro, "rollout");
  RG_NEED(call, ro->obs, "rollout.obs");
  if (grad) RG_NEED(call, ro->action, "rollout.action");
  RG_NEED(call, ro->mean, "rollout.mean");
  RG_NEED(call, ro->logstd, "rollout.logstd");
  if (grad) RG_NEED(call, ro->adv, "rollout.adv");
  RG_NEED(call, ro->mask, "rollout.mask");
  return RG_BPTT_OK;
}

}  // namespace

extern "C" {

int32_t rg_bptt_abi_version(void) { return RG_BPTT_ABI_VERSION; }
int32_t rg_bptt_tile(void) { return RG_RNN_TILE; }
const char *rg_bptt_last_error(const rg_bptt_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }
int64_t rg_bptt_workspace_bytes(const rg_bptt_handle *h) { return h ? (int64_t)h->ws_bytes : -1; }
int64_t rg_bptt_opt_state_bytes(const rg_bptt_handle *h) { return h ? (int64_t)h->opt_bytes : -1; }
int32_t rg_bptt_groups(const rg_bptt_handle *h) { return h ? h->dv.G : -1; }

int rg_bptt_create(const rg_rnn_config *rnn_cfg, const rg_ppo_config *ppo_cfg, int32_t T, int32_t B, int32_t device, rg_bptt_handle **out) {
  if (!rnn_cfg || !ppo_cfg || !out) { g_create_err = "create: null rnn_cfg, ppo_cfg or out"; return RG_BPTT_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  const IntField sizes[] = {{"T", T, 1, RG_RNN_MAX_T}, {"B", B, 1, RG_RNN_MAX_BATCH}};
  if (!check_rnn_config("rnn_cfg.", rnn_cfg, err) || !check_ppo_config(ppo_cfg, err) || !check_ints("", sizes, err) || !check_samples(T, B, err)) {
    g_create_err = err;
    return RG_BPTT_ERR_INVALID;
  }
  rg_bptt_handle *h = new rg_bptt_handle();
  h->rcfg = *rnn_cfg;
  h->cfg = *ppo_cfg;
  h->T = T; h->B = B; h->N = T * B; h->device = device;
  BpttDev &d = h->dv;
  rg_rnn_layout L;
  fill_layout(rnn_cfg, L);
  const int H = L.gru_units, nd = L.n_dense, n_x = L.n_x, A = rnn_cfg->act_dim;
  d.T = T; d.B = B; d.N = h->N; d.obs_dim = rnn_cfg->obs_dim; d.act_dim = A;
  layout_to_dev(L, d);
  d.count = L.policy_count;
  d.nchunks = (h->N + kChunk - 1) / kChunk;
  const int gmax = d.nchunks < kMaxGroups ? d.nchunks : kMaxGroups;
  d.per = (d.nchunks + gmax - 1) / gmax;
  d.G = (d.nchunks + d.per - 1) / d.per;
  d.P = (int)((h->N + kThreads - 1) / kThreads);
  if (d.P > kMaxParts) d.P = kMaxParts;
  d.obs_clip = rnn_cfg->obs_clip;
  d.c = ppo_cfg->conv_logpdf == RG_PPO_LOGPDF_EXACT ? 1.0 : 0.5;
  d.thr = ppo_cfg->kl_target * ppo_cfg->kl_cutoff_factor;
  d.coef = ppo_cfg->kl_cutoff_coef;
  // the transposed copies: the second dense layer, W_ru, W_c, the head
  NetDesc &tr = h->tr;
  int k = 0;
  auto add = [&](int in, int out_, int w) { tr.in[k] = in; tr.out[k] = out_; tr.w[k] = w; tr.b[k] = 0; k++; };
  if (nd == 2) add(d.dense_in[1], d.dense_out[1], d.dense_w[1]);
  add(n_x + H, 2 * H, d.w_ru);
  add(n_x + H, H, d.w_c);
  add(H, A, d.head_w);
  tr.n = k;
  const size_t N = (size_t)h->N, f = sizeof(float);
  size_t o = 0;
  h->o_desc = o; o += round8(sizeof(BpttDev));
  h->o_part = o; o += sizeof(double) * (size_t)d.P * kPart;
  h->o_klr = o; o += sizeof(double) * (size_t)B;
  h->o_kls = o; o += sizeof(double) * N;
  h->o_grad = o; o += round8(f * (size_t)d.count);
  h->o_wt = o; o += round8(f * (size_t)d.count);
  h->o_gpart = o; o += sizeof(double) * (size_t)d.G * (size_t)d.count;
  h->o_a[0] = o; o += round8(f * N * (size_t)d.obs_dim);
  for (int l = 0; l < 2; l++) { h->o_a[l + 1] = o; if (l < nd) o += round8(f * N * (size_t)d.dense_out[l]); }
  size_t *cell[] = {&h->o_hin, &h->o_r, &h->o_u, &h->o_c, &h->o_rh, &h->o_hn, &h->o_dcs};
  for (size_t *p : cell) { *p = o; o += round8(f * N * (size_t)H); }
  h->o_dru = o; o += round8(f * N * 2 * (size_t)H);
  h->o_mean = o; o += round8(f * N * (size_t)A);
  h->o_dmean = o; o += round8(f * N * (size_t)A);
  for (int l = 0; l < 2; l++) { h->o_dd[l] = o; if (l < nd) o += round8(f * N * (size_t)d.dense_out[l]); }
  h->ws_bytes = o;
  h->opt_bytes = RG_BPTT_OPT_HEADER_BYTES + f * 2 * (size_t)d.count;
  if (device == RG_BPTT_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_BPTT_OK;
  }
  if (const int rc = enter_device(device, nullptr, RG_BPTT_ERR_NO_DEVICE, RG_BPTT_ERR_INVALID, RG_BPTT_ERR_HIP, g_create_err)) { delete h; return rc; }
  *out = h;
  return RG_BPTT_OK;
}

void rg_bptt_destroy(rg_bptt_handle *h) { delete h; }

int rg_bptt_policy_grad(rg_bptt_handle *h, const rg_ppo_rollout *ro, const int32_t *reset, const float *h0, const double *adv_stats,
                        const double *norm_state, const float *policy_params, const void *opt_state, void *workspace, float *grad_out,
                        double *loss_out, void *stream) {
  if (!h) { g_create_err = "policy_grad: null handle"; return RG_BPTT_ERR_INVALID; }
  int rc = check_rollout(h, "policy_grad", ro, true);
  if (rc) return rc;
  RG_NEED("policy_grad", reset, "reset");
  RG_NEED("policy_grad", h0, "h0");
  RG_NEED("policy_grad", adv_stats, "adv_stats");
  RG_NEED("policy_grad", norm_state, "norm_state");
  RG_NEED("policy_grad", policy_params, "policy_params");
  RG_NEED("policy_grad", opt_state, "opt_state");
  RG_NEED("policy_grad", workspace, "workspace");
  RG_NEED("policy_grad", grad_out, "grad_out");
  RG_NEED("policy_grad", loss_out, "loss_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  rc = run_describe(h, Call{ro, reset, h0, adv_stats, norm_state, penalty_of(opt_state)}, workspace, s);
  if (rc) return rc;
  return run_policy_grad(h, policy_params, opt_state, workspace, grad_out, loss_out, nullptr, s);
}

int rg_bptt_kl(rg_bptt_handle *h, const rg_ppo_rollout *ro, const int32_t *reset, const float *h0, const double *norm_state,
               const float *policy_params, void *workspace, double *kl_out, void *stream) {
  if (!h) { g_create_err = "kl: null handle"; return RG_BPTT_ERR_INVALID; }
  int rc = check_rollout(h, "kl", ro, false);
  if (rc) return rc;
  RG_NEED("kl", reset, "reset");
  RG_NEED("kl", h0, "h0");
  RG_NEED("kl", norm_state, "norm_state");
  RG_NEED("kl", policy_params, "policy_params");
  RG_NEED("kl", workspace, "workspace");
  RG_NEED("kl", kl_out, "kl_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  rc = run_describe(h, Call{ro, reset, h0, nullptr, norm_state, nullptr}, workspace, s);
  if (rc) return rc;
  return run_robot_kl(h, policy_params, workspace, kl_out, s);
}

int rg_bptt_adam(rg_bptt_handle *h, float *params, const float *grad, void *opt_state, void *stream) {
  if (!h) { g_create_err = "adam: null handle"; return RG_BPTT_ERR_INVALID; }
  RG_NEED("adam", params, "params");
  RG_NEED("adam", grad, "grad");
  RG_NEED("adam", opt_state, "opt_state");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_adam(h, params, grad, opt_state, (hipStream_t)stream);
}

int rg_bptt_penalty(rg_bptt_handle *h, const double *kl, void *opt_state, double *stats, void *stream) {
  if (!h) { g_create_err = "penalty: null handle"; return RG_BPTT_ERR_INVALID; }
  RG_NEED("penalty", kl, "kl");
  RG_NEED("penalty", opt_state, "opt_state");
  RG_NEED("penalty", stats, "stats");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_penalty(h, kl, opt_state, stats, nullptr, (hipStream_t)stream);
}

int rg_bptt_update_policy(rg_bptt_handle *h, const rg_ppo_rollout *ro, const int32_t *reset, const float *h0, const double *adv_stats,
                          const double *norm_state, float *policy_params, void *opt_state, void *workspace, double *stats, void *stream) {
  if (!h) { g_create_err = "update_policy: null handle"; return RG_BPTT_ERR_INVALID; }
  int rc = check_rollout(h, "update_policy", ro, true);
  if (rc) return rc;
  RG_NEED("update_policy", reset, "reset");
  RG_NEED("update_policy", h0, "h0");
  RG_NEED("update_policy", adv_stats, "adv_stats");
  RG_NEED("update_policy", norm_state, "norm_state");
  RG_NEED("update_policy", policy_params, "policy_params");
  RG_NEED("update_policy", opt_state, "opt_state");
  RG_NEED("update_policy", workspace, "workspace");
  RG_NEED("update_policy", stats, "stats");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  float *grad = ws_at<float>(workspace, h->o_grad);
  rc = run_describe(h, Call{ro, reset, h0, adv_stats, norm_state, penalty_of(opt_state)}, workspace, s);
  for (int e = 0; e < h->cfg.epochs_policy && !rc; e++) {
    rc = run_policy_grad(h, policy_params, opt_state, workspace, grad, e == 0 ? stats + 0 : stats + 1, e == 0 ? stats + 1 : nullptr, s);
    if (!rc) rc = run_adam(h, policy_params, grad, opt_state, s);
  }
  if (rc) return rc;
  double *klr = ws_at<double>(workspace, h->o_klr);
  rc = run_robot_kl(h, policy_params, workspace, klr, s);
  if (rc) return rc;
  return run_penalty(h, klr, opt_state, stats + 2, h->cfg.epochs_policy == 0 ? stats : nullptr, s);
}

}  // extern "C"
