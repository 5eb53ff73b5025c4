// rg_ddpg.hip -- the DDPG agent of include/rg_ddpg.h.  Its own translation unit of librg_mpc.so.  The noise stream, a layer's
// forward and backward pass over a tile, the workgroup sums, the bodies of the transpose and slab-finish kernels and Adam's
// arithmetic behind the clip are those of rg_agent_dev.inc, which the PPO agent's files include too, and the host helpers those of rg_host.h;
// rg_mpc.hip includes neither, so the source hash behind profiles/ is unaffected.
//
// Sweeps (rg_ddpg_critic_sweep_kernel, rg_ddpg_actor_sweep_kernel): G workgroups of 256 threads, workgroup g walks the tiles
// g, g + G, ... of kTile samples.  LDS (dynamic): the tile's activations of every layer of the critic, then of the actor, as
// a[layer][neuron * kTile + sample] (the input first), then two delta buffers of the widest layer.  A tile's samples are
// gathered from the replay ring by the window rule of rg_ddpg.h: thread s < kTile finds how many of sample s's window are kept,
// then every thread fills its share of the input.
//   critic sweep  s1 -> target actor -> [a', s1] -> target critic -> y; [a, s0] -> critic -> delta -> backward with weights.
//   actor sweep   s0 -> actor -> [mu, s0] -> critic -> delta_Q -> backward through the critic's inputs -> the action's
//                 components times (1 - mu^2) -> backward through the actor with weights.
// The layer descriptors are kernel arguments, copied into LDS by thread 0 and indexed there (dynamic indexing of a by-value
// kernel argument would end on the stack).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rg_ddpg.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_agent_dev.inc"

namespace {

constexpr int kTile = RG_DDPG_TILE;
constexpr int kThreads = kAgentThreads;
constexpr int kMaxGroups = RG_DDPG_MAX_GROUPS;
constexpr int kMaxAct = RG_DDPG_MAX_ACT;
constexpr int kMaxIn = RG_DDPG_MAX_INPUT;
constexpr int kMaxHidden = RG_DDPG_MAX_LAYERS * RG_DDPG_MAX_WIDTH;
// dynamic LDS of a sweep at the widest configuration: the critic's activations (input, three hidden layers, head), the actor's, two delta buffers
constexpr int kMaxLds = ((kMaxAct + kMaxIn) + kMaxHidden + 1 + kMaxIn + kMaxHidden + kMaxAct + 2 * RG_DDPG_MAX_WIDTH) * kTile * 4;
static_assert(kMaxLds == 148032 && kMaxLds <= 160 * 1024, "a sweep's tile fits a compute unit's LDS at every configuration");
// static LDS of the act kernel: the actor's activations of every layer
constexpr int kActFloats = (kMaxIn + kMaxHidden + kMaxAct) * kTile;
static_assert(kActFloats * 4 <= 60 * 1024, "the act kernel's activations fit the static LDS of a workgroup");

static_assert(kTile == kAgentTile, "the sweeps run the shared layers, whose tile is four float4");
static_assert(RG_DDPG_MAX_WIDTH <= kThreads && kMaxAct + kMaxIn <= kThreads, "one neuron per thread");
static_assert(kMaxGroups <= kThreads && kTile * kMaxAct <= 64, "thread maps");
static_assert(RG_DDPG_MAX_OBS * RG_DDPG_MAX_WINDOW >= kMaxIn, "the input limit is the tighter one");

struct Net : NetDesc {
  int count, asum;             // floats in the buffer; floats per sample of the activations, the input included
};

struct RingDev {
  float *obs, *action, *reward;
  int *done;
  long long *state;
};

struct Geo {
  int B, C, obs_dim, act_dim, window, in_s, M, G, ntiles, dmax;
  double gamma;
};

// the sample stream: rg_ddpg.h, rg_ddpg_sample (the chain of rg_stream_dev.inc, which rg_agent_dev.inc includes)
__device__ __forceinline__ unsigned long long sample_hash(unsigned long long seed, unsigned long long updates, unsigned long long m,
                                                          unsigned long long draw) {
  return mix_word(mix_word(mix_word(seed, updates), m), draw);
}

__device__ __forceinline__ bool short_ring(const long long *__restrict__ state) { return state[1] < 2; }

// ---- the window rule --------------------------------------------------------------------------------------------------

__device__ __forceinline__ long long slot_of(long long head, long long age, int C) {
  long long s = (head - 1 - age) % (long long)C;
  return s < 0 ? s + C : s;
}

// how many elements (newest first) of the state of robot b ending at age a are kept; a = -1 is the acting state, whose element 0
// is the current observation
__device__ __forceinline__ int window_kept(const int *__restrict__ done, long long head, long long count, const Geo &g, long long a, int b) {
  int k = 0;
  for (; k < g.window; k++) {
    const long long age = a + k;
    if (age >= count) break;
    if (k > 0 && done[(size_t)slot_of(head, age, g.C) * g.B + b] != 0) break;
  }
  return k;
}

// x[f * kTile + s] for f = (window - 1 - k) * obs_dim + i: oldest first.  cur: the current observation [obs_dim][B] of an acting state (age -1);
// the sweeps, whose ages are never negative, pass the ring itself
__device__ __forceinline__ void fill_state(const Geo &g, const float *__restrict__ ring_obs, const float *__restrict__ cur, long long head,
                                           const int *s_age, const int *s_rob, const int *s_kept, float *x) {
  for (int idx = threadIdx.x; idx < g.in_s * kTile; idx += kThreads) {
    const int f = idx / kTile, s = idx % kTile;
    const int k = g.window - 1 - f / g.obs_dim, i = f % g.obs_dim;
    float v = 0.0f;
    if (k < s_kept[s]) {
      const long long age = (long long)s_age[s] + k;
      const int b = s_rob[s];
      v = age < 0 ? cur[(size_t)i * g.B + b] : ring_obs[((size_t)slot_of(head, age, g.C) * g.obs_dim + i) * g.B + b];
    }
    x[idx] = v;
  }
}

// ---- the layers (rg_agent_dev.inc's) and what only this agent needs of them -------------------------------------------------

// the critic's input layer toward the action: dn[k][s] = (float)((double)(sum_j Wt[j][k] dl[j][s]) * (1 - mu[k][s]^2)) for k < act_dim; no gate
__device__ __forceinline__ void backward_action(const float *__restrict__ Wt, const int nin, const int nout, const int woff, const int act_dim,
                                                const float *mu, const float *dl, float *dn) {
  const int i = threadIdx.x;
  if (i < act_dim) {
    float acc[kTile];
    input_chain(Wt, nin, nout, woff, dl, acc);
    const float *mi = mu + i * kTile;
    float *di = dn + i * kTile;
#pragma unroll
    for (int r = 0; r < kTile; r++) {
      const double m = (double)mi[r];
      di[r] = (float)((double)acc[r] * (1.0 - m * m));
    }
  }
}

// a value every lane holds alike, as a scalar: the layer descriptors are read from LDS
__device__ __forceinline__ int uni(const int v) { return __builtin_amdgcn_readfirstlane(v); }

// every layer of a network over the tile in acts (the input first); head 1 tanhf, 2 linear.  Ends behind a barrier.
__device__ __forceinline__ void forward_net(const Net &nd, const float *__restrict__ P, float *acts, const int head) {
  const int n = uni(nd.n);
  int ao = 0;
  for (int l = 0; l < n; l++) {
    __syncthreads();
    const int nin = uni(nd.in[l]);
    const int an = ao + nin * kTile;
    forward_layer(P, nin, uni(nd.out[l]), uni(nd.w[l]), uni(nd.b[l]), acts + ao, acts + an, l < n - 1 ? 0 : head);
    ao = an;
  }
  __syncthreads();
}

// where the input of layer l lies in a network's activations
__device__ __forceinline__ int input_offset(const Net &nd, const int l) {
  int ao = 0;
  for (int m = 0; m < l; m++) ao += uni(nd.in[m]) * kTile;
  return ao;
}

// the backward pass with weight gradients, the head's delta in dl.  Starts with a barrier.
__device__ __forceinline__ void backward_net(const Net &nd, const float *__restrict__ Wt, float *__restrict__ slab, const float *acts, float *dl,
                                             float *dn) {
  for (int l = uni(nd.n) - 1; l >= 0; l--) {
    __syncthreads();
    const float *x = acts + input_offset(nd, l);
    const int nin = uni(nd.in[l]), nout = uni(nd.out[l]), woff = uni(nd.w[l]);
    backward_weights(slab, nin, nout, woff, uni(nd.b[l]), x, dl);
    if (l > 0) backward_inputs(Wt, nin, nout, woff, x, dl, dn);
    float *t = dl; dl = dn; dn = t;
  }
}

// every element of the slab belongs to the thread that accumulates it: that thread clears it
__device__ __forceinline__ void clear_slab(const Net &nd, float *__restrict__ slab) {
  const int tid = threadIdx.x;
  for (int l = 0; l < uni(nd.n); l++) {
    const int nin = uni(nd.in[l]), nout = uni(nd.out[l]), woff = uni(nd.w[l]), boff = uni(nd.b[l]);
    if (tid < nout) {
      slab[boff + tid] = 0.0f;
      for (int i = 0; i < nin; i++) slab[woff + (size_t)i * nout + tid] = 0.0f;
    }
  }
}

// the layer descriptors from the kernel's arguments into LDS, where the loops over layers index them (dynamic indexing of a
// by-value kernel argument ends on the stack).  Ends behind a barrier.
__device__ __forceinline__ void stage_nets(const Net &actor, const Net &critic, Net *s_net) {
  if (threadIdx.x == 0) { s_net[0] = actor; s_net[1] = critic; }
  __syncthreads();
}

// ---- the transposed copy of the weights -------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_ddpg_transpose_kernel(const Net nd, const float *__restrict__ P, float *__restrict__ Wt,
                                                                     const long long *__restrict__ gate) {
  if (short_ring(gate)) return;
  transpose_element(nd, P, Wt, blockIdx.x * kThreads + (int)threadIdx.x);
}

// ---- act, store, sample -----------------------------------------------------------------------------------------------

struct OuCfg {
  double theta, mu, sigma, dt;
  unsigned long long seed;
};

__global__ void __launch_bounds__(kThreads) rg_ddpg_act_kernel(const Geo g, const Net actor_arg, const OuCfg ou, const RingDev ring, const float *__restrict__ obs,
                                                               const float *__restrict__ P, float *__restrict__ ou_state, long long *__restrict__ act_state,
                                                               const int mode, float *__restrict__ action, float *__restrict__ mean) {
  __shared__ __attribute__((aligned(16))) float acts[kActFloats];
  __shared__ int s_age[kTile], s_rob[kTile], s_kept[kTile];
  __shared__ Net s_net[2];
  stage_nets(actor_arg, actor_arg, s_net);
  const Net &actor = s_net[0];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * kTile;
  const long long head = ring.state[0], count = ring.state[1];
  if (tid < kTile) {
    const int b = b0 + tid;
    s_age[tid] = -1;
    s_rob[tid] = b < g.B ? b : 0;
    s_kept[tid] = b < g.B ? window_kept(ring.done, head, count, g, -1, b) : 0;
  }
  __syncthreads();
  fill_state(g, ring.obs, obs, head, s_age, s_rob, s_kept, acts);
  forward_net(actor, P, acts, 1);
  const float *mean_s = acts + (uni(actor.asum) - g.act_dim) * kTile;   // [component * kTile + robot]
  // thread r * act_dim + a, so that a tile's actions are one contiguous store
  if (tid < kTile * g.act_dim) {
    const int r = tid / g.act_dim, a = tid % g.act_dim, b = b0 + r;
    if (b < g.B) {
      const float m = mean_s[a * kTile + r];
      float act = m;
      if (mode == RG_DDPG_MODE_SAMPLE) {
        const size_t o = (size_t)b * g.act_dim + a;
        const double e = (double)noise_eps(ou.seed, (unsigned long long)act_state[b], (unsigned long long)act_state[(size_t)g.B + b], (unsigned long long)a);
        const double x = (double)ou_state[o];
        const float xn = (float)((x + (ou.theta * (ou.mu - x)) * ou.dt) + (ou.sigma * sqrt(ou.dt)) * e);
        ou_state[o] = xn;
        act = m + xn;
      }
      action[(size_t)b * g.act_dim + a] = act;
      if (mean) mean[(size_t)b * g.act_dim + a] = m;
    }
  }
  __syncthreads();   // every counter has been read
  if (mode == RG_DDPG_MODE_SAMPLE && tid < kTile && b0 + tid < g.B) act_state[(size_t)g.B + b0 + tid] = act_state[(size_t)g.B + b0 + tid] + 1;
}

__global__ void __launch_bounds__(kThreads) rg_ddpg_store_kernel(const Geo g, const RingDev ring, const float *__restrict__ obs, const float *__restrict__ action,
                                                                 const float *__restrict__ reward, const int *__restrict__ done, float *__restrict__ ou_state) {
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t B = (size_t)g.B, no = (size_t)g.obs_dim * B, na = (size_t)g.act_dim * B;
  const long long raw = ring.state[0];
  const size_t head = (size_t)(raw < 0 ? 0 : (raw >= g.C ? g.C - 1 : raw));   // a state the caller spoilt cannot send a write outside the ring
  if (e < no) {
    ring.obs[head * no + e] = obs[e];
  } else if (e < no + na) {
    const size_t k = e - no;
    ring.action[head * na + k] = action[k];
    if (ou_state && done[k / g.act_dim] != 0) ou_state[k] = 0.0f;
  } else if (e < no + na + B) {
    const size_t k = e - no - na;
    ring.reward[head * B + k] = reward[k];
  } else if (e < no + na + 2 * B) {
    const size_t k = e - no - na - B;
    ring.done[head * B + k] = done[k];
  }
}

__global__ void rg_ddpg_store_advance_kernel(const int C, long long *__restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long raw = state[0];
    const long long head = raw < 0 ? 0 : (raw >= C ? C - 1 : raw);
    state[0] = (head + 1) % C;
    state[1] = state[1] + 1 < C ? state[1] + 1 : C;
  }
}

__global__ void __launch_bounds__(kThreads) rg_ddpg_sample_kernel(const int M, const int B, const unsigned long long seed, const long long *__restrict__ state,
                                                                  int *__restrict__ idx) {
  if (short_ring(state)) return;
  const int m = blockIdx.x * kThreads + (int)threadIdx.x;
  if (m >= M) return;
  const unsigned long long count = (unsigned long long)state[1], updates = (unsigned long long)state[2];
  idx[2 * m] = 1 + (int)(sample_hash(seed, updates, (unsigned long long)m, 0) % (count - 1ull));
  idx[2 * m + 1] = (int)(sample_hash(seed, updates, (unsigned long long)m, 1) % (unsigned long long)B);
}

__global__ void rg_ddpg_advance_kernel(long long *__restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && !short_ring(state)) state[2] = state[2] + 1;
}

// ---- the sweeps -------------------------------------------------------------------------------------------------------

struct SweepPtrs {
  const int *idx;
  const float *Pa, *Pc, *Pq;   // critic sweep: target actor, target critic, critic; actor sweep: actor, critic, unused
  const float *wt_a, *wt_c;
  float *slabs;
  double *part;
};

// the tile's samples: (age, robot), live or not, and how many elements of the window of the state ending at age - back are kept
__device__ __forceinline__ void tile_samples(const Geo &g, const RingDev &ring, const int *__restrict__ idx, const int tile, const long long head,
                                             const long long count, int *s_age, int *s_rob, int *s_live) {
  const int tid = threadIdx.x;
  if (tid < kTile) {
    const int n = tile * kTile + tid;
    int a = 1, b = 0, live = 0;
    if (n < g.M) {
      a = idx[2 * n]; b = idx[2 * n + 1];
      live = a >= 1 && (long long)a < count && b >= 0 && b < g.B;
      if (!live) { a = 1; b = 0; }
    }
    s_age[tid] = a; s_rob[tid] = b; s_live[tid] = live;
  }
}

__global__ void __launch_bounds__(kThreads) rg_ddpg_critic_sweep_kernel(const Geo g, const Net actor_arg, const Net critic_arg, const RingDev ring, const SweepPtrs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ Net s_net[2];
  __shared__ int s_age[kTile], s_rob[kTile], s_live[kTile], s_kept[kTile], s_back[kTile];
  __shared__ double s_y[kTile];
  if (short_ring(ring.state)) return;
  stage_nets(actor_arg, critic_arg, s_net);
  const Net &actor = s_net[0], &critic = s_net[1];
  const int casum = uni(critic.asum), aasum = uni(actor.asum);
  const int tid = threadIdx.x;
  const long long head = ring.state[0], count = ring.state[1];
  float *ca = lds, *aa = ca + casum * kTile;                       // the critic's activations, the actor's
  float *d0 = aa + aasum * kTile, *d1 = d0 + g.dmax * kTile;
  float *slab = p.slabs + (size_t)blockIdx.x * uni(critic.count);
  const int cin = g.act_dim + g.in_s;
  double loss = 0.0;
  clear_slab(critic, slab);
  for (int tile = blockIdx.x; tile < g.ntiles; tile += g.G) {
    __syncthreads();   // the tile before has been read
    tile_samples(g, ring, p.idx, tile, head, count, s_age, s_rob, s_live);
    __syncthreads();
    const float *ahead = aa + (aasum - g.act_dim) * kTile;
    // pass 0: s1 (the state ending at age - 1) through the targets to y; pass 1: [action, s0] through the critic to delta
    for (int pass = 0; pass < 2; pass++) {
      if (tid < kTile) {
        s_back[tid] = s_age[tid] - 1 + pass;
        s_kept[tid] = s_live[tid] ? window_kept(ring.done, head, count, g, s_age[tid] - 1 + pass, s_rob[tid]) : 0;
      }
      __syncthreads();
      fill_state(g, ring.obs, ring.obs, head, s_back, s_rob, s_kept, pass ? ca + g.act_dim * kTile : aa);
      if (pass == 0) {
        forward_net(actor, p.Pa, aa, 1);
        for (int e = tid; e < cin * kTile; e += kThreads) ca[e] = e < g.act_dim * kTile ? ahead[e] : aa[e - g.act_dim * kTile];
      } else {
        for (int e = tid; e < g.act_dim * kTile; e += kThreads) {
          const int k = e / kTile, s = e % kTile;
          ca[e] = s_live[s] ? ring.action[((size_t)slot_of(head, s_age[s], g.C) * g.B + s_rob[s]) * g.act_dim + k] : 0.0f;
        }
      }
      forward_net(critic, pass ? p.Pq : p.Pc, ca, 2);
      if (tid < kTile) {
        const double q = (double)ca[(casum - 1) * kTile + tid];
        if (pass == 0) {
          const size_t k = (size_t)slot_of(head, s_age[tid], g.C) * g.B + s_rob[tid];
          const double nd = ring.done[k] != 0 ? 0.0 : 1.0;
          s_y[tid] = (double)ring.reward[k] + (g.gamma * nd) * q;
        } else {
          float dlt = 0.0f;
          if (s_live[tid]) {
            const double e = q - s_y[tid];
            loss = loss + 0.5 * (e * e);
            dlt = (float)(e / (double)g.M);
          }
          d0[tid] = dlt;
        }
      }
    }
    backward_net(critic, p.wt_c, slab, ca, d0, d1);
  }
  if (tid < kTile) p.part[(size_t)blockIdx.x * kTile + tid] = loss;
}

__global__ void __launch_bounds__(kThreads) rg_ddpg_actor_sweep_kernel(const Geo g, const Net actor_arg, const Net critic_arg, const RingDev ring, const SweepPtrs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ Net s_net[2];
  __shared__ int s_age[kTile], s_rob[kTile], s_live[kTile], s_kept[kTile];
  if (short_ring(ring.state)) return;
  stage_nets(actor_arg, critic_arg, s_net);
  const Net &actor = s_net[0], &critic = s_net[1];
  const int casum = uni(critic.asum), aasum = uni(actor.asum);
  const int tid = threadIdx.x;
  const long long head = ring.state[0], count = ring.state[1];
  float *ca = lds, *aa = ca + casum * kTile;
  float *d0 = aa + aasum * kTile, *d1 = d0 + g.dmax * kTile;
  float *slab = p.slabs + (size_t)blockIdx.x * uni(actor.count);
  const int cin = g.act_dim + g.in_s;
  double loss = 0.0;
  clear_slab(actor, slab);
  for (int tile = blockIdx.x; tile < g.ntiles; tile += g.G) {
    __syncthreads();   // the tile before has been read
    tile_samples(g, ring, p.idx, tile, head, count, s_age, s_rob, s_live);
    __syncthreads();
    if (tid < kTile) s_kept[tid] = s_live[tid] ? window_kept(ring.done, head, count, g, s_age[tid], s_rob[tid]) : 0;
    __syncthreads();
    fill_state(g, ring.obs, ring.obs, head, s_age, s_rob, s_kept, aa);
    forward_net(actor, p.Pa, aa, 1);
    const float *ahead = aa + (aasum - g.act_dim) * kTile;
    for (int e = tid; e < cin * kTile; e += kThreads) ca[e] = e < g.act_dim * kTile ? ahead[e] : aa[e - g.act_dim * kTile];
    forward_net(critic, p.Pc, ca, 2);
    if (tid < kTile) {
      float dlt = 0.0f;
      if (s_live[tid]) {
        loss = loss + (double)ca[(casum - 1) * kTile + tid];
        dlt = (float)(-1.0 / (double)g.M);
      }
      d0[tid] = dlt;
    }
    // backward through the critic's inputs only
    float *dl = d0, *dn = d1;
    for (int l = uni(critic.n) - 1; l >= 0; l--) {
      __syncthreads();
      const int nin = uni(critic.in[l]), nout = uni(critic.out[l]), woff = uni(critic.w[l]);
      if (l > 0) backward_inputs(p.wt_c, nin, nout, woff, ca + input_offset(critic, l), dl, dn);
      else backward_action(p.wt_c, nin, nout, woff, g.act_dim, ahead, dl, dn);
      float *t = dl; dl = dn; dn = t;
    }
    backward_net(actor, p.wt_a, slab, aa, dl, dn);
  }
  if (tid < kTile) p.part[(size_t)blockIdx.x * kTile + tid] = loss;
}

// grad[e] = (float) sum_g slab[g][e], g in order
__global__ void __launch_bounds__(kThreads) rg_ddpg_grad_finish_kernel(const int count, const int G, const float *__restrict__ slabs, float *__restrict__ grad,
                                                                       const long long *__restrict__ gate) {
  if (short_ring(gate)) return;
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= count) return;
  grad[e] = slab_sum(slabs, count, G, e);
}

// loss = sign * (sum of the partials) / M; out2, out3 (optional) receive the loss and its negative
__global__ void __launch_bounds__(kThreads) rg_ddpg_loss_finish_kernel(const int n, const int M, const double sign, const double *__restrict__ part,
                                                                       double *__restrict__ out, double *__restrict__ out2, double *__restrict__ out3,
                                                                       const long long *__restrict__ gate) {
  __shared__ double sh[4];
  if (short_ring(gate)) return;   // uniform
  const double s = strided_sum(part, n, 1, sh);
  if (threadIdx.x == 0) {
    const double mean = s / (double)M;
    *out = sign * mean;
    if (out2) *out2 = sign * mean;
    if (out3) *out3 = -(sign * mean);
  }
}

// ---- Adam, the soft update ----------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rg_ddpg_norm_kernel(const int count, const int GN, const float *__restrict__ grad, double *__restrict__ part,
                                                                const long long *__restrict__ gate) {
  __shared__ double sh[4];
  if (gate && short_ring(gate)) return;   // uniform
  double s = 0.0;
  for (int e = blockIdx.x * kThreads + (int)threadIdx.x; e < count; e += GN * kThreads) { const double v = (double)grad[e]; s = s + v * v; }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

struct AdamCfg {
  int count, GN;
  double lr, b1, b2, eps, clipnorm;
};

__global__ void __launch_bounds__(kThreads) rg_ddpg_adam_kernel(const AdamCfg c, float *__restrict__ p, float *__restrict__ grad, float *__restrict__ m,
                                                                float *__restrict__ v, const long long *__restrict__ step, const double *__restrict__ part,
                                                                double *__restrict__ norm_out, const long long *__restrict__ gate) {
  __shared__ double sh[4];
  if (gate && short_ring(gate)) return;   // uniform
  const double norm = sqrt(strided_sum(part, c.GN, 1, sh));
  if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= c.count) return;
  float gg = grad[e];
  if (c.clipnorm > 0.0 && norm >= c.clipnorm) {
    gg = (float)((double)gg * (c.clipnorm / norm));
    grad[e] = gg;
  }
  const AdamBias bias = adam_bias(c, *step);
  adam_element(c, bias, gg, p, m, v, e);
}

__global__ void rg_ddpg_adam_count_kernel(long long *__restrict__ step, const long long *__restrict__ gate) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && !(gate && short_ring(gate))) *step = *step + 1;
}

__global__ void __launch_bounds__(kThreads) rg_ddpg_soft_update_kernel(const int count, const double tau, float *__restrict__ target,
                                                                       const float *__restrict__ online, const long long *__restrict__ gate) {
  if (gate && short_ring(gate)) return;
  const int e = blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= count) return;
  target[e] = (float)((1.0 - tau) * (double)target[e] + tau * (double)online[e]);
}

__global__ void rg_ddpg_stats_kernel(double *__restrict__ stats) {
  if (blockIdx.x == 0 && threadIdx.x < RG_DDPG_STATS) stats[threadIdx.x] = nan("");
}

thread_local std::string g_create_err;

}  // namespace

struct rg_ddpg_handle {
  rg_ddpg_config cfg{};
  rg_ddpg_layout lay{};
  Net actor{}, critic{};
  Geo geo{};
  int B = 0, device = 0, maxc = 0;
  size_t lds = 0;
  // byte offsets into the workspace
  size_t o_idx = 0, o_part = 0, o_norm = 0, o_grad = 0, o_wt_a = 0, o_wt_c = 0, o_slab = 0, ws_bytes = 0, opt_bytes = 0;
  std::string err;
};

namespace {

bool validate(const rg_ddpg_config *cfg, std::string &err) {
  const IntField ints[] = {{"obs_dim", cfg->obs_dim, 1, RG_DDPG_MAX_OBS}, {"act_dim", cfg->act_dim, 1, RG_DDPG_MAX_ACT}, {"window", cfg->window, 1, RG_DDPG_MAX_WINDOW},
                           {"n_actor_layers", cfg->n_actor_layers, 0, RG_DDPG_MAX_LAYERS}, {"n_critic_layers", cfg->n_critic_layers, 0, RG_DDPG_MAX_LAYERS},
                           {"capacity", cfg->capacity, 2, RG_DDPG_MAX_CAPACITY}, {"minibatch", cfg->minibatch, 1, RG_DDPG_MAX_MINIBATCH}};
  if (!check_abi("config.", cfg->abi_version, RG_DDPG_ABI_VERSION, err) || !check_ints("config.", ints, err)) return false;
  if (cfg->window * cfg->obs_dim > RG_DDPG_MAX_INPUT) {
    char msg[200];
    snprintf(msg, sizeof(msg), "config.window: window * obs_dim = %d above %d", cfg->window * cfg->obs_dim, RG_DDPG_MAX_INPUT);
    err = msg;
    return false;
  }
  const RealField reals[] = {{"gamma", &cfg->gamma, 1, kUnit}, {"tau", &cfg->tau, 1, kUnitPositive}, {"actor_lr", &cfg->actor_lr, 1, kNonNegative},
                             {"critic_lr", &cfg->critic_lr, 1, kNonNegative}, {"beta1", &cfg->beta1, 1, kBelowOne}, {"beta2", &cfg->beta2, 1, kBelowOne},
                             {"adam_eps", &cfg->adam_eps, 1, kPositive}, {"clipnorm", &cfg->clipnorm, 1, kNonNegative},
                             {"ou_theta", &cfg->ou_theta, 1, kNonNegative}, {"ou_mu", &cfg->ou_mu, 1, kFinite}, {"ou_sigma", &cfg->ou_sigma, 1, kNonNegative},
                             {"ou_dt", &cfg->ou_dt, 1, kPositive}};
  return check_widths("config.", "actor_layers", cfg->actor_layers, cfg->n_actor_layers, RG_DDPG_MAX_LAYERS, RG_DDPG_MAX_WIDTH, err) &&
         check_widths("config.", "critic_layers", cfg->critic_layers, cfg->n_critic_layers, RG_DDPG_MAX_LAYERS, RG_DDPG_MAX_WIDTH, err) &&
         check_reals("config.", reals, err);
}

void fill_layout(const rg_ddpg_config *cfg, rg_ddpg_layout &L) {
  std::memset(&L, 0, sizeof(L));
  const int in_s = cfg->window * cfg->obs_dim;
  L.n_actor = cfg->n_actor_layers + 1;
  L.actor_count = layer_layout(in_s, cfg->actor_layers, cfg->n_actor_layers, cfg->act_dim, L.actor_in, L.actor_out, L.actor_w, L.actor_b);
  L.n_critic = cfg->n_critic_layers + 1;
  L.critic_count = layer_layout(cfg->act_dim + in_s, cfg->critic_layers, cfg->n_critic_layers, 1, L.critic_in, L.critic_out, L.critic_w, L.critic_b);
}

void fill_net(const rg_ddpg_layout &L, int net, Net &nd) {
  std::memset(&nd, 0, sizeof(nd));
  nd.n = net ? L.n_critic : L.n_actor;
  nd.count = net ? L.critic_count : L.actor_count;
  for (int l = 0; l < 4; l++) {
    nd.in[l] = net ? L.critic_in[l] : L.actor_in[l]; nd.out[l] = net ? L.critic_out[l] : L.actor_out[l];
    nd.w[l] = net ? L.critic_w[l] : L.actor_w[l]; nd.b[l] = net ? L.critic_b[l] : L.actor_b[l];
  }
  nd.asum = nd.in[0];
  for (int l = 0; l < nd.n; l++) nd.asum += nd.out[l];
}

int hip_fail(rg_ddpg_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_DDPG_ERR_HIP, what, e); }
int no_device(rg_ddpg_handle *h) { return no_device(h, RG_DDPG_ERR_NO_DEVICE, "RG_DDPG"); }
int launch_status(rg_ddpg_handle *h, const char *what) { return launch_status(h, RG_DDPG_ERR_HIP, what); }
int null_arg(rg_ddpg_handle *h, const char *call, const char *name) { return null_arg(h, RG_DDPG_ERR_INVALID, call, name); }

int check_ring(rg_ddpg_handle *h, const char *call, const rg_ddpg_ring *ring, bool obs, bool action, bool reward, bool done) {
  RG_NEED(call, ring, "ring");
  if (obs) RG_NEED(call, ring->obs, "ring.obs");
  if (action) RG_NEED(call, ring->action, "ring.action");
  if (reward) RG_NEED(call, ring->reward, "ring.reward");
  if (done) RG_NEED(call, ring->done, "ring.done");
  RG_NEED(call, ring->state, "ring.state");
  return RG_DDPG_OK;
}

RingDev ring_dev(const rg_ddpg_ring *r) { return RingDev{r->obs, r->action, r->reward, (int *)r->done, (long long *)r->state}; }

unsigned blocks_of(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// ---- the launches of each entry, arguments checked and the device set by the caller ------------------------------------

int run_sample(rg_ddpg_handle *h, const rg_ddpg_ring *ring, int32_t *idx, hipStream_t s) {
  hipLaunchKernelGGL(rg_ddpg_sample_kernel, dim3(blocks_of((size_t)h->geo.M)), dim3(kThreads), 0, s, h->geo.M, h->B, (unsigned long long)h->cfg.seed,
                     (const long long *)ring->state, (int *)idx);
  return launch_status(h, "rg_ddpg_sample_kernel launch");
}

int run_transpose(rg_ddpg_handle *h, const Net &nd, const float *P, float *wt, const long long *gate, hipStream_t s) {
  hipLaunchKernelGGL(rg_ddpg_transpose_kernel, dim3(blocks_of((size_t)nd.count)), dim3(kThreads), 0, s, nd, P, wt, gate);
  return launch_status(h, "rg_ddpg_transpose_kernel launch");
}

int run_finish(rg_ddpg_handle *h, const Net &nd, double sign, void *ws, float *grad, double *loss, double *loss2, double *neg, const long long *gate,
               hipStream_t s) {
  hipLaunchKernelGGL(rg_ddpg_grad_finish_kernel, dim3(blocks_of((size_t)nd.count)), dim3(kThreads), 0, s, nd.count, h->geo.G, ws_at<float>(ws, h->o_slab), grad,
                     gate);
  int rc = launch_status(h, "rg_ddpg_grad_finish_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ddpg_loss_finish_kernel, dim3(1), dim3(kThreads), 0, s, h->geo.G * kTile, h->geo.M, sign, ws_at<double>(ws, h->o_part), loss, loss2, neg,
                     gate);
  return launch_status(h, "rg_ddpg_loss_finish_kernel launch");
}

int run_critic_grad(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const int32_t *idx, const float *cp, const float *tap, const float *tcp, void *ws,
                    float *grad, double *loss, double *loss2, hipStream_t s) {
  const long long *gate = (const long long *)ring->state;
  float *wt_c = ws_at<float>(ws, h->o_wt_c);
  int rc = run_transpose(h, h->critic, cp, wt_c, gate, s);
  if (rc) return rc;
  const SweepPtrs p{(const int *)idx, tap, tcp, cp, nullptr, wt_c, ws_at<float>(ws, h->o_slab), ws_at<double>(ws, h->o_part)};
  hipLaunchKernelGGL(rg_ddpg_critic_sweep_kernel, dim3((unsigned)h->geo.G), dim3(kThreads), h->lds, s, h->geo, h->actor, h->critic, ring_dev(ring), p);
  rc = launch_status(h, "rg_ddpg_critic_sweep_kernel launch");
  if (rc) return rc;
  return run_finish(h, h->critic, 1.0, ws, grad, loss, loss2, nullptr, gate, s);
}

int run_actor_grad(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const int32_t *idx, const float *ap, const float *cp, void *ws, float *grad, double *loss,
                   double *loss2, double *mean_q, hipStream_t s) {
  const long long *gate = (const long long *)ring->state;
  float *wt_a = ws_at<float>(ws, h->o_wt_a), *wt_c = ws_at<float>(ws, h->o_wt_c);
  int rc = run_transpose(h, h->critic, cp, wt_c, gate, s);
  if (!rc) rc = run_transpose(h, h->actor, ap, wt_a, gate, s);
  if (rc) return rc;
  const SweepPtrs p{(const int *)idx, ap, cp, nullptr, wt_a, wt_c, ws_at<float>(ws, h->o_slab), ws_at<double>(ws, h->o_part)};
  hipLaunchKernelGGL(rg_ddpg_actor_sweep_kernel, dim3((unsigned)h->geo.G), dim3(kThreads), h->lds, s, h->geo, h->actor, h->critic, ring_dev(ring), p);
  rc = launch_status(h, "rg_ddpg_actor_sweep_kernel launch");
  if (rc) return rc;
  return run_finish(h, h->actor, -1.0, ws, grad, loss, loss2, mean_q, gate, s);
}

int run_adam(rg_ddpg_handle *h, int which, float *params, float *grad, void *opt, void *ws, double *norm_out, const long long *gate, hipStream_t s) {
  const int ac = h->actor.count, cc = h->critic.count;
  const int count = which == RG_DDPG_ACTOR ? ac : cc;
  float *mom = reinterpret_cast<float *>(static_cast<char *>(opt) + RG_DDPG_OPT_HEADER_BYTES);
  float *m = which == RG_DDPG_ACTOR ? mom : mom + 2 * (size_t)ac;
  long long *step = reinterpret_cast<long long *>(opt) + which;
  int GN = (count + kThreads - 1) / kThreads;
  if (GN > kMaxGroups) GN = kMaxGroups;
  double *part = ws_at<double>(ws, h->o_norm);
  hipLaunchKernelGGL(rg_ddpg_norm_kernel, dim3((unsigned)GN), dim3(kThreads), 0, s, count, GN, (const float *)grad, part, gate);
  int rc = launch_status(h, "rg_ddpg_norm_kernel launch");
  if (rc) return rc;
  const AdamCfg c{count, GN, which == RG_DDPG_ACTOR ? h->cfg.actor_lr : h->cfg.critic_lr, h->cfg.beta1, h->cfg.beta2, h->cfg.adam_eps, h->cfg.clipnorm};
  hipLaunchKernelGGL(rg_ddpg_adam_kernel, dim3(blocks_of((size_t)count)), dim3(kThreads), 0, s, c, params, grad, m, m + count, (const long long *)step,
                     (const double *)part, norm_out, gate);
  rc = launch_status(h, "rg_ddpg_adam_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ddpg_adam_count_kernel, dim3(1), dim3(64), 0, s, step, gate);
  return launch_status(h, "rg_ddpg_adam_count_kernel launch");
}

int run_soft(rg_ddpg_handle *h, int which, float *target, const float *online, const long long *gate, hipStream_t s) {
  const int count = which == RG_DDPG_ACTOR ? h->actor.count : h->critic.count;
  hipLaunchKernelGGL(rg_ddpg_soft_update_kernel, dim3(blocks_of((size_t)count)), dim3(kThreads), 0, s, count, h->cfg.tau, target, online, gate);
  return launch_status(h, "rg_ddpg_soft_update_kernel launch");
}

int run_advance(rg_ddpg_handle *h, const rg_ddpg_ring *ring, hipStream_t s) {
  hipLaunchKernelGGL(rg_ddpg_advance_kernel, dim3(1), dim3(64), 0, s, (long long *)ring->state);
  return launch_status(h, "rg_ddpg_advance_kernel launch");
}

bool bad_which(int32_t which) { return which != RG_DDPG_ACTOR && which != RG_DDPG_CRITIC; }

}  // namespace

extern "C" {

int32_t rg_ddpg_abi_version(void) { return RG_DDPG_ABI_VERSION; }
int32_t rg_ddpg_config_size(void) { return (int32_t)sizeof(rg_ddpg_config); }
int32_t rg_ddpg_layout_size(void) { return (int32_t)sizeof(rg_ddpg_layout); }
int32_t rg_ddpg_ring_size(void) { return (int32_t)sizeof(rg_ddpg_ring); }
int32_t rg_ddpg_tile(void) { return RG_DDPG_TILE; }
const char *rg_ddpg_last_error(const rg_ddpg_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }
int64_t rg_ddpg_workspace_bytes(const rg_ddpg_handle *h) { return h ? (int64_t)h->ws_bytes : -1; }
int64_t rg_ddpg_opt_state_bytes(const rg_ddpg_handle *h) { return h ? (int64_t)h->opt_bytes : -1; }
int32_t rg_ddpg_groups(const rg_ddpg_handle *h) { return h ? h->geo.G : -1; }
int32_t rg_ddpg_lds_bytes(const rg_ddpg_handle *h) { return h ? (int32_t)h->lds : -1; }

int rg_ddpg_param_layout(const rg_ddpg_config *cfg, rg_ddpg_layout *out) {
  if (!cfg || !out) { g_create_err = "param_layout: null config or out"; return RG_DDPG_ERR_INVALID; }
  std::string err;
  if (!validate(cfg, err)) { g_create_err = err; return RG_DDPG_ERR_INVALID; }
  fill_layout(cfg, *out);
  return RG_DDPG_OK;
}

int rg_ddpg_create(const rg_ddpg_config *cfg, int32_t batch, int32_t device, rg_ddpg_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_DDPG_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!validate(cfg, err) || !check_batch(batch, RG_DDPG_MAX_BATCH, err)) { g_create_err = err; return RG_DDPG_ERR_INVALID; }
  rg_ddpg_handle *h = new rg_ddpg_handle();
  h->cfg = *cfg;
  h->B = batch;
  h->device = device;
  fill_layout(cfg, h->lay);
  fill_net(h->lay, 0, h->actor);
  fill_net(h->lay, 1, h->critic);
  Geo &g = h->geo;
  g.B = batch; g.C = cfg->capacity; g.obs_dim = cfg->obs_dim; g.act_dim = cfg->act_dim; g.window = cfg->window;
  g.in_s = cfg->window * cfg->obs_dim;
  g.M = cfg->minibatch;
  g.ntiles = (g.M + kTile - 1) / kTile;
  g.G = g.ntiles < kMaxGroups ? g.ntiles : kMaxGroups;
  g.dmax = 0;
  for (int l = 0; l < h->actor.n; l++) if (h->actor.out[l] > g.dmax) g.dmax = h->actor.out[l];
  for (int l = 0; l < h->critic.n; l++) if (h->critic.out[l] > g.dmax) g.dmax = h->critic.out[l];
  g.gamma = cfg->gamma;
  h->lds = sizeof(float) * (size_t)kTile * (size_t)(h->critic.asum + h->actor.asum + 2 * g.dmax);
  h->maxc = h->actor.count > h->critic.count ? h->actor.count : h->critic.count;
  size_t off = 0;
  h->o_idx = off; off += round8(sizeof(int32_t) * 2 * (size_t)g.M);
  h->o_part = off; off += sizeof(double) * (size_t)g.G * kTile;
  h->o_norm = off; off += sizeof(double) * kMaxGroups;
  h->o_grad = off; off += round8(sizeof(float) * (size_t)h->maxc);
  h->o_wt_a = off; off += round8(sizeof(float) * (size_t)h->actor.count);
  h->o_wt_c = off; off += round8(sizeof(float) * (size_t)h->critic.count);
  h->o_slab = off; off += round8(sizeof(float) * (size_t)g.G * (size_t)h->maxc);
  h->ws_bytes = off;
  h->opt_bytes = round8(RG_DDPG_OPT_HEADER_BYTES + sizeof(float) * 2 * ((size_t)h->actor.count + (size_t)h->critic.count));
  if (device == RG_DDPG_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_DDPG_OK;
  }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_DDPG_ERR_NO_DEVICE, RG_DDPG_ERR_INVALID, RG_DDPG_ERR_HIP, g_create_err)) { delete h; return rc; }
  // the sweeps' tiles need more dynamic LDS than the default limit of a launch.  The attribute belongs to the function and the
  // device, not to the handle: it is set to the most any configuration of the ABI needs, so handles do not undo each other
  hipError_t e = hipFuncSetAttribute((const void *)rg_ddpg_critic_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)rg_ddpg_actor_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
  if (e != hipSuccess) {
    g_create_err = std::string("hipFuncSetAttribute failed: ") + hipGetErrorString(e);
    delete h;
    return RG_DDPG_ERR_HIP;
  }
  *out = h;
  return RG_DDPG_OK;
}

void rg_ddpg_destroy(rg_ddpg_handle *h) { delete h; }

int rg_ddpg_act(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const float *obs, const float *actor_params, float *ou_state, int64_t *act_state,
                int32_t mode, float *action, float *mean, void *stream) {
  if (!h) { g_create_err = "act: null handle"; return RG_DDPG_ERR_INVALID; }
  int rc = check_ring(h, "act", ring, true, false, false, true);
  if (rc) return rc;
  RG_NEED("act", obs, "obs");
  RG_NEED("act", actor_params, "actor_params");
  if (mode != RG_DDPG_MODE_SAMPLE && mode != RG_DDPG_MODE_MEAN) { h->err = "act: mode is neither RG_DDPG_MODE_SAMPLE nor RG_DDPG_MODE_MEAN"; return RG_DDPG_ERR_INVALID; }
  if (mode == RG_DDPG_MODE_SAMPLE) {
    RG_NEED("act", ou_state, "ou_state");
    RG_NEED("act", act_state, "act_state");
  }
  RG_NEED("act", action, "action");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const OuCfg ou{h->cfg.ou_theta, h->cfg.ou_mu, h->cfg.ou_sigma, h->cfg.ou_dt, (unsigned long long)h->cfg.seed};
  hipLaunchKernelGGL(rg_ddpg_act_kernel, dim3(((unsigned)h->B + kTile - 1) / kTile), dim3(kThreads), 0, (hipStream_t)stream, h->geo, h->actor, ou,
                     ring_dev(ring), obs, actor_params, ou_state, (long long *)act_state, mode, action, mean);
  return launch_status(h, "rg_ddpg_act_kernel launch");
}

int rg_ddpg_store(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const float *obs, const float *action, const float *reward, const int32_t *done,
                  float *ou_state, void *stream) {
  if (!h) { g_create_err = "store: null handle"; return RG_DDPG_ERR_INVALID; }
  int rc = check_ring(h, "store", ring, true, true, true, true);
  if (rc) return rc;
  RG_NEED("store", obs, "obs");
  RG_NEED("store", action, "action");
  RG_NEED("store", reward, "reward");
  RG_NEED("store", done, "done");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)h->B * (size_t)(h->cfg.obs_dim + h->cfg.act_dim + 2);
  hipLaunchKernelGGL(rg_ddpg_store_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, h->geo, ring_dev(ring), obs, action, reward, (const int *)done, ou_state);
  rc = launch_status(h, "rg_ddpg_store_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_ddpg_store_advance_kernel, dim3(1), dim3(64), 0, s, h->geo.C, (long long *)ring->state);
  return launch_status(h, "rg_ddpg_store_advance_kernel launch");
}

int rg_ddpg_sample(rg_ddpg_handle *h, const rg_ddpg_ring *ring, int32_t *idx_out, void *stream) {
  if (!h) { g_create_err = "sample: null handle"; return RG_DDPG_ERR_INVALID; }
  int rc = check_ring(h, "sample", ring, false, false, false, false);
  if (rc) return rc;
  RG_NEED("sample", idx_out, "idx_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_sample(h, ring, idx_out, (hipStream_t)stream);
}

int rg_ddpg_critic_grad(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const int32_t *idx, const float *critic_params, const float *target_actor_params,
                        const float *target_critic_params, void *workspace, float *grad_out, double *loss_out, void *stream) {
  if (!h) { g_create_err = "critic_grad: null handle"; return RG_DDPG_ERR_INVALID; }
  int rc = check_ring(h, "critic_grad", ring, true, true, true, true);
  if (rc) return rc;
  RG_NEED("critic_grad", idx, "idx");
  RG_NEED("critic_grad", critic_params, "critic_params");
  RG_NEED("critic_grad", target_actor_params, "target_actor_params");
  RG_NEED("critic_grad", target_critic_params, "target_critic_params");
  RG_NEED("critic_grad", workspace, "workspace");
  RG_NEED("critic_grad", grad_out, "grad_out");
  RG_NEED("critic_grad", loss_out, "loss_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_critic_grad(h, ring, idx, critic_params, target_actor_params, target_critic_params, workspace, grad_out, loss_out, nullptr, (hipStream_t)stream);
}

int rg_ddpg_actor_grad(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const int32_t *idx, const float *actor_params, const float *critic_params,
                       void *workspace, float *grad_out, double *loss_out, void *stream) {
  if (!h) { g_create_err = "actor_grad: null handle"; return RG_DDPG_ERR_INVALID; }
  int rc = check_ring(h, "actor_grad", ring, true, false, false, true);
  if (rc) return rc;
  RG_NEED("actor_grad", idx, "idx");
  RG_NEED("actor_grad", actor_params, "actor_params");
  RG_NEED("actor_grad", critic_params, "critic_params");
  RG_NEED("actor_grad", workspace, "workspace");
  RG_NEED("actor_grad", grad_out, "grad_out");
  RG_NEED("actor_grad", loss_out, "loss_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_actor_grad(h, ring, idx, actor_params, critic_params, workspace, grad_out, loss_out, nullptr, nullptr, (hipStream_t)stream);
}

int rg_ddpg_adam(rg_ddpg_handle *h, int32_t which, float *params, float *grad, void *opt_state, void *workspace, double *norm_out, const int64_t *gate,
                 void *stream) {
  if (!h) { g_create_err = "adam: null handle"; return RG_DDPG_ERR_INVALID; }
  if (bad_which(which)) { h->err = "adam: which is neither RG_DDPG_ACTOR nor RG_DDPG_CRITIC"; return RG_DDPG_ERR_INVALID; }
  RG_NEED("adam", params, "params");
  RG_NEED("adam", grad, "grad");
  RG_NEED("adam", opt_state, "opt_state");
  RG_NEED("adam", workspace, "workspace");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_adam(h, which, params, grad, opt_state, workspace, norm_out, (const long long *)gate, (hipStream_t)stream);
}

int rg_ddpg_soft_update(rg_ddpg_handle *h, int32_t which, float *target, const float *online, const int64_t *gate, void *stream) {
  if (!h) { g_create_err = "soft_update: null handle"; return RG_DDPG_ERR_INVALID; }
  if (bad_which(which)) { h->err = "soft_update: which is neither RG_DDPG_ACTOR nor RG_DDPG_CRITIC"; return RG_DDPG_ERR_INVALID; }
  RG_NEED("soft_update", target, "target");
  RG_NEED("soft_update", online, "online");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_soft(h, which, target, online, (const long long *)gate, (hipStream_t)stream);
}

int rg_ddpg_advance(rg_ddpg_handle *h, const rg_ddpg_ring *ring, void *stream) {
  if (!h) { g_create_err = "advance: null handle"; return RG_DDPG_ERR_INVALID; }
  int rc = check_ring(h, "advance", ring, false, false, false, false);
  if (rc) return rc;
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return run_advance(h, ring, (hipStream_t)stream);
}

int rg_ddpg_update(rg_ddpg_handle *h, const rg_ddpg_ring *ring, float *actor_params, float *critic_params, float *target_actor_params,
                   float *target_critic_params, void *opt_state, void *workspace, int32_t n_updates, double *stats, void *stream) {
  if (!h) { g_create_err = "update: null handle"; return RG_DDPG_ERR_INVALID; }
  int rc = check_ring(h, "update", ring, true, true, true, true);
  if (rc) return rc;
  RG_NEED("update", actor_params, "actor_params");
  RG_NEED("update", critic_params, "critic_params");
  RG_NEED("update", target_actor_params, "target_actor_params");
  RG_NEED("update", target_critic_params, "target_critic_params");
  RG_NEED("update", opt_state, "opt_state");
  RG_NEED("update", workspace, "workspace");
  if (n_updates < 0 || n_updates > RG_DDPG_MAX_UPDATES) {
    char msg[96];
    snprintf(msg, sizeof(msg), "update: n_updates %d outside [0, %d]", n_updates, RG_DDPG_MAX_UPDATES);
    h->err = msg;
    return RG_DDPG_ERR_INVALID;
  }
  RG_NEED("update", stats, "stats");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  const long long *gate = (const long long *)ring->state;
  float *grad = ws_at<float>(workspace, h->o_grad);
  int32_t *idx = ws_at<int32_t>(workspace, h->o_idx);
  hipLaunchKernelGGL(rg_ddpg_stats_kernel, dim3(1), dim3(64), 0, s, stats);
  rc = launch_status(h, "rg_ddpg_stats_kernel launch");
  for (int u = 0; u < n_updates && !rc; u++) {
    rc = run_sample(h, ring, idx, s);
    if (!rc) rc = run_critic_grad(h, ring, idx, critic_params, target_actor_params, target_critic_params, workspace, grad, u == 0 ? stats + 0 : stats + 1,
                                  u == 0 ? stats + 1 : nullptr, s);
    if (!rc) rc = run_adam(h, RG_DDPG_CRITIC, critic_params, grad, opt_state, workspace, stats + 5, gate, s);
    if (!rc) rc = run_actor_grad(h, ring, idx, actor_params, critic_params, workspace, grad, u == 0 ? stats + 2 : stats + 3, u == 0 ? stats + 3 : nullptr,
                                 stats + 4, s);
    if (!rc) rc = run_adam(h, RG_DDPG_ACTOR, actor_params, grad, opt_state, workspace, nullptr, gate, s);
    if (!rc) rc = run_soft(h, RG_DDPG_ACTOR, target_actor_params, actor_params, gate, s);
    if (!rc) rc = run_soft(h, RG_DDPG_CRITIC, target_critic_params, critic_params, gate, s);
    if (!rc) rc = run_advance(h, ring, s);
  }
  return rc;
}

}  // extern "C"
