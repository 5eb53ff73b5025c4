// rg_agent_dev.inc -- the device code that rg_policy.hip, rg_ppo.hip and rg_ddpg.hip share: the noise stream, the observation
// transform's arithmetic, the workgroup sums, a layer's forward and backward pass over a tile of 16 samples, and the
// per-element bodies of the transpose, slab-finish and Adam kernels.  The GPU tests demand that the three agree to the bit
// (the update's forward mean is rg_policy_act's, DDPG's noise is the policy's stream), so each of these exists once.
// Included after the including file's `#pragma clang fp contract(off)`: a product and a sum stay two roundings, and every
// fused multiply-add below is an explicit __builtin_fmaf.  Device functions and plain structs only, no kernel: what is not
// called is not emitted.  rg_mpc.hip does not include it, so the source hash behind profiles/ does not move.

namespace {

constexpr int kAgentTile = 16;       // samples per tile of a sweep: a neuron's tile is four float4
constexpr int kAgentThreads = 256;   // threads of a workgroup that calls block_sum or runs a layer: four waves

struct NetDesc {
  int n;                       // layers, the head included
  int in[4], out[4], w[4], b[4];
};

// ---- the noise stream -------------------------------------------------------------------------------------------------

#include "rg_stream_dev.inc"   // the chain over the four words (key, counter, axis, draw)

__device__ __forceinline__ unsigned long long noise_hash(unsigned long long seed, unsigned long long key, unsigned long long counter,
                                                         unsigned long long axis, unsigned long long draw) {
  return mix_word(mix_word(mix_word(mix_word(seed, key), counter), axis), draw);
}

// the standard normal of (seed, key, counter, axis): rg_policy.h, Noise
__device__ __forceinline__ float noise_eps(unsigned long long seed, unsigned long long key, unsigned long long counter, unsigned long long axis) {
  const double u1 = (double)((noise_hash(seed, key, counter, axis, 0) >> 11) + 1ull) * 0x1.0p-53;
  const double u2 = unit53(noise_hash(seed, key, counter, axis, 1));
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

// ---- the normaliser ---------------------------------------------------------------------------------------------------

// 1 / the divisor of StreamingNormalize.transform is never formed: the value is divided, as the reference divides it
__device__ __forceinline__ double norm_scale(double count, double var_sum) {
  return count > 1.0 ? sqrt(var_sum / (count - 1.0) + 1e-4) + 1e-8 : 1.0;
}

__device__ __forceinline__ double clip_sym(double v, double c) { return c > 0.0 ? (v < -c ? -c : (v > c ? c : v)) : v; }

// ---- sums over a workgroup ----------------------------------------------------------------------------------------------

// the sum of v over the workgroup of 256, the same in every thread: a shuffle tree in each wave, the four waves in order.
// Every thread of the workgroup calls it.
__device__ __forceinline__ double block_sum(double v, double *sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
  __syncthreads();   // sh may still be read from the call before
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// sum over idx = 0 .. n-1 of p[idx * stride]: thread t takes t, t + 256, ... in order, then block_sum
__device__ __forceinline__ double strided_sum(const double *__restrict__ p, int n, int stride, double *sh) {
  double s = 0.0;
  for (int idx = threadIdx.x; idx < n; idx += kAgentThreads) s = s + p[(size_t)idx * stride];
  return block_sum(s, sh);
}

// ---- a layer over a tile ------------------------------------------------------------------------------------------------

// y[j][s] = act(sum_i W[i][j] x[i][s] + b[j]): rg_policy_act_kernel's neuron, kAgentTile samples wide.  mode 0 relu, 1 tanhf, 2 linear
__device__ __forceinline__ void forward_layer(const float *__restrict__ P, const int nin, const int nout, const int woff, const int boff,
                                              const float *x, float *y, const int mode) {
  const int j = threadIdx.x;
  if (j < nout) {
    const float *__restrict__ W = P + woff + j;
    float acc[kAgentTile];
#pragma unroll
    for (int r = 0; r < kAgentTile; r++) acc[r] = 0.0f;
#pragma unroll 4
    for (int i = 0; i < nin; i++) {
      const float w = W[(size_t)i * nout];
      const float4 xa = *reinterpret_cast<const float4 *>(x + i * kAgentTile);
      const float4 xb = *reinterpret_cast<const float4 *>(x + i * kAgentTile + 4);
      const float4 xc = *reinterpret_cast<const float4 *>(x + i * kAgentTile + 8);
      const float4 xd = *reinterpret_cast<const float4 *>(x + i * kAgentTile + 12);
      acc[0] = __builtin_fmaf(w, xa.x, acc[0]); acc[1] = __builtin_fmaf(w, xa.y, acc[1]);
      acc[2] = __builtin_fmaf(w, xa.z, acc[2]); acc[3] = __builtin_fmaf(w, xa.w, acc[3]);
      acc[4] = __builtin_fmaf(w, xb.x, acc[4]); acc[5] = __builtin_fmaf(w, xb.y, acc[5]);
      acc[6] = __builtin_fmaf(w, xb.z, acc[6]); acc[7] = __builtin_fmaf(w, xb.w, acc[7]);
      acc[8] = __builtin_fmaf(w, xc.x, acc[8]); acc[9] = __builtin_fmaf(w, xc.y, acc[9]);
      acc[10] = __builtin_fmaf(w, xc.z, acc[10]); acc[11] = __builtin_fmaf(w, xc.w, acc[11]);
      acc[12] = __builtin_fmaf(w, xd.x, acc[12]); acc[13] = __builtin_fmaf(w, xd.y, acc[13]);
      acc[14] = __builtin_fmaf(w, xd.z, acc[14]); acc[15] = __builtin_fmaf(w, xd.w, acc[15]);
    }
    const float bias = P[boff + j];
    float *yj = y + j * kAgentTile;
#pragma unroll
    for (int r = 0; r < kAgentTile; r++) {
      float v = acc[r] + bias;
      if (mode == 0) v = v > 0.0f ? v : 0.0f;
      else if (mode == 1) v = tanhf(v);
      yj[r] = v;
    }
  }
}

// slab[W[i][j]] += sum_s x[i][s] delta[j][s], slab[b[j]] += sum_s delta[j][s]
__device__ __forceinline__ void backward_weights(float *__restrict__ slab, const int nin, const int nout, const int woff, const int boff,
                                                 const float *x, const float *dl) {
  const int j = threadIdx.x;
  if (j < nout) {
    float d[kAgentTile];
#pragma unroll
    for (int q = 0; q < kAgentTile / 4; q++) {
      const float4 v = *reinterpret_cast<const float4 *>(dl + j * kAgentTile + 4 * q);
      d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
    }
    float bs = d[0];
#pragma unroll
    for (int r = 1; r < kAgentTile; r++) bs = bs + d[r];
    slab[boff + j] = slab[boff + j] + bs;
    float *__restrict__ sw = slab + woff + j;
#pragma unroll 4
    for (int i = 0; i < nin; i++) {
      const float4 xa = *reinterpret_cast<const float4 *>(x + i * kAgentTile);
      const float4 xb = *reinterpret_cast<const float4 *>(x + i * kAgentTile + 4);
      const float4 xc = *reinterpret_cast<const float4 *>(x + i * kAgentTile + 8);
      const float4 xd = *reinterpret_cast<const float4 *>(x + i * kAgentTile + 12);
      float v = xa.x * d[0];
      v = __builtin_fmaf(xa.y, d[1], v); v = __builtin_fmaf(xa.z, d[2], v); v = __builtin_fmaf(xa.w, d[3], v);
      v = __builtin_fmaf(xb.x, d[4], v); v = __builtin_fmaf(xb.y, d[5], v); v = __builtin_fmaf(xb.z, d[6], v); v = __builtin_fmaf(xb.w, d[7], v);
      v = __builtin_fmaf(xc.x, d[8], v); v = __builtin_fmaf(xc.y, d[9], v); v = __builtin_fmaf(xc.z, d[10], v); v = __builtin_fmaf(xc.w, d[11], v);
      v = __builtin_fmaf(xd.x, d[12], v); v = __builtin_fmaf(xd.y, d[13], v); v = __builtin_fmaf(xd.z, d[14], v); v = __builtin_fmaf(xd.w, d[15], v);
      const size_t o = (size_t)i * nout;
      sw[o] = sw[o] + v;
    }
  }
}

// acc[s] = sum_j Wt[j][i] dl[j][s] for this thread's input i (an fma chain over j in order)
__device__ __forceinline__ void input_chain(const float *__restrict__ Wt, const int nin, const int nout, const int woff, const float *dl, float *acc) {
  const float *__restrict__ W = Wt + woff + threadIdx.x;
#pragma unroll
  for (int r = 0; r < kAgentTile; r++) acc[r] = 0.0f;
#pragma unroll 4
  for (int j = 0; j < nout; j++) {
    const float w = W[(size_t)j * nin];
    const float4 da = *reinterpret_cast<const float4 *>(dl + j * kAgentTile);
    const float4 db = *reinterpret_cast<const float4 *>(dl + j * kAgentTile + 4);
    const float4 dc = *reinterpret_cast<const float4 *>(dl + j * kAgentTile + 8);
    const float4 dd = *reinterpret_cast<const float4 *>(dl + j * kAgentTile + 12);
    acc[0] = __builtin_fmaf(w, da.x, acc[0]); acc[1] = __builtin_fmaf(w, da.y, acc[1]);
    acc[2] = __builtin_fmaf(w, da.z, acc[2]); acc[3] = __builtin_fmaf(w, da.w, acc[3]);
    acc[4] = __builtin_fmaf(w, db.x, acc[4]); acc[5] = __builtin_fmaf(w, db.y, acc[5]);
    acc[6] = __builtin_fmaf(w, db.z, acc[6]); acc[7] = __builtin_fmaf(w, db.w, acc[7]);
    acc[8] = __builtin_fmaf(w, dc.x, acc[8]); acc[9] = __builtin_fmaf(w, dc.y, acc[9]);
    acc[10] = __builtin_fmaf(w, dc.z, acc[10]); acc[11] = __builtin_fmaf(w, dc.w, acc[11]);
    acc[12] = __builtin_fmaf(w, dd.x, acc[12]); acc[13] = __builtin_fmaf(w, dd.y, acc[13]);
    acc[14] = __builtin_fmaf(w, dd.z, acc[14]); acc[15] = __builtin_fmaf(w, dd.w, acc[15]);
  }
}

// dn[i][s] = x[i][s] > 0 ? sum_j Wt[j][i] dl[j][s] : 0
__device__ __forceinline__ void backward_inputs(const float *__restrict__ Wt, const int nin, const int nout, const int woff, const float *x,
                                                const float *dl, float *dn) {
  const int i = threadIdx.x;
  if (i < nin) {
    float acc[kAgentTile];
    input_chain(Wt, nin, nout, woff, dl, acc);
    const float *xi = x + i * kAgentTile;
    float *di = dn + i * kAgentTile;
#pragma unroll
    for (int r = 0; r < kAgentTile; r++) di[r] = xi[r] > 0.0f ? acc[r] : 0.0f;
  }
}

// ---- per-element bodies of the small kernels ------------------------------------------------------------------------------

// element e of the parameter buffer into the transposed copy: Wt[w[l] + j * in + i] = W[i][j]; the biases are not copied
__device__ __forceinline__ void transpose_element(const NetDesc &nd, const float *__restrict__ P, float *__restrict__ Wt, const int e) {
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (l < nd.n) {
      const int k = e - nd.w[l];
      if (k >= 0 && k < nd.in[l] * nd.out[l]) {
        const int i = k / nd.out[l], j = k - i * nd.out[l];
        Wt[nd.w[l] + j * nd.in[l] + i] = P[e];
      }
    }
  }
}

// (float) sum_g slab[g][e], g in order, in float64
__device__ __forceinline__ float slab_sum(const float *__restrict__ slabs, const int count, const int G, const int e) {
  double s = 0.0;
  for (int g = 0; g < G; g++) s = s + (double)slabs[(size_t)g * count + e];
  return (float)s;
}

// Adam, as the three updates' Adam kernels run it (torch.optim.Adam's order): the bias corrections of the step after `step`
// updates, the same for every element, then element e with gradient gg (DDPG's clips it first): moments in float32, the
// parameter's move in float64.  Cfg is the kernel's own argument struct: its lr, b1, b2 and eps are read where they are used.
// The corrections are formed before a kernel loads its gradient, as each kernel's own text had it: with the load as an
// argument in front of the two pow, rg_ppo_adam_kernel took 34 VGPRs for 33.
struct AdamBias { double bc1, bc2s; };

template <typename Cfg>
__device__ __forceinline__ AdamBias adam_bias(const Cfg &c, const long long step) {
  const double t = (double)(step + 1);
  return AdamBias{1.0 - pow(c.b1, t), sqrt(1.0 - pow(c.b2, t))};
}

template <typename Cfg>
__device__ __forceinline__ void adam_element(const Cfg &c, const AdamBias &bias, const float gg, float *p, float *m, float *v, const int e) {
  const float b1 = (float)c.b1, b2 = (float)c.b2, o1 = (float)(1.0 - c.b1), o2 = (float)(1.0 - c.b2);
  const float t1 = b1 * m[e], t2 = o1 * gg;
  const float mn = t1 + t2;
  const float t3 = b2 * v[e], t4 = gg * gg;
  const float t5 = o2 * t4;
  const float vn = t3 + t5;
  m[e] = mn;
  v[e] = vn;
  const double denom = sqrt((double)vn) / bias.bc2s + c.eps;
  p[e] = (float)((double)p[e] - (c.lr / bias.bc1) * (double)mn / denom);
}

// The Gaussian head of rg_ppo.h, which the two PPO updates share, is rg_ppo_dev.inc, and the GRU tick that the recurrent
// policy's acting kernels and its update share is rg_gru_dev.inc; both are included after this file.

}  // namespace
