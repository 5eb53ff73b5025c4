// rg_gru_dev.inc -- the device code of the GRU policy's tick (include/rg_rnn.h), once, for the acting kernels and for the
// update's forward pass.  The update's means must be the rollout's to the bit ("nothing changed since the rollout" is KL = 0
// and ratio = 1 exactly), so the arithmetic of a tick, the normalised observation and the fmaf chain exist here only.
// Included after rg_agent_dev.inc, and so after the including file's `#pragma clang fp contract(off)`; rg_policy.h and
// rg_rnn.h have been included.  Device functions, constants and plain structs only, no kernel.
//
// A tile of kTile robots per workgroup, one output neuron per thread with kTile accumulators in registers; the activations
// of a layer lie in LDS as x[i][robot] (a thread reads the kTile values of input i as two 16-byte broadcasts); the weight
// W[i][j] is read once per (workgroup, neuron), coalesced along j, and used kTile times.  The sum over i runs in order with
// explicit fmaf: over the x inputs, then over the h (or r*h) inputs.
//
// The tick is gru_stage(s) for s = 0 .. n_dense + 2, a barrier in front of each:
//   s < n_dense       dense relu layer s, ping-pong between the two x buffers
//   s = n_dense       the 2H gates: threads 0 .. H-1 leave r*h, threads H .. 2H-1 leave u
//   s = n_dense + 1   the H candidates; thread j forms h'[j] from its own h[j] and u[j] and writes it over h[j]
//   s = n_dense + 2   the head from h', into the x buffer the cell did not read
// What a stage forms goes to LDS and then to the caller's sink: the acting kernels keep h' alone, the update keeps everything.

namespace {

constexpr int kTile = RG_RNN_TILE;
constexpr int kMaxW = RG_RNN_MAX_WIDTH;
constexpr int kMaxH = RG_RNN_MAX_UNITS;
constexpr int kMaxAct = RG_RNN_MAX_ACT;
constexpr int kCols = RG_POLICY_NORM_COLS;

static_assert(kTile == 8, "a neuron reads the activations of an input as two float4");
static_assert(RG_RNN_MAX_OBS <= RG_POLICY_MAX_OBS && RG_RNN_MAX_OBS <= kMaxW, "norm_state columns");

// acc[r] = fma(W[i * stride], x[i][r], acc[r]) for i = 0 .. nin-1 in order; for a layer W points at W[0][j], stride = its `out`
__device__ __forceinline__ void chain8(const float *__restrict__ W, const int stride, const float *x, const int nin, float (&acc)[kTile]) {
#pragma unroll 8
  for (int i = 0; i < nin; i++) {
    const float w = W[(size_t)i * stride];
    const float4 xa = *reinterpret_cast<const float4 *>(x + i * kTile);
    const float4 xb = *reinterpret_cast<const float4 *>(x + i * kTile + 4);
    acc[0] = __builtin_fmaf(w, xa.x, acc[0]); acc[1] = __builtin_fmaf(w, xa.y, acc[1]);
    acc[2] = __builtin_fmaf(w, xa.z, acc[2]); acc[3] = __builtin_fmaf(w, xa.w, acc[3]);
    acc[4] = __builtin_fmaf(w, xb.x, acc[4]); acc[5] = __builtin_fmaf(w, xb.y, acc[5]);
    acc[6] = __builtin_fmaf(w, xb.z, acc[6]); acc[7] = __builtin_fmaf(w, xb.w, acc[7]);
  }
}

__device__ __forceinline__ float sigmoidf(const float a) { return 1.0f / (1.0f + expf(-a)); }

// observation component i of robot b through the normaliser: float64, rounded to float32 once (rg_policy.h, transform)
__device__ __forceinline__ float normalised(const float *__restrict__ obs, const double *__restrict__ norm, const int i, const int b, const int B,
                                            const double clip) {
  double v = (double)obs[(size_t)i * B + b] - norm[kCols + i];
  v = v / norm_scale(norm[i], norm[2 * kCols + i]);
  return (float)clip_sym(v, clip);
}

// a kernel's descriptor from device memory into its LDS copy, word by word, by a workgroup of kAgentThreads: as scalar
// registers its fields, live through the loop over t, do not fit beside the pointers
template <typename D>
__device__ __forceinline__ const D *descriptor_to_lds(const D *__restrict__ dg, D *dsh) {
  static_assert(sizeof(D) % sizeof(int) == 0, "copied word by word");
  for (int idx = threadIdx.x; idx < (int)(sizeof(D) / sizeof(int)); idx += kAgentThreads)
    reinterpret_cast<int *>(dsh)[idx] = reinterpret_cast<const int *>(dg)[idx];
  __syncthreads();
  return dsh;
}

// stage s of the tick for output neuron j (0 .. 255).  D names the layout as the descriptors of both callers do (n_dense, H,
// n_x, act_dim, dense_in/out/w/b, w_ru, b_ru, w_c, b_c, head_w, head_b).  xs: the two x buffers, x0 in xs[0]; hs, rh, us
// [H][kTile].  After the LDS write of robot r's value the sink receives it:
//   dense(s, nout, j, r, a)       neuron j of dense layer s
//   reset_gate(H, j, r, g, p)     the reset gate g of unit j and p = g * h
//   update_gate(H, j, r, u)       the update gate of unit j
//   cell(H, j, r, c, hn)          the candidate and h' of unit j
template <typename D, typename Sink>
__device__ __forceinline__ void gru_stage(const D *d, const float *__restrict__ pp, const int s, const int j, float (*xs)[kMaxW * kTile], float *hs,
                                          float *rh, float *us, const Sink &sink) {
  const int n_dense = d->n_dense, H = d->H, n_x = d->n_x;
  float acc[kTile];
#pragma unroll
  for (int r = 0; r < kTile; r++) acc[r] = 0.0f;
  if (s < n_dense) {
    const int nin = d->dense_in[s], nout = d->dense_out[s];
    if (j < nout) {
      chain8(pp + d->dense_w[s] + j, nout, xs[s & 1], nin, acc);
      const float bias = pp[d->dense_b[s] + j];
      float *y = xs[(s & 1) ^ 1] + j * kTile;
#pragma unroll
      for (int r = 0; r < kTile; r++) {
        const float v = acc[r] + bias;
        const float a = v > 0.0f ? v : 0.0f;
        y[r] = a;
        sink.dense(s, nout, j, r, a);
      }
    }
  } else if (s == n_dense) {
    if (j < 2 * H) {
      const float *__restrict__ W = pp + d->w_ru + j;
      chain8(W, 2 * H, xs[n_dense & 1], n_x, acc);
      chain8(W + (size_t)n_x * 2 * H, 2 * H, hs, H, acc);
      const float bias = pp[d->b_ru + j];
      if (j < H) {
#pragma unroll
        for (int r = 0; r < kTile; r++) {
          const float g = sigmoidf(acc[r] + bias);
          const float p = g * hs[j * kTile + r];
          rh[j * kTile + r] = p;
          sink.reset_gate(H, j, r, g, p);
        }
      } else {
#pragma unroll
        for (int r = 0; r < kTile; r++) {
          const float g = sigmoidf(acc[r] + bias);
          us[(j - H) * kTile + r] = g;
          sink.update_gate(H, j - H, r, g);
        }
      }
    }
  } else if (s == n_dense + 1) {
    if (j < H) {
      const float *__restrict__ W = pp + d->w_c + j;
      chain8(W, H, xs[n_dense & 1], n_x, acc);
      chain8(W + (size_t)n_x * H, H, rh, H, acc);
      const float bias = pp[d->b_c + j];
#pragma unroll
      for (int r = 0; r < kTile; r++) {
        const float c = tanhf(acc[r] + bias);
        const float u = us[j * kTile + r], h = hs[j * kTile + r];
        const float hn = __builtin_fmaf(u, h, __builtin_fmaf(-u, c, c));
        hs[j * kTile + r] = hn;   // only this thread reads or writes h[j] in this stage
        sink.cell(H, j, r, c, hn);
      }
    }
  } else if (s == n_dense + 2) {
    const int act_dim = d->act_dim;
    if (j < act_dim) {
      chain8(pp + d->head_w + j, act_dim, hs, H, acc);
      const float bias = pp[d->head_b + j];
      float *y = xs[(n_dense & 1) ^ 1] + j * kTile;
#pragma unroll
      for (int r = 0; r < kTile; r++) y[r] = tanhf(acc[r] + bias);
    }
  }
}

}  // namespace
