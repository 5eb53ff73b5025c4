/*
 * rg_bptt.h -- C-ABI of the recurrent PPO policy update on the device in librg_mpc.so: the policy half of RecurrentPPO.update
 * (robot_gym_amd/agents/ppo/recurrent.py) as kernels on the caller's stream, with no host read: the T ticks of rg_rnn.h run
 * forward with every intermediate kept, the float64 head of rg_ppo.h, back-propagation through time through the GRU cell and
 * the dense layers, the weight gradients, Adam, the per-robot KL and the move of the KL penalty.  It reads the rollout slots
 * that rg_rnn_act / rg_policy_record / rg_policy_returns fill and steps the buffer rg_rnn_act reads, in place.  The value
 * network of the recurrent policy is feed-forward: its update is rg_ppo.h's (rg_ppo_prepare, rg_ppo_value_grad, rg_ppo_adam).
 *
 * Conventions (those of rg_ppo.h)
 *   - return 0 on success, a negative rg_bptt_status otherwise; nothing throws across the ABI; rg_bptt_last_error() gives the
 *     text of the last failure on a handle (or of create(), with a NULL handle).
 *   - the CALLER owns every buffer (device memory), the workspace included (rg_bptt_workspace_bytes).  The handle holds the
 *     two configurations and the layouts; it allocates nothing on the device.
 *   - all work is enqueued on the hipStream_t passed in (NULL = default stream); NO call synchronises, stages or copies.
 *   - one handle per (device, stream); calls on one handle are not thread-safe.  Every call leaves the calling thread's
 *     current HIP device as it found it.
 *   - float64 arithmetic is IEEE with floating-point contraction off; the networks are float32, and a float32 product and a
 *     float32 sum are two roundings wherever no fused multiply-add (fma) is written below.  No atomics anywhere: every
 *     result is a function of the inputs, the configuration, T and B alone, never of the device.
 *
 * Buffers.  policy_params float32 [policy_count] in the layout of rg_rnn.h (rg_rnn_param_layout): the dense layers, W_ru,
 * b_ru, W_c, b_c, the head, logstd.  The rollout is rg_ppo.h's rg_ppo_rollout (sample n = t * B + b; obs [T][obs_dim][B],
 * action and mean [T][B][act_dim], logstd [act_dim], adv and mask [T][B]; ret is not read).  reset int32 [T][B] and h0
 * float32 [B][H] are rg_rnn_unroll's.  adv_stats float64 [4] is what rg_ppo_prepare leaves at rg_ppo_scalars_offset: n clamped
 * to 1, m, sd, n; advn = ((double)adv - m) / sd.
 *
 * opt_state (caller, RG_BPTT_OPT_HEADER_BYTES + 4 * 2 * policy_count bytes, which is a multiple of 8; 8-byte aligned;
 * rg_bptt_opt_state_bytes gives the size):
 *   byte  0  int64   step       Adam's step count t of the policy buffer
 *   byte  8  float64 penalty    the KL penalty
 *   byte 16  float32 m[policy_count], v[policy_count]
 * All zeros with penalty = kl_init_penalty is the fresh state.
 *
 * F, the forward pass: the tick of rg_rnn.h to the bit, T times from h0 (with unchanged parameters and normaliser the mean is
 * rg_rnn_unroll's to the bit).  x0 = the observation through the normaliser in float64, rounded to float32 once; a neuron is
 * acc = 0, acc = fma(W[i][j], in[i], acc) over the x inputs in order and then over the h (or r*h) inputs in order, acc + b[j];
 * relu as v > 0 ? v : 0; h = 0 where reset != 0, else the state before (h0 at t = 0); sigmoid(a) = 1.0f / (1.0f + expf(-a));
 * r*h one float32 product; c = tanhf(.); h' = fmaf(u, h, fmaf(-u, c, c)); mean = tanhf(.).  Per sample it keeps x0, the dense
 * activations, h, r, u, c, r*h, h' and the mean in the workspace.
 *
 * H, the head: rg_ppo.h's policy loss per sample in float64 over the float32 mean mu, mu0, action a, logstd, old_logstd
 * (at most 4 components k):
 *   sigma = exp(logstd), sigma0 = exp(old_logstd), D = mu - mu0, z = (a - mu) / sigma, z0 = (a - mu0) / sigma0,
 *   q = (sigma0 * sigma0 + D * D) / (sigma * sigma),  c = 1 (RG_PPO_LOGPDF_EXACT) or 0.5 (RG_PPO_LOGPDF_REFERENCE)
 *   kl    = 0.5 * sum_k [ (q - 1) + 2 * (logstd - old_logstd) ]
 *   ratio = exp( sum_k [ -c * logstd - 0.5 z^2 ] - sum_k [ -c * old_logstd - 0.5 z0^2 ] )
 *   KL_b  = (sum_t valid ? kl : 0) / T  (t in order),  thr = kl_target * kl_cutoff_factor
 *   L     = -(sum_n valid ? ratio * advn : 0) / (T * B) + (sum_b [ penalty * KL_b + coef * [KL_b > thr] * (KL_b - thr)^2 ]) / B
 *   g_b   = penalty + 2 * coef * [KL_b > thr] * (KL_b - thr)
 *   dL/dmu_k     = valid ? (-advn * ratio * z_k / sigma_k + g_b * D_k / sigma_k^2) / (T * B) : 0
 *   delta_mean_k = (float)(dL/dmu_k * (1 - mu_k^2))                 the one rounding into the float32 backward pass
 *   dL/dlogstd_k = sum_n valid ? (-advn * ratio * (z_k^2 - c) + g_b * (1 - q_k)) / (T * B) : 0     float64 throughout
 *   With mu = mu0 and logstd = old_logstd bit for bit: q = 1, kl = 0 and ratio = 1 exactly.
 * The sums over n of L and of dL/dlogstd: P = min(ceil(T * B / 256), 256) workgroups of 256; thread (p, i) takes the samples
 * p * 256 + i, + P * 256, ... in order; a workgroup's 256 partials in a shuffle tree per wave and the four waves in order; the
 * P partials thread i = 0 .. 255 of one workgroup takes i, i + 256, ... in order, then the same tree.  The sum over b of the
 * penalty terms likewise over the robots.
 *
 * B, the delta pass, float32, per robot with t from T - 1 down to 0; dh = 0 before tick T - 1.  A "chain over j" is acc = 0,
 * acc = fma(W[.][.], delta[j], acc) for j in order.  Per tick, with h the state the tick read and x its cell input:
 *   dh        = dh + (chain over a of W_head[i][a] delta_mean[a])
 *   dc = dh * (1 - u);  du = dh * (h - c);  dh_prev = dh * u
 *   delta_c   = dc * (1 - c * c);  delta_u = du * (u * (1 - u))
 *   d(rh)[i]  = chain over j = 0 .. H-1 of W_c[n_x + i][j] delta_c[j]
 *   dr = d(rh) * h;  dh_prev = dh_prev + d(rh) * r;  delta_r = dr * (r * (1 - r))
 *   dh_prev   = dh_prev + (chain over j = 0 .. 2H-1 of W_ru[n_x + i][j] delta_ru[j]),   delta_ru = [delta_r, delta_u]
 *   dx[k]     = one chain over j = 0 .. 2H-1 of W_ru[k][j] delta_ru[j], continued over j = 0 .. H-1 of W_c[k][j] delta_c[j]
 *   the dense layers, last to first: delta_l[k] = (activation_l[k] > 0) ? (dx, or the chain over j of W_{l+1}[k][j]
 *   delta_{l+1}[j]) : 0 (relu'(0) = 0); nothing is formed for the observation.
 *   The dh handed to tick t - 1 is dh_prev where reset[t][b] == 0 and exactly 0 where it is not; nothing flows into h0.  A
 *   masked sample enters with delta_mean = 0 and still carries the dh of later ticks.
 *
 * W, the weight gradients.  For every block (the dense layers, W_ru with input [x, h], W_c with input [x, r*h], the head
 * with input h'), dW[i][j] = sum_n in_n[i] delta_n[j] and db[j] = sum_n delta_n[j] (the chain below with in = 1):
 *   a chunk is RG_BPTT_CHUNK consecutive samples (the last one may be short); inside it v = 0, v = fma(in_n[i], delta_n[j], v)
 *   for n in order, float32; nchunks = ceil(T * B / RG_BPTT_CHUNK), per = ceil(nchunks / min(nchunks, RG_BPTT_MAX_GROUPS)),
 *   G = ceil(nchunks / per): group g owns the chunks g * per .. and adds their v in order in float64; the G float64 partials
 *   are added in index order and the sum is rounded to float32 once.  G is a function of T and B, never of the device.
 *
 * rg_bptt_adam is rg_ppo_adam's arithmetic on the policy buffer (torch.optim.Adam's formula), per element, t = step + 1:
 *   m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * g * g           float32, (float)b1, (float)(1 - b1), ... ; one rounding per operation
 *   p = (float)( p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) )       float64, one rounding;  lr = policy_lr
 *   then step = t.
 * rg_bptt_penalty: kl_change = (sum_b KL_b) / B (thread i takes b = i, i + 256, ... in order, then the tree above);
 *   penalty *= 1.5 when kl_change > 1.3 * kl_target, /= 1.5 when kl_change < 0.7 * kl_target.
 * rg_bptt_update_policy: epochs_policy x (policy_grad, adam); kl; penalty -- the composition of the single entries, launch
 *   for launch.  stats float64 [RG_BPTT_STATS]: policy_loss_first, policy_loss_last (NaN with 0 epochs), kl_change, penalty.
 *   epochs_value, value_lr of the rg_ppo_config are validated and not used.
 *
 * Launches of one gradient.  The transposed copy of W_ru, W_c, the head and the second dense layer into the workspace
 * (refreshed by every gradient call); F: RG_RNN_TILE robots per 256-thread workgroup through all T ticks, one output neuron
 * per thread, the state in LDS; H: one thread per sample (kl), one per robot (KL_b), then the deltas and the partial sums;
 * B: the same tile of robots backwards through the ticks, dh in registers, the deltas of a tick in LDS, the transposed
 * weights read coalesced; W: a grid of (row tiles of RG_BPTT_ROWS input rows of a block) x G, thread j owns column j;
 * then the two finishing sums.  Every entry that launches first writes its descriptor into the head of the workspace with
 * a one-thread kernel.
 *
 * Workspace: per sample 4 * (obs_dim + 2 * sum(dense widths) + 9 * H + 2 * act_dim) + 8 bytes (about 4.5 KB with the default
 * networks), 8 * G * policy_count bytes of float64 partials, two float32 copies of the buffer's size (the transposes, the
 * gradient of update_policy) and less than 64 KB of descriptors and small sums.
 */
#ifndef RG_BPTT_H
#define RG_BPTT_H

#include <stdint.h>
#include "rg_ppo.h"
#include "rg_rnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_BPTT_ABI_VERSION 1
#define RG_BPTT_CHUNK 16                 /* samples per float32 chain of a weight gradient */
#define RG_BPTT_ROWS 16                  /* input rows of a block per workgroup of the W phase */
#define RG_BPTT_MAX_GROUPS 64            /* float64 partials per weight, at most */
#define RG_BPTT_STATS 4
#define RG_BPTT_OPT_HEADER_BYTES 16
#define RG_BPTT_DEVICE_NONE (-1)

typedef enum {
  RG_BPTT_OK = 0,
  RG_BPTT_ERR_INVALID = -1,   /* bad argument / configuration (the text names the field) */
  RG_BPTT_ERR_HIP = -2,       /* HIP runtime error (text in last_error) */
  RG_BPTT_ERR_NO_DEVICE = -3  /* no usable GPU */
} rg_bptt_status;

typedef struct rg_bptt_handle rg_bptt_handle;

/* Validates rnn_cfg (as rg_rnn_create does, the text says "rnn_cfg.<field>"), ppo_cfg field by field ("ppo_cfg.<field>"), T
 * (1 .. RG_RNN_MAX_T), B (1 .. RG_RNN_MAX_BATCH) and T * B (<= RG_PPO_MAX_SAMPLES) BEFORE it looks for a device.  device =
 * RG_BPTT_DEVICE_NONE makes a host-only handle: every later call checks its arguments (RG_BPTT_ERR_INVALID, naming the
 * argument) and, where they are valid, returns RG_BPTT_ERR_NO_DEVICE. */
int rg_bptt_create(const rg_rnn_config *rnn_cfg, const rg_ppo_config *ppo_cfg, int32_t T, int32_t B, int32_t device, rg_bptt_handle **out);
void rg_bptt_destroy(rg_bptt_handle *h);
const char *rg_bptt_last_error(const rg_bptt_handle *h);   /* h may be NULL: the last create() failure of this thread */
int32_t rg_bptt_abi_version(void);
int32_t rg_bptt_tile(void);                                 /* RG_RNN_TILE: robots per workgroup of F and B */
int64_t rg_bptt_workspace_bytes(const rg_bptt_handle *h);  /* 8-byte aligned device memory; nothing is carried in it between calls; < 0: null handle */
int64_t rg_bptt_opt_state_bytes(const rg_bptt_handle *h);
int32_t rg_bptt_groups(const rg_bptt_handle *h);           /* G of the W phase */

/* Reads ro->obs, action, mean, logstd, adv, mask; reset, h0, adv_stats, norm_state float64 [RG_POLICY_NORM_ROWS], policy_params,
 * the penalty of opt_state.  grad_out float32 [policy_count] in the buffer's order (logstd last), loss_out float64 [1]. */
int rg_bptt_policy_grad(rg_bptt_handle *h, const rg_ppo_rollout *ro, const int32_t *reset, const float *h0, const double *adv_stats,
                        const double *norm_state, const float *policy_params, const void *opt_state, void *workspace, float *grad_out,
                        double *loss_out, void *stream);

/* Reads ro->obs, mean, logstd, mask; reset, h0, norm_state, policy_params.  kl_out float64 [B]: KL(behaviour || current) per robot. */
int rg_bptt_kl(rg_bptt_handle *h, const rg_ppo_rollout *ro, const int32_t *reset, const float *h0, const double *norm_state,
               const float *policy_params, void *workspace, double *kl_out, void *stream);

/* One Adam step in place on params (policy_count floats) with grad of the same length; advances the step count of opt_state. */
int rg_bptt_adam(rg_bptt_handle *h, float *params, const float *grad, void *opt_state, void *stream);

/* kl float64 [B] (of rg_bptt_kl).  Moves the penalty of opt_state; stats float64 [2]: kl_change, the new penalty. */
int rg_bptt_penalty(rg_bptt_handle *h, const double *kl, void *opt_state, double *stats, void *stream);

/* The policy's whole update.  policy_params is stepped in place; stats float64 [RG_BPTT_STATS]. */
int rg_bptt_update_policy(rg_bptt_handle *h, const rg_ppo_rollout *ro, const int32_t *reset, const float *h0, const double *adv_stats,
                          const double *norm_state, float *policy_params, void *opt_state, void *workspace, double *stats, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_BPTT_H */
