/*
 * rg_ddpg.h -- C-ABI of the DDPG agent on the device in librg_mpc.so: the reference's agents/ddpg (simple_ddpg_agent.py, a
 * keras-rl DDPGAgent) for B robots sharing one replay ring, with no host in the loop: acting with Ornstein-Uhlenbeck noise,
 * the replay ring with keras-rl's window rule, minibatch sampling, the critic's and the actor's gradients (the deterministic
 * policy gradient through the critic), Adam with a global-norm clip, and the soft update of the two target networks.
 *
 * Conventions (those of rg_policy.h / rg_ppo.h)
 *   - return 0 on success, a negative rg_ddpg_status otherwise; nothing throws across the ABI; rg_ddpg_last_error() gives the
 *     text of the last failure on a handle (or of create() / param_layout(), with a NULL handle).  The text names the offending
 *     field or argument.
 *   - the CALLER owns every buffer (device memory), the workspace included (rg_ddpg_workspace_bytes).  The handle holds the
 *     configuration and the layouts; it allocates nothing on the device.
 *   - all work is enqueued on the hipStream_t passed in (NULL = default stream); NO call synchronises, stages or copies.
 *   - one handle per (device, stream); calls on one handle are not thread-safe.  Every call leaves the calling thread's
 *     current HIP device as it found it.
 *   - device = RG_DDPG_DEVICE_NONE makes a host-only handle: every call checks its arguments, then returns NO_DEVICE.
 *   - the networks are float32 with explicit fused multiply-adds in a fixed order; heads, losses and reductions are float64
 *     IEEE with floating-point contraction off.  No atomics anywhere: every result is a function of the inputs and the
 *     configuration alone.
 *
 * Networks.  Actor: window * obs_dim inputs, relu hidden layers, tanh head to act_dim.  Critic: act_dim + window * obs_dim
 * inputs -- THE ACTION FIRST, then the window (the reference's Concatenate([action_input, flattened_observation])) -- relu
 * hidden layers, a linear scalar head.  Parameter buffers follow rg_policy.h's layout rule: per layer W[in][out] (out
 * contiguous) then b[out], layer after layer, the head last; rg_ddpg_param_layout gives the counts and every offset.  Four
 * buffers: actor, critic, target actor, target critic.  A neuron: acc = 0; acc = fma(W[i][j], x[i], acc) for i in order;
 * acc + b[j]; relu as v > 0 ? v : 0, tanhf on the actor's head.
 *
 * opt_state (caller, RG_DDPG_OPT_HEADER_BYTES + 4 * (2 * actor_count + 2 * critic_count) bytes rounded up to 8, 8-byte aligned):
 *   byte  0  int64   step[2]   Adam's step count of the actor, of the critic
 *   byte 16  float32 m_actor[actor_count], v_actor[actor_count], m_critic[critic_count], v_critic[critic_count]
 * All zeros is the fresh state.
 *
 * The replay ring (rg_ddpg_ring, device pointers; C = capacity ticks of all B robots)
 *   obs     float32 [C][obs_dim][B]   the observation acted on
 *   action  float32 [C][B][act_dim]
 *   reward  float32 [C][B]
 *   done    int32   [C][B]
 *   state   int64   [4]               head (next slot written, 0 .. C-1), count (ticks held, at most C), updates, reserved
 * The state lives on the device so that a captured loop needs no host argument that changes.  All zeros is the empty ring.
 *   The tick of age a is slot (head - 1 - a) mod C; it exists iff a < count.
 *   The state of robot b ending at age a is `window` observations, oldest first: element k (0 = newest) is the observation at
 *   age a + k, kept iff a + k < count and no done is set for b at ages a+1 .. a+k; otherwise it is zeros.  (keras-rl's
 *   SequentialMemory pads before an episode's start with zeros; here the rule also covers overwritten slots.)
 *   Transition (a, b), a >= 1: s0 = the state ending at a; action, reward, done those at a; s1 = the state ending at a - 1;
 *   nd = 1 - (done != 0).
 *   Acting: the state is the current observation (element 0) and the ages 0 .. window-2 (element k is age k - 1), cut at a
 *   done at age 0 and beyond.
 *
 * Noise: rg_policy.h's stateless stream, eps(seed, key, counter, axis) with act_state int64 [2][B] (row 0 key, the caller
 * initialises it; row 1 counter, incremented by every sampling act).
 *
 * A SHORT RING (count < 2) holds no transition.  rg_ddpg_sample, critic_grad and actor_grad then write nothing; rg_ddpg_adam,
 * soft_update and advance write nothing when they are given the ring (`gate`); rg_ddpg_update moves nothing (no parameter, no
 * step count, not `updates`) and its stats are NaN.  All of it is decided on the device.
 *
 * rg_ddpg_act (one kernel, RG_DDPG_TILE robots per workgroup of 256, one output neuron per thread, activations in LDS):
 *   mean = actor(state).  SAMPLE: per component one Ornstein-Uhlenbeck step in float64 over the float32 ou_state[B][act_dim],
 *   x = (x + (theta * (mu - x)) * dt) + (sigma * sqrt(dt)) * eps, stored as float32; action = mean + x (float32); counter += 1.
 *   MEAN: action = mean; ou_state and the counter are left alone (both may be NULL).  The action is not clipped: the task clips it.
 * rg_ddpg_store: writes obs, action, reward, done of all B robots at slot head, zeroes the ou_state rows of the robots with
 *   done != 0 (keras-rl's reset_states), then head = (head + 1) mod C, count = min(count + 1, C).  A head outside [0, C) (a ring
 *   state the caller spoilt) is first clamped to the nearest slot, 0 or C - 1, so that no write leaves the ring.
 * rg_ddpg_sample: idx int32 [M][2] = (age, robot), with replacement:
 *   h(draw) = the hash of rg_stream.h over the words (updates, m, draw);  age = 1 + h(0) mod (count - 1),
 *   robot = h(1) mod B (unsigned).
 * rg_ddpg_critic_grad, per sample (age, robot) of idx: a' = target_actor(s1); Q' = target_critic([a', s1]);
 *   y = r + (gamma * nd) * Q' (float64); Q = critic([action, s0]); loss = (sum 0.5 (y - Q)^2) / M (keras-rl's huber_loss with
 *   delta_clip = inf); delta = (float)((Q - y) / M); then the backward pass of rg_ppo.h: through a hidden layer
 *   dx[i] = (x[i] > 0) ? sum_j W[i][j] delta[j] : 0 (an fma chain over j in order, relu'(0) = 0), weights read from a
 *   transposed copy in the workspace; dW[i][j] = sum x[i] delta[j], db[j] = sum delta[j]: a float32 fma chain over a tile's
 *   samples in order, a float32 running sum over the tiles a workgroup walks (tile g, g + G, ...) in the workgroup's own slab,
 *   a float64 sum over the G = min(ceil(M / RG_DDPG_TILE), RG_DDPG_MAX_GROUPS) workgroups in index order, rounded to float32
 *   once.  Padded samples of a ragged tile contribute exact zeros; so does a sample whose age is outside [1, count - 1] or
 *   whose robot is outside [0, B).
 * rg_ddpg_actor_grad: mu = actor(s0) (activations kept); Q = critic([mu, s0]); loss = -(sum Q) / M; delta_Q = (float)(-1 / M);
 *   backward through the critic's inputs only (no critic weight gradients; relu gates on the hidden layers, none on the
 *   input layer); the act_dim action components g_k of the input gradient (float32) become the actor head's delta
 *   (float)((double)g_k * (1 - mu_k^2)); backward through the actor with weight gradients as above.
 * rg_ddpg_adam(which): norm = sqrt(sum g^2) over the whole buffer in float64 (per workgroup a strided sum and a shuffle tree,
 *   the workgroups in a fixed order); when norm >= clipnorm > 0 every g becomes (float)((double)g * (clipnorm / norm)), IN
 *   PLACE in grad; then rg_ppo.h's Adam (torch.optim.Adam's formula), t = step + 1:
 *     m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * g * g        float32, one rounding per operation
 *     p = (float)( p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) )     float64, one rounding
 *   then step = t.  Keras places epsilon differently (lr_t * m / (sqrt(v) + eps) with the bias corrections folded into lr_t,
 *   and keras-rl's clipnorm clips per tensor list the same global way): parity with a Keras run is to Adam's epsilon.
 * rg_ddpg_soft_update: target = (float)((1 - tau) * target + tau * online) in float64.
 * rg_ddpg_update(n_updates): stats = NaN; then per update, IN THIS ORDER (the project's choice: the reference leaves the place
 *   of the soft update relative to the step to TensorFlow's scheduling):
 *     sample; critic_grad with the targets as they are; adam(critic); actor_grad with the stepped critic; adam(actor); the soft
 *     update of both targets toward the stepped networks; updates += 1 (rg_ddpg_advance).
 *   stats float64 [RG_DDPG_STATS]: critic_loss_first, critic_loss_last, actor_loss_first, actor_loss_last, mean_q_last (the
 *   critic's mean over the last minibatch at the actor's actions), critic_grad_norm_last (before the clip).  It is the
 *   composition of the single entries, launch for launch.
 *
 * Launches.  The two gradient sweeps: G workgroups of 256 threads, each owning a tile of RG_DDPG_TILE samples through every
 * network, both networks' activations and two delta buffers in dynamic LDS: (act_dim + in + sum(critic out) + in + sum(actor
 * out) + 2 * widest) * RG_DDPG_TILE floats, 148 032 bytes at the limits: one workgroup per compute unit.
 */
#ifndef RG_DDPG_H
#define RG_DDPG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_DDPG_ABI_VERSION 1
#define RG_DDPG_MAX_OBS 64
#define RG_DDPG_MAX_ACT 4
#define RG_DDPG_MAX_WINDOW 8
#define RG_DDPG_MAX_INPUT 128            /* window * obs_dim */
#define RG_DDPG_MAX_LAYERS 3
#define RG_DDPG_MAX_WIDTH 256
#define RG_DDPG_MAX_CAPACITY (1 << 20)
#define RG_DDPG_MAX_MINIBATCH (1 << 16)
#define RG_DDPG_MAX_BATCH (1 << 24)
#define RG_DDPG_MAX_UPDATES (1 << 20)    /* n_updates of one rg_ddpg_update */
#define RG_DDPG_TILE 16                  /* samples (robots, in act) per tile */
#define RG_DDPG_MAX_GROUPS 256           /* workgroups of a sweep, at most */
#define RG_DDPG_STATS 6
#define RG_DDPG_OPT_HEADER_BYTES 16
#define RG_DDPG_RING_STATE 4             /* int64 entries of rg_ddpg_ring.state */
#define RG_DDPG_DEVICE_NONE (-1)
#define RG_DDPG_MODE_SAMPLE 0
#define RG_DDPG_MODE_MEAN 1
#define RG_DDPG_ACTOR 0                  /* `which` of rg_ddpg_adam / rg_ddpg_soft_update */
#define RG_DDPG_CRITIC 1

typedef enum {
  RG_DDPG_OK = 0,
  RG_DDPG_ERR_INVALID = -1,   /* bad argument / configuration (the text names the field) */
  RG_DDPG_ERR_HIP = -2,       /* HIP runtime error (text in last_error) */
  RG_DDPG_ERR_NO_DEVICE = -3  /* no usable GPU */
} rg_ddpg_status;

/* The defaults (robot_gym_amd/core/ddpg_abi.py) are the reference's simple_ddpg_agent.py. */
typedef struct {
  int32_t abi_version;       /* RG_DDPG_ABI_VERSION */
  int32_t obs_dim;           /* 16     1 .. RG_DDPG_MAX_OBS */
  int32_t act_dim;           /* 2      1 .. RG_DDPG_MAX_ACT */
  int32_t window;            /* 5      1 .. RG_DDPG_MAX_WINDOW; window * obs_dim <= RG_DDPG_MAX_INPUT */
  int32_t n_actor_layers;    /* 3      hidden layers of the actor (0 .. RG_DDPG_MAX_LAYERS) */
  int32_t n_critic_layers;   /* 3      hidden layers of the critic (0 .. RG_DDPG_MAX_LAYERS) */
  int32_t actor_layers[3];   /* 128, 128, 64    widths (1 .. RG_DDPG_MAX_WIDTH); entries past n_actor_layers must be 0 */
  int32_t critic_layers[3];  /* 256, 256, 128   likewise */
  int32_t capacity;          /* caller's choice   ticks in the ring, 2 .. RG_DDPG_MAX_CAPACITY */
  int32_t minibatch;         /* 32     M, 1 .. RG_DDPG_MAX_MINIBATCH */
  double gamma;              /* 0.99   in [0, 1] */
  double tau;                /* 1e-3   in (0, 1] */
  double actor_lr;           /* 1e-3   finite, >= 0 */
  double critic_lr;          /* 1e-3   finite, >= 0 */
  double beta1;              /* 0.9    in [0, 1) */
  double beta2;              /* 0.999  in [0, 1) */
  double adam_eps;           /* 1e-8   finite, > 0 */
  double clipnorm;           /* 1.0    finite, >= 0; 0 = off */
  double ou_theta;           /* 0.5    finite, >= 0 */
  double ou_mu;              /* 0.4    finite */
  double ou_sigma;           /* 0.3    finite, >= 0 */
  double ou_dt;              /* 1e-2   finite, > 0 */
  uint64_t seed;             /* of the noise stream and of the sample stream */
} rg_ddpg_config;

/* Layers count the head: n_actor = n_actor_layers + 1.  Offsets are in floats from the start of the net's buffer. */
typedef struct {
  int32_t actor_count;       /* floats in an actor buffer */
  int32_t critic_count;      /* floats in a critic buffer */
  int32_t n_actor;
  int32_t n_critic;
  int32_t actor_in[4], actor_out[4], actor_w[4], actor_b[4];
  int32_t critic_in[4], critic_out[4], critic_w[4], critic_b[4];
} rg_ddpg_layout;

typedef struct {
  float *obs;
  float *action;
  float *reward;
  int32_t *done;
  int64_t *state;
} rg_ddpg_ring;

typedef struct rg_ddpg_handle rg_ddpg_handle;

/* Validates cfg field by field (the text names the field) and batch (1 .. RG_DDPG_MAX_BATCH) BEFORE it looks for a device. */
int rg_ddpg_create(const rg_ddpg_config *cfg, int32_t batch, int32_t device, rg_ddpg_handle **out);
void rg_ddpg_destroy(rg_ddpg_handle *h);
const char *rg_ddpg_last_error(const rg_ddpg_handle *h);   /* h may be NULL: the last create() / param_layout() failure of this thread */
int32_t rg_ddpg_abi_version(void);
int32_t rg_ddpg_config_size(void);
int32_t rg_ddpg_layout_size(void);
int32_t rg_ddpg_ring_size(void);
int32_t rg_ddpg_tile(void);
int64_t rg_ddpg_workspace_bytes(const rg_ddpg_handle *h);   /* 8-byte aligned device memory; it carries nothing between calls; < 0: null handle */
int64_t rg_ddpg_opt_state_bytes(const rg_ddpg_handle *h);
int32_t rg_ddpg_groups(const rg_ddpg_handle *h);            /* G of the sweeps */
int32_t rg_ddpg_lds_bytes(const rg_ddpg_handle *h);         /* dynamic LDS of a sweep's workgroup */

/* The layout rule for cfg (validated as in create).  Needs no device. */
int rg_ddpg_param_layout(const rg_ddpg_config *cfg, rg_ddpg_layout *out);

/* obs float32 [obs_dim][B] (the current observation); reads ring->obs, done, state.  actor_params float32 [actor_count];
 * ou_state float32 [B][act_dim] and act_state int64 [2][B] may be NULL with mode = RG_DDPG_MODE_MEAN; action float32 [B][act_dim];
 * mean float32 [B][act_dim] or NULL. */
int rg_ddpg_act(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const float *obs, const float *actor_params, float *ou_state, int64_t *act_state,
                int32_t mode, float *action, float *mean, void *stream);

/* obs float32 [obs_dim][B] (the observation that was acted on), action float32 [B][act_dim], reward float32 [B], done int32 [B];
 * ou_state float32 [B][act_dim] or NULL. */
int rg_ddpg_store(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const float *obs, const float *action, const float *reward, const int32_t *done,
                  float *ou_state, void *stream);

/* idx_out int32 [M][2]; reads ring->state alone. */
int rg_ddpg_sample(rg_ddpg_handle *h, const rg_ddpg_ring *ring, int32_t *idx_out, void *stream);

/* idx int32 [M][2].  grad_out float32 [critic_count], loss_out float64 [1]. */
int rg_ddpg_critic_grad(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const int32_t *idx, const float *critic_params, const float *target_actor_params,
                        const float *target_critic_params, void *workspace, float *grad_out, double *loss_out, void *stream);

/* grad_out float32 [actor_count], loss_out float64 [1]. */
int rg_ddpg_actor_grad(rg_ddpg_handle *h, const rg_ddpg_ring *ring, const int32_t *idx, const float *actor_params, const float *critic_params,
                       void *workspace, float *grad_out, double *loss_out, void *stream);

/* One clipped Adam step in place on params (actor_count or critic_count floats by `which`); grad is scaled in place when the clip
 * acts; advances that buffer's step count in opt_state.  norm_out float64 [1] or NULL: the norm before the clip.  gate: ring->state
 * or NULL; given, a short ring makes the call write nothing. */
int rg_ddpg_adam(rg_ddpg_handle *h, int32_t which, float *params, float *grad, void *opt_state, void *workspace, double *norm_out,
                 const int64_t *gate, void *stream);

/* target and online: actor_count or critic_count floats by `which`.  gate as above. */
int rg_ddpg_soft_update(rg_ddpg_handle *h, int32_t which, float *target, const float *online, const int64_t *gate, void *stream);

/* updates += 1 in ring->state (nothing on a short ring). */
int rg_ddpg_advance(rg_ddpg_handle *h, const rg_ddpg_ring *ring, void *stream);

/* n_updates (0 .. RG_DDPG_MAX_UPDATES) whole updates.  The four parameter buffers and opt_state are stepped in place; stats
 * float64 [RG_DDPG_STATS]. */
int rg_ddpg_update(rg_ddpg_handle *h, const rg_ddpg_ring *ring, float *actor_params, float *critic_params, float *target_actor_params,
                   float *target_critic_params, void *opt_state, void *workspace, int32_t n_updates, double *stats, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_DDPG_H */
