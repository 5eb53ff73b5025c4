/*
 * rg_sensor.h -- C-ABI of the sensor and actuator model of librg_mpc.so: what a policy sees is the clean observation with a
 * per-episode bias, white noise, quantisation, dropout and a per-episode latency, and what it commands reaches the plant with
 * noise and a per-episode latency -- applied on the device to float32 observation rows [D][B] and action rows [B][A], with no
 * host in the loop.  It knows nothing of the simulator: the clean buffers are whatever the caller's task and scan kernels
 * write, which must STAY clean (the go-to task latches its previous path observation), so the model writes buffers of its own.
 *
 * Stated limits
 *   - this model leaves the controller's own state estimate (the simulator's obs tensors) alone: its rpy and quat are both read
 *     by the controller's front kernel, and consistent errors on the two are the design of rg_est.h, the estimator model;
 *   - dropout is per row and per tick: there is no frame-level dropout (all rows of a sensor lost together);
 *   - the noise is white (no correlation over ticks or rows) and has bounded support (`n` of rg_stream.h);
 *   - a robot's delays are drawn at its reset and constant over the episode.
 * Every magnitude is the caller's: the defaults are the identity (no group, delays 0, no action noise), and the identity
 * copies bits (-0.0f, NaN payloads and denormals survive).
 *
 * Conventions (those of rg_episode.h)
 *   - return 0 on success, a negative rg_sensor_status otherwise; nothing throws across the ABI; rg_sensor_last_error() gives
 *     the text of the last failure on a handle (or of create(), with a NULL handle).
 *   - the CALLER owns every buffer (device memory).  The handle holds the configuration only.
 *   - all work is enqueued on the hipStream_t passed in (NULL = default stream); NO call synchronises or stages anything.
 *   - one handle per (device, stream); calls on one handle are not thread-safe.  Every call leaves the calling thread's
 *     current HIP device as it found it.
 *   - every value is computed in IEEE float64 with floating-point contraction off, every expression left to right as
 *     written.  Only integer operations, correctly rounded + - * / , rint (round to nearest, ties to even) and the
 *     conversions float32 <-> float64 are used: there is no log, cos, sqrt or exp, so tests/sensor_model.py restates every
 *     output in numpy bit for bit.
 *
 * The stream is rg_stream.h's: hash, u, ix and n (see there why n is bounded and not a Gaussian) over the words (key, draw,
 * purpose, index).
 *   purpose: 16 observation delay, 17 action delay, 18 bias, 19 observation noise, 20 dropout, 21 action noise
 *   (RG_SENSOR_PURPOSE_*), block 1 of that header's registry.
 *   The row of ix(k, row, j) is the observation row (< 256) or the action component.
 *
 * State (owned by the caller): double sensor_state[RG_SENSOR_ROWS][B], component-major, integers stored as exactly
 * representable doubles, rows
 *      0  key         THE CALLER INITIALISES IT, usually to the robot's index, and nothing here writes it.  The stream is keyed
 *                     by this row (read through int64 to uint64), never by the robot's position in the batch.
 *      1  draws       number of draws (rg_sensor_reset) this robot has had (read like the key)
 *      2  obs_ticks   observations measured since the robot's reset, the reset's own included
 *      3  act_ticks   actions taken since the robot's reset
 *      4  obs_delay   ticks, obs_delay_min .. obs_delay_max
 *      5  act_delay   ticks, act_delay_min .. act_delay_max
 *      6..7           reserved, zero
 *   Rows 2..5 are data the caller may have written: a tick row v is read as k = (uint64) fmin(fmax(v, 0), 2^52) and a delay
 *   row as (uint64) fmin(fmax(v, 0), delay_max) (a NaN is 0), so no value of them addresses outside a ring.
 * and the rings
 *      obs_ring float32 [Lo][D][B],  Lo = obs_delay_max + 1          act_ring float32 [La][A][B],  La = act_delay_max + 1
 * The bias is NOT stored: it is bias_half_width * (2.0 * u(key, draws, 18, row) - 1.0), recomputed on every tick from the
 * draws row, which moves only at a reset.  So save, restore and clone are plain copies of columns of the state, the rings and
 * the delivered buffers (obs_out, act_out).
 *
 * Measurement of row r at tick k, with d = the draw count the episode began with (below) and the settings of the group that
 * holds r:
 *      x = (double) clean[r][b]
 *      x = x + bias_half_width * (2.0 * u(key, d, 18, r) - 1.0)                 skipped where bias_half_width == 0
 *      x = x + noise_sigma * n(key, d, 19, k, r)                                skipped where noise_sigma == 0
 *      x = quantum * rint(x / quantum)                                          skipped where quantum == 0
 *      if u(key, d, 20, ix(k, r, 0)) < dropout_probability:  x = dropout_value  skipped where dropout_probability == 0
 *      measured = (float) x
 *   A skipped step is skipped, not added as zero.  A row in no group, or in a group all four of whose amplitudes
 *   (bias_half_width, noise_sigma, quantum, dropout_probability) are 0, is copied bit for bit.  A non-finite clean value
 *   propagates (a dropout replaces it like any other).
 *   `d` is the same in every entry: rg_sensor_reset measures with the draws row as it finds it and THEN increments it, so
 *   rg_sensor_observe and rg_sensor_act use row 1 minus 1.  (A robot never reset has draws 0; observe and act then use
 *   d = 2^64 - 1, a stream of its own.  Reset every robot once before the first observe.)
 *
 * Launches: one kernel per entry, 256-thread workgroups, no LDS, no atomics.  reset and observe give a robot 8 lanes: a
 * workgroup holds 32 consecutive robots (lane % 32) times 8 row slices (lane / 32), slice s takes the rows s, s + 8, ...; every
 * load and store is row * B + b, a 128-byte run per slice.  The tick and draw rows have one writer per robot (slice 0); every
 * lane of the robot reads them, then the workgroup meets at a barrier, then slice 0 writes.  A robot's lanes are never spread
 * over workgroups.  act is one lane per robot.
 */
#ifndef RG_SENSOR_H
#define RG_SENSOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_SENSOR_ABI_VERSION 1
#define RG_SENSOR_ROWS 8
#define RG_SENSOR_ROW_KEY 0
#define RG_SENSOR_ROW_DRAWS 1
#define RG_SENSOR_ROW_OBS_TICKS 2
#define RG_SENSOR_ROW_ACT_TICKS 3
#define RG_SENSOR_ROW_OBS_DELAY 4
#define RG_SENSOR_ROW_ACT_DELAY 5
#define RG_SENSOR_MAX_GROUPS 4
#define RG_SENSOR_MAX_OBS 256
#define RG_SENSOR_MAX_ACT 8
#define RG_SENSOR_MAX_DELAY 15
#define RG_SENSOR_PURPOSE_OBS_DELAY 16
#define RG_SENSOR_PURPOSE_ACT_DELAY 17
#define RG_SENSOR_PURPOSE_BIAS 18
#define RG_SENSOR_PURPOSE_NOISE 19
#define RG_SENSOR_PURPOSE_DROPOUT 20
#define RG_SENSOR_PURPOSE_ACT_NOISE 21
#define RG_SENSOR_MAX_BATCH (1 << 24)
#define RG_SENSOR_DEVICE_NONE (-1) /* create(): a host-only handle, see rg_sensor_create */

typedef enum {
  RG_SENSOR_OK = 0,
  RG_SENSOR_ERR_INVALID = -1,   /* bad argument / configuration (the text names the field) */
  RG_SENSOR_ERR_HIP = -2,       /* HIP runtime error (text in last_error) */
  RG_SENSOR_ERR_NO_DEVICE = -3, /* no usable GPU */
  RG_SENSOR_ERR_ALLOC = -4
} rg_sensor_status;

/* One group of observation rows [begin, end) and what happens to them.  All zero: unused. */
typedef struct {
  int32_t begin;               /* 0      first row */
  int32_t end;                 /* 0      one past the last row: 0 <= begin < end <= obs_dim */
  double noise_sigma;          /* 0.0    standard deviation of the white noise; >= 0, finite */
  double bias_half_width;      /* 0.0    the episode's bias is uniform in [-w, w); >= 0, finite */
  double dropout_probability;  /* 0.0    chance per row and tick that the row reads dropout_value; in [0, 1] */
  double dropout_value;        /* 0.0    finite */
  double quantum;              /* 0.0    the row is rounded to a multiple of it (ties to even); >= 0, finite; 0: not rounded */
} rg_sensor_group;

/* The defaults (robot_gym_amd/core/sensor_abi.py) are the identity. */
typedef struct {
  int32_t abi_version;         /* RG_SENSOR_ABI_VERSION */
  int32_t obs_dim;             /* D: rows of an observation, 1 .. RG_SENSOR_MAX_OBS */
  uint64_t seed;               /* 0      of the stream */
  int32_t act_dim;             /* A: components of an action, 1 .. RG_SENSOR_MAX_ACT */
  int32_t n_groups;            /* 0      groups in use, 0 .. RG_SENSOR_MAX_GROUPS; disjoint; the entries past them all zero */
  rg_sensor_group groups[RG_SENSOR_MAX_GROUPS];
  int32_t obs_delay_min;       /* 0      ticks: 0 <= min <= max <= RG_SENSOR_MAX_DELAY */
  int32_t obs_delay_max;       /* 0 */
  int32_t act_delay_min;       /* 0      likewise */
  int32_t act_delay_max;       /* 0 */
  double act_noise_sigma[RG_SENSOR_MAX_ACT];   /* 0.0   per component; >= 0, finite; 0 past act_dim */
  double act_fill[RG_SENSOR_MAX_ACT];          /* 0.0   what a delayed actuator applies before the first action arrives; finite; 0 past act_dim */
  int32_t reserved0;           /* must be 0 */
  int32_t reserved1;           /* must be 0 */
} rg_sensor_config;

typedef struct rg_sensor_handle rg_sensor_handle;

/* Validates cfg (every constraint above; the text names the field, "config.groups[1].quantum: ...") and batch
 * (1 .. RG_SENSOR_MAX_BATCH) BEFORE it looks for a device.  device = RG_SENSOR_DEVICE_NONE makes a host-only handle: every
 * later call checks its arguments (RG_SENSOR_ERR_INVALID, naming the argument) and, where they are valid, returns
 * RG_SENSOR_ERR_NO_DEVICE. */
int rg_sensor_create(const rg_sensor_config *cfg, int32_t batch, int32_t device, rg_sensor_handle **out);
void rg_sensor_destroy(rg_sensor_handle *h);
const char *rg_sensor_last_error(const rg_sensor_handle *h);   /* h may be NULL: the last create() failure of this thread */
int32_t rg_sensor_abi_version(void);
int32_t rg_sensor_config_size(void);
int32_t rg_sensor_state_rows(void);

/* A new episode for each robot b with mask[b] != 0; a robot outside the mask is written in no buffer.  Per robot, in this
 * order, with key = row 0:
 *   1. obs_prev non-NULL: obs_prev[r][b] = obs_out[r][b] for every row (the DELIVERED terminal observation)
 *   2. d = row 1 (draws)
 *   3. obs_delay = obs_delay_min + min((uint64)((double)(obs_delay_max - obs_delay_min + 1) * u(key, d, 16, 0)), obs_delay_max - obs_delay_min)
 *      act_delay likewise with act_delay_min, act_delay_max and purpose 17
 *   4. m[r] = the measurement of obs_clean[r][b] at k = 0;  obs_ring[s][r][b] = m[r] for EVERY slot s;  obs_out[r][b] = m[r]
 *   5. act_ring[s][a][b] = (float) act_fill[a] for every slot s
 *   6. rows 4, 5 = obs_delay, act_delay;  row 2 (obs_ticks) = 1;  row 3 (act_ticks) = 0;  row 1 = d + 1
 * Device pointers: mask int32 [B]; sensor_state float64 [RG_SENSOR_ROWS][B]; obs_clean, obs_out, obs_prev float32 [D][B];
 * obs_ring float32 [Lo][D][B]; act_ring float32 [La][A][B].  obs_prev may be NULL; it must not alias obs_out. */
int rg_sensor_reset(rg_sensor_handle *h, const int32_t *mask, double *sensor_state, const float *obs_clean, float *obs_ring, float *obs_out,
                    float *obs_prev, float *act_ring, void *stream);

/* The observation of this tick for EVERY robot, with d = row 1 - 1 and k = row 2 (obs_ticks):
 *      obs_ring[k % Lo][r][b] = the measurement of obs_clean[r][b] at k
 *      obs_out[r][b] = obs_ring[(k + Lo - obs_delay) % Lo][r][b]
 *      row 2 = k + 1
 * Because the reset filled every slot, a robot younger than its delay sees its first measurement: there is no branch. */
int rg_sensor_observe(rg_sensor_handle *h, double *sensor_state, const float *obs_clean, float *obs_ring, float *obs_out, void *stream);

/* The action of this tick for EVERY robot, with d = row 1 - 1 and k = row 3 (act_ticks); act_in and act_out are float32
 * [B][A], robot-major as the task's pre_step reads them, and may be the same buffer:
 *      v = (double) act_in[b][a];  v = v + act_noise_sigma[a] * n(key, d, 21, k, a)   (skipped where the sigma is 0: bits are copied)
 *      act_ring[k % La][a][b] = (float) v
 *      act_out[b][a] = act_ring[(k + La - act_delay) % La][a][b]
 *      row 3 = k + 1
 * Nothing is clipped: the task's pre_step clips to its action box. */
int rg_sensor_act(rg_sensor_handle *h, double *sensor_state, const float *act_in, float *act_ring, float *act_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_SENSOR_H */
