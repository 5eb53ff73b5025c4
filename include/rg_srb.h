/*
 * rg_srb.h -- C-ABI of the batched single-rigid-body (SRB) simulator of librg_mpc.so.
 *
 * An EXTENSION: the reference simulates in PyBullet, one process per environment.  This is the reduced-order model
 * the convex MPC itself plans with -- one rigid body pushed by the ground-reaction forces at the stance feet -- integrated
 * forward with the controller's own first-step forces and kinematic feet, for B robots per call with no host in the
 * loop.  It is for closed-loop validation of the controller, branched (cloned) rollouts and RL on the reduced model.
 *
 * Stated limits: feet that do not bounce and, in rg_srb_step and rg_srb_step_contact, do not slip; massless legs; first-order
 * (semi-implicit Euler) integration.  Every tick delivers the forces as they are planned unless a motor model stands in front of
 * it (rg_srb_motor_apply, rg_srb_motor.h: a strength and a torque limit per motor).  The ground is the plane z = 0 or a heightfield (rg_srb_set_terrain, below): kinematic
 * feet.  In rg_srb_step touch-down
 * and lift-off follow the gait schedule (the controller's desired_state), not a measurement.  rg_srb_step_contact
 * (rg_srb_contact.h, which states its rule) measures ONE thing on either ground: the early touch-down of a swinging foot, which
 * stops at the ground and reports contact.  rg_srb_step_friction (rg_srb_friction.h, which states its rule and its limits)
 * gives every robot a Coulomb friction coefficient: a stance foot that is asked for more tangential force than the ground
 * holds passes on what the ground holds, and slides.  Still not measured by any entry: late contact, a reach limit of the leg,
 * collision of the body with the ground.  Late contact is left out on purpose: a commanded-stance foot that descends at a
 * finite speed and carries no force until it arrives made every robot of the CPU model fall, on the plane too (rg_srb_contact.h).
 *
 * Conventions (those of rg_posctl.h)
 *   - return 0 on success, a negative rg_srb_status otherwise; nothing throws across the ABI; rg_srb_last_error() gives
 *     the text of the last failure on a handle (or of create(), with a NULL handle).
 *   - the CALLER owns every buffer (device memory, e.g. torch-ROCm tensors passed as data_ptr()), the simulation state
 *     included; the handle holds the configuration and the per-robot true body.
 *   - all work is enqueued on the hipStream_t passed in (NULL = default stream); rg_srb_step never synchronises.
 *     rg_srb_reset and rg_srb_set_body take HOST arrays and wait for their own small host->device copy; nothing else
 *     synchronises.
 *   - one handle per (device, stream); calls on one handle are not thread-safe.  Every call leaves the calling thread's
 *     current HIP device as it found it.
 *   - every value is computed in IEEE float64 with floating-point contraction off; the observation is stored as float32.
 *
 * Simulation state (owned by the caller): double state[RG_SRB_STATE_ROWS][B], component-major, rows
 *      0.. 2  p        CoM position, world
 *      3.. 6  quat     body orientation (x, y, z, w)
 *      7.. 9  v        CoM velocity, world
 *     10..12  w        angular velocity, world
 *     13..24  foot_w   world foot positions, 13 + 3*leg + c, legs FR, FL, RR, RL
 *     25..36  q        motor angles, 25 + 3*leg + joint: the start point of the next leg IK
 *     37..40  stance   per leg: 1 = the foot is on the ground
 *     41      steps    simulation sub-steps since the robot's reset
 *     42      status   0 running, 1 fallen
 *   Integers are stored as exactly representable doubles.  Save, restore and clone are plain copies of columns.
 *
 * One control tick (rg_srb_step), given the controller's outputs of this tick
 *   1. Feet.  A leg whose desired_state is SWING (0) follows its target perfectly: foot_w = p + R foot_target, stance = 0.
 *      Otherwise a foot that was swinging lands where it is (foot_w.z = 0, on a terrain the ground's height there; stance = 1);
 *      a foot on the ground stays (no slip).
 *   2. `substeps` sub-steps of dt_sim with the forces held in the body frame.  With the current rotation R of quat:
 *        f_l = R (-grf_l) for the legs not in SWING (grf is the negated first-step force: the ground pushes with -grf)
 *        F   = ((f_0 + f_1) + (f_2 + f_3)) + m (0, 0, -g) + ext_F
 *        tau = ((r_0 x f_0 + r_1 x f_1) + (r_2 x f_2 + r_3 x f_3)) + ext_tau,   r_l = foot_w_l - p
 *        w  += dt R I^-1 (R' tau - (R' w) x I (R' w))      [ = I_w^-1 (tau - w x I_w w) with I_w = R I R', in the body frame ]
 *        v  += dt F / m ;  p += dt v ;  quat += 1/2 dt (w, 0) (x) quat, then normalised
 *      Semi-implicit Euler in exactly this order; steps += substeps.
 *   3. Fall.  status = 1 if any state value is non-finite, p.z (on a terrain: p.z less the ground's height under the body)
 *      < fall_height_scale * body_height, or the body z axis is
 *      tilted more than fall_tilt from vertical.  A robot whose new state is non-finite keeps its last state (only status
 *      is written).  A fallen robot is frozen: later ticks leave its state and its observation untouched until it is
 *      reset, so nothing non-finite ever reaches the controller.
 *   4. Observation for the next tick, float32 / int32 component-major [c][B] in the layout of rg_mpc_state_ptrs:
 *      rpy (ZYX Euler of R), rpy_rate = R' w, v_world = v, quat, foot_pos_l = R' (foot_w_l - p), contact = stance,
 *      q = damped-Newton leg IK of foot_pos_l started from the stored q (chain, iteration count, damping and step limit of
 *      the configuration: the controller's own leg_ik), jac = the leg's Jacobian at the new q (d foot_i / d joint_j, index
 *      leg*9 + i*3 + j, as rg_mpc_state_ptrs.jac), t_robot = steps * dt_sim (float64).
 *
 * Terrain (rg_srb_set_terrain; an extension of the reference's model/world/terrain.py to the batched model)
 *   The ground is a height h(x, y; robot) over a square lattice of vertices, float64 with contraction off.
 *   RANDOM: the reference's `random` heightfield made stateless and unbounded.  Vertex (i, j) sits at (i cell, j cell) and
 *     its height is amplitude * u(seed, key_robot, i >> 1, j >> 1) (arithmetic shifts: heights are constant over 2 x 2 vertex
 *     groups, as in the reference), u of rg_stream.h over the words (key, I, J), I and J as two's-complement 64-bit
 *     words.
 *     key: a caller-owned int64 [B] device row the caller initialises (robots with equal keys walk the same world); NULL
 *     means key 0 for every robot.  The reference's defaults: cell 0.05, amplitude 0.06.
 *   GRID: caller-owned float64 heights[rows][cols] on the device, heights[i][j] at (x0 + i cell, y0 + j cell), indices
 *     clamped at the edges (the ground goes on at its border value), shared by all robots; rows, cols in 2 .. 4096.
 *   Inside a cell, with s = x / cell (grid: (x - x0) / cell), i = floor(s), u = s - i and likewise t, j, v from y, the cell
 *     is split along the diagonal from (i, j) to (i+1, j+1):
 *        u >= v:  h = h00 + u (h10 - h00) + v (h11 - h10)        otherwise:  h = h00 + u (h11 - h01) + v (h01 - h00)
 *     evaluated left to right; the surface is continuous.  Which diagonal Bullet's heightfield shape uses is not pinned
 *     anywhere this project can read: this is a choice, not a port.
 *   Before the conversion to an integer, s and t are clamped to +-2^40 as fmin(fmax(s, -2^40), 2^40): a NaN becomes the
 *     lower bound, no conversion is undefined, and any state value has a defined ground.
 *   With a terrain set, three rules of the tick change and nothing else:
 *     landing   foot_w.z = h(foot_w.x, foot_w.y) instead of 0.  A swinging foot still follows its target and is not tested
 *               against the ground (rg_srb_step_contact tests it): with amplitude 0 every value is the plane's, bit for bit.
 *     fall      p.z - h(p.x, p.y) < fall_height_scale * body_height
 *     reset     the flat reset followed by rg_srb_settle of the robots reset
 *   Settle (rg_srb_settle), for the robots of a mask whose status is 0: foot_w.z = h_l = h(foot_w.xy) for each foot l,
 *     p.z += ((h_0 + h_1) + (h_2 + h_3)) * 0.25, and the observation rewritten with RG_SRB_RESET_IK_PASSES IK passes from the
 *     stored q.
 */
#ifndef RG_SRB_H
#define RG_SRB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_SRB_ABI_VERSION 1
#define RG_SRB_STATE_ROWS 43
#define RG_SRB_ROW_P 0
#define RG_SRB_ROW_QUAT 3
#define RG_SRB_ROW_V 7
#define RG_SRB_ROW_W 10
#define RG_SRB_ROW_FOOT 13
#define RG_SRB_ROW_Q 25
#define RG_SRB_ROW_STANCE 37
#define RG_SRB_ROW_STEPS 41
#define RG_SRB_ROW_STATUS 42
#define RG_SRB_MAX_BATCH (1 << 24)
#define RG_SRB_MAX_SUBSTEPS 1024
#define RG_SRB_RESET_IK_PASSES 4 /* a reset repeats the leg IK (ik_iters each) until the foot error is below 1e-9 m */

typedef enum {
  RG_SRB_OK = 0,
  RG_SRB_ERR_INVALID = -1,   /* bad argument / configuration (the text names the field) */
  RG_SRB_ERR_HIP = -2,       /* HIP runtime error (text in last_error) */
  RG_SRB_ERR_NO_DEVICE = -3, /* no usable GPU */
  RG_SRB_ERR_ALLOC = -4
} rg_srb_status;

/* The body and kinematic fields of rg_mpc_config (same names, same meaning) and the simulator's own. */
typedef struct {
  int32_t abi_version;      /* RG_SRB_ABI_VERSION */
  int32_t reserved0;        /* must be 0 */
  double mass;              /* default true body: the planner's (rg_srb_set_body changes it per robot) */
  double inertia[9];        /* body frame, row-major */
  double gravity;
  double body_height;       /* default reset height and the scale of the fall threshold */
  double hip[12];           /* hip positions [leg][xyz]: the feet of a reset stand under them */
  double motor_dir[12];
  double motor_off[12];
  double jxyz[36];          /* URDF leg chains, as in rg_mpc_config */
  double jrpy[36];
  double jaxis[36];
  double toe_xyz[12];
  double toe_com[12];
  double base_com[3];
  double init_q[12];        /* INIT_MOTOR_ANGLES of the robot: the start point of the reset's IK */
  int32_t ik_iters;         /* damped-Newton iterations per IK pass (rg_mpc_config.ik_iters) */
  int32_t substeps;         /* sub-steps per control tick: ACTION_REPEAT = 10 */
  double ik_damping;
  double ik_max_step;
  double dt_sim;            /* SIMULATION_TIME_STEP = 0.001 */
  double fall_height_scale; /* 0.5: fallen below this share of body_height */
  double fall_tilt;         /* 1.0 rad: fallen when the body z axis is further than this from vertical */
} rg_srb_config;

/* Where the observation goes: the layout of rg_mpc_state_ptrs with non-const pointers (e.g. the tensors of a PackedState).
 * Every pointer is required. */
typedef struct {
  float *rpy;        /* [3][B] */
  float *rpy_rate;   /* [3][B] body frame */
  float *v_world;    /* [3][B] */
  float *quat;       /* [4][B] x, y, z, w */
  float *q;          /* [12][B] */
  float *foot_pos;   /* [12][B] base frame */
  float *jac;        /* [36][B] */
  int32_t *contact;  /* [4][B] */
  double *t_robot;   /* [B] */
} rg_srb_obs_ptrs;

typedef struct rg_srb_handle rg_srb_handle;

/* Validates cfg (abi_version, reserved0, finite values, positive mass / gravity / body_height / dt_sim, positive definite
 * symmetric inertia, motor_dir +-1, non-zero joint axes, 1 <= ik_iters <= 64, 1 <= substeps <= RG_SRB_MAX_SUBSTEPS,
 * fall_height_scale in [0, 1), fall_tilt in (0, pi]) and batch (1 .. RG_SRB_MAX_BATCH) BEFORE it looks for a device, so a
 * bad configuration is RG_SRB_ERR_INVALID on any machine.  Every robot starts with the configuration's body. */
int rg_srb_create(const rg_srb_config *cfg, int32_t batch, int32_t device, rg_srb_handle **out);
void rg_srb_destroy(rg_srb_handle *h);
const char *rg_srb_last_error(const rg_srb_handle *h);   /* h may be NULL: the last create() failure of this thread */
int32_t rg_srb_abi_version(void);
int32_t rg_srb_config_size(void);
int32_t rg_srb_state_rows(void);

/* The TRUE body of robots idx_host[0..n) (NULL = robots 0..n-1 with n = batch): mass [n], inertia [9][n] (row-major
 * entries, component-major over robots), HOST arrays; either may be NULL (kept).  Both NULL with idx_host NULL and n = 0
 * returns every robot to the configuration's body.  Validated like rg_mpc_set_body (positive finite mass; finite,
 * symmetric, positive definite inertia) before anything is written.  The simulated body may differ from the body the
 * planner believes in. */
int rg_srb_set_body(rg_srb_handle *h, const int32_t *idx_host, int32_t n, const double *mass, const double *inertia, void *stream);

/* Reset of robots idx_host[0..n) (distinct, else RG_SRB_ERR_INVALID; NULL = robots 0..n-1): p = (xy[k], xy[n + k], height[k]), yaw[k], zero
 * velocities, the feet on the ground under the hips (R hip + (x, y), z = 0), all four in stance, q = IK from init_q,
 * steps = 0, status = 0, and the observation written.  HOST arrays; xy NULL = origin, yaw NULL = 0, height NULL =
 * body_height.  Mirrors RobotGymEnv.reset (gym/robot_gym_env.py:81-111).  The controller is reset by its own rg_mpc_reset. */
int rg_srb_reset(rg_srb_handle *h, const int32_t *idx_host, int32_t n, const double *xy, const double *yaw, const double *height,
                 double *state, const rg_srb_obs_ptrs *obs, void *stream);

/* One control tick for every robot (see the top of this file).
 *   state          [RG_SRB_STATE_ROWS][B] float64, read and written
 *   grf            [B][12] float32, foot_target [B][12] float32, desired_state [B][4] int32: rg_mpc_out_ptrs of this tick
 *   ext            [6][B] float64 world force and world torque about the CoM, or NULL
 *   obs            where the observation of the next tick goes */
int rg_srb_step(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *desired_state,
                const double *ext, const rg_srb_obs_ptrs *obs, void *stream);

#ifdef __cplusplus
}
#endif

/* The terrain entries (the ground struct, set_terrain, ground_height, settle): part of this ABI, declared in their own file. */
#include "rg_srb_terrain.h"

/* The tick with measured foot contact (rg_srb_step_contact) and the text of its rule: part of this ABI, declared in its own file. */
#include "rg_srb_contact.h"

/* The tick with Coulomb friction at the stance feet (rg_srb_step_friction), the draw of its coefficient and the text of its
 * rule: part of this ABI, declared in its own file. */
#include "rg_srb_friction.h"

/* The motor model in front of any tick (rg_srb_motor_apply), the draw of its strengths and the text of its rule: part of this
 * ABI, declared in its own file. */
#include "rg_srb_motor.h"

#endif /* RG_SRB_H */
