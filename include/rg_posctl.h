/*
 * rg_posctl.h -- C-ABI of the MI355X-native batched position-mode controllers.
 *
 * The two POSITION-mode plugins of nicrusso7/robot-gym (robot_gym/controllers/), batched over B robots:
 *   - the open-loop Bezier trot, BezierController.update_controller_params (-> loop) followed by get_action
 *     (bezier/bezier_controller.py:154-189, 191-227);
 *   - the body-pose controller, PoseController.get_action (pose/pose_controller.py:54-99), both on the leg IK of
 *     pose/kinematics.py:25-83;
 *   - the POSITION branch of the motor model over the action-repeat loop of one control tick
 *     (model/robots/simple_motor.py:122-140; core/simulation.py:175-179).
 * The library is the same librg_mpc.so as include/rg_mpc.h; these entries have their own prefix and status codes.
 *
 * Conventions (those of rg_mpc.h)
 *   - return 0 on success, a negative rg_posctl_status otherwise; nothing throws across the ABI;
 *     rg_posctl_last_error() gives the text of the last failure on a handle (or of create(), with a NULL handle).
 *   - the CALLER owns every buffer (device memory, e.g. torch-ROCm tensors passed as data_ptr()), the Bezier gait state
 *     included (below); the handle holds only the configuration.
 *   - all work is enqueued on the hipStream_t passed in (NULL = default stream); no hidden synchronisation.
 *   - one handle per (device, stream); calls on one handle are not thread-safe.  Every call leaves the calling thread's
 *     current HIP device as it found it.
 *   - inputs are component-major:  x[c*B + b];  outputs are row-major per robot:  angles[b*12 + k], k = 3*leg + joint,
 *     legs FR, FL, RR, RL, joints (theta, alpha, gamma) of kinematics.solve_IK.
 *   - every value is computed in IEEE float64 (no fast-math, no approximate division); angles are stored as float32.
 *
 * Bezier gait state (owned by the caller): double state[RG_POSCTL_STATE_ROWS][B], component-major, rows
 *     0  phi        gait phase of the last update (BezierController._phi)
 *     1  last_time  clock origin of the phase (_last_time)
 *     2  alpha      rotation angle carried from leg to leg and from tick to tick (_alpha)
 *     3 + 3*leg + c foot frame of leg (FR, FL, RR, RL), component c = x, y, z (_frame)
 *   The constructor state is all zeros; a reset at clock t0 is all zeros except last_time = t0.  Save, restore and clone
 *   are plain copies of columns of this array (add a shift to row 1 to move a state to a shifted clock).
 *
 * Deliberate deviations from the reference classes
 *   1. The clock is the caller's per-robot simulation time (t / t_robot: the plugin's get_time_since_reset), not the
 *      wall clock the reference reads (bezier_controller.py:159-161).  With it the gait is deterministic and batchable.
 *   2. A reset returns a robot to the constructor state with its clock origin at t0 (reference: a no-op, :244-245).
 *      Under a clock that restarts at every environment reset a no-op would leave the phase negative for a period.
 *   3. The pose controller starts from the zero pose (the reference's get_action raises before its first update:
 *      pose_controller.py:14 keeps the orientation as a list, and negates it in get_action, :80).
 */
#ifndef RG_POSCTL_H
#define RG_POSCTL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_POSCTL_ABI_VERSION 1
#define RG_POSCTL_NUM_LEGS 4
#define RG_POSCTL_NUM_MOTORS 12
#define RG_POSCTL_STATE_ROWS 15 /* phi, last_time, alpha, frame[4][3] */
#define RG_POSCTL_PARAMS 4      /* step_length, step_angle (deg), step_rotation, step_period */
#define RG_POSCTL_POSE 6        /* x, y, z, roll, pitch, yaw */
#define RG_POSCTL_MAX_BATCH (1 << 24)
#define RG_POSCTL_MAX_SUBSTEPS 1024

typedef enum {
  RG_POSCTL_OK = 0,
  RG_POSCTL_ERR_INVALID = -1,   /* bad argument / configuration (the text names the field) */
  RG_POSCTL_ERR_HIP = -2,       /* HIP runtime error (text in last_error) */
  RG_POSCTL_ERR_NO_DEVICE = -3, /* no usable GPU */
  RG_POSCTL_ERR_ALLOC = -4
} rg_posctl_status;

/* Everything both controllers read from the robot and their own instance attributes.  Legs are FR, FL, RR, RL and
 * points are [leg][xyz].  Constants local to a reference method (Bezier control points, stance half-length and
 * amplitude, the 0.01 period floor, the 0.99 wrap, the +-0.99 IK clamp) are named constants of the kernels. */
typedef struct {
  int32_t abi_version;      /* RG_POSCTL_ABI_VERSION */
  int32_t reserved0;        /* must be 0 */
  double hip;               /* link lengths: ghost/ctrl_constants.py:48-50 (hip, leg, foot) */
  double leg;
  double foot;
  double hip_v[12];         /* hip vertices hip_*_v, ctrl_constants.py:55-58 */
  double pose_frames[12];   /* PoseController foot frames (+-x_dist/2, +-y_dist/2, -height), pose_controller.py:16-19 */
  double start_frames[12];  /* BezierController._start_frames from its own x_dist 0.23, y_dist 0.155, height 0.22
                               (bezier_controller.py:21-28), not the ctrl constants */
  double leg_offset[4];     /* BezierController._offset = 0, 0, 0.8, 0.8 (:39) */
  double step_offset;       /* stance share of the cycle, 0.5 (:40) */
  double motor_kp[12];      /* MOTOR_POSITION_GAINS ghost/motor_constants.py:13 (rg_posctl_position_to_torque) */
  double motor_kd[12];      /* MOTOR_VELOCITY_GAINS :15 */
} rg_posctl_config;

typedef struct rg_posctl_handle rg_posctl_handle;

/* Validates cfg (finite values, positive link lengths, abi_version, reserved fields) and batch (1 .. RG_POSCTL_MAX_BATCH)
 * BEFORE it looks for a device, so a bad configuration is RG_POSCTL_ERR_INVALID on any machine.  The host then
 * precomputes each leg's r and foot angle from the start frames in float64, as step_trajectory does at every call
 * (bezier_controller.py:121-122). */
int rg_posctl_create(const rg_posctl_config *cfg, int32_t batch, int32_t device, rg_posctl_handle **out);
void rg_posctl_destroy(rg_posctl_handle *h);
const char *rg_posctl_last_error(const rg_posctl_handle *h);   /* h may be NULL: the last create() failure of this thread */
int32_t rg_posctl_abi_version(void);
int32_t rg_posctl_config_size(void);

/* One control tick of the Bezier trot for every robot: update_controller_params (loop, bezier_controller.py:154-189)
 * then get_action (IK of the new frames, :191-227).
 *   t        clock of every robot when t_robot is NULL
 *   t_robot  [B] float64 per-robot clocks, or NULL
 *   params   [4][B] float32: step_length, step_angle (deg), step_rotation, step_period.  NULL advances nothing and writes
 *            the IK of the frames held in state (get_action before any update, or a repeated get_action).
 *   state    [RG_POSCTL_STATE_ROWS][B] float64, read and (params != NULL) written
 *   angles   [B][12] float32 */
int rg_posctl_bezier_step(rg_posctl_handle *h, double t, const double *t_robot, const float *params, double *state,
                          float *angles, void *stream);

/* PoseController.get_action for every robot: pose [6][B] float32 (x, y, z, roll, pitch, yaw) -> angles [B][12] float32. */
int rg_posctl_pose(rg_posctl_handle *h, const float *pose, float *angles, void *stream);

/* RobotMotorModel.convert_to_torque, POSITION branch (simple_motor.py:122-140: -kp (q - q*) - kd qd, strength 1, no torque
 * limit, as robot.py:40-45 builds the model) for S = substeps sub-steps of one control tick, each on the joint state of that
 * sub-step: angles [B][12] float32 (q*), q / qd [S][12][B] float32 -> tau [S][B][12] float32.  The position-mode counterpart
 * of rg_mpc_hybrid_to_torque_substeps. */
int rg_posctl_position_to_torque(rg_posctl_handle *h, const float *angles, const float *q, const float *qd, float *tau,
                                 int32_t substeps, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_POSCTL_H */
