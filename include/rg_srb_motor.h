/*
 * rg_srb_motor.h -- the motor model of the C-ABI of the batched single-rigid-body simulator: a strength ratio and a torque
 * limit per motor, applied to the controller's forces BEFORE the tick, and the per-episode draw of the strengths.  Part of
 * rg_srb.h, which includes this file at its end and states the state, the tick and the conventions at its top; include
 * rg_srb.h, not this file.
 *
 * The ticks of rg_srb.h apply the controller's first-step forces grf exactly as they are planned: between the MPC and the
 * ground there are no motors.  The reference passes every command through RobotMotorModel.convert_to_torque, which multiplies
 * the torque by a per-motor strength ratio and clips it to a torque limit.  rg_srb_motor_apply is that rule for the stance
 * force: it turns the force of each leg into the joint torques the controller itself commands for it, weakens and clips those,
 * and turns what is left back into the force the leg delivers.  It is a pre-pass, one launch per control tick: the delivered
 * force goes to whichever step entry the caller uses, in place of grf.  The step kernels hold the force in the body frame
 * over their sub-steps, so once per tick is what the rule means.
 *
 * The rule.  One lane per (robot b, leg l), float64 with contraction off, every expression evaluated left to right.  With g
 * the three floats of grf of the leg widened to double, q the leg's three motor angles in rows RG_SRB_ROW_Q + 3l .. + 2 of the
 * state, J the Jacobian of the controller's leg_fk at q (d foot_i / d joint_j, index 3i + j) and mdir the configuration's
 * motor_dir, for the joints j = 0, 1, 2 with m = 3l + j:
 *      tau_j = ((g0 * J[0 + j] + g1 * J[3 + j]) + g2 * J[6 + j]) * mdir[m]        the controller's own tau_stance expression
 *      a_j   = strength[m][b] * tau_j
 *      c_j   = fmin(fmax(a_j, -limit[m][b]), limit[m][b])                         a NaN a_j stays a NaN (fmin and fmax alone
 *                                                                                 would drop it and hand back a limit)
 *      tau_cmd[m][b] = tau_j ;  tau_out[m][b] = c_j
 *   Pass-through.  If c_j == tau_j for all three joints the leg's three floats of grf_out are the BITS of grf: a leg with zero
 *     force (a swinging leg), and every leg under strength 1 with limit +inf, costs nothing and changes nothing.
 *   Otherwise the delivered force g' solves J' g' = c o mdir (o: element by element; mdir is +-1, so multiplying undoes the
 *     multiplication above): Cramer's rule in the operation order of the controller's solve3 on A[3j + i] = J[3i + j], and
 *     grf_out = (float) g'.
 *   Singular leg.  If the determinant is exactly 0.0 the map has no inverse: g' = k g with k = min_j r_j (fmin, j = 0, 1, 2 in
 *     order), r_j = c_j / tau_j where tau_j != 0, else 1.  A non-finite determinant goes through Cramer and yields non-finite
 *     floats, which the tick of rg_srb.h handles: the robot keeps its last state and is marked fallen.  So does a NaN in the
 *     force: its leg, and only its leg, delivers NaN, whatever the limit.
 *
 * Settings the Python layer refuses and this entry takes as they are (nothing here is checked on the device; every case stays
 * inside its leg, and what a leg delivers non-finite the tick of rg_srb.h handles for that robot alone):
 *   strength 0: a_j = +-0, so a leg with force takes the solve on a zero right-hand side and delivers zero, each float with the
 *     sign Cramer's sums give it; tau_out = +-0.
 *   limit 0: c_j = +-0 for every a_j, and the leg delivers zero as under strength 0.
 *   a NaN limit is no limit: fmin and fmax drop a NaN operand, so c_j = a_j, as under +inf.
 *   a negative limit is not an interval: fmax(a_j, -limit) is at least -limit > limit, so c_j is the limit itself, a finite
 *     negative torque, whatever a_j; the leg takes the solve.
 *   +inf strength: a_j = +-inf where tau_j != 0, clipped to a finite limit like any torque; where tau_j == 0 (a swinging leg's
 *     zero force among them) inf * 0 = NaN stays a NaN, and that leg, and only that leg, delivers NaN.
 *   -0.0 and denormal floats in grf are widened exactly (nothing is flushed): a leg of -0.0 has tau_j = +-0 == c_j and passes
 *     through with its signs, a denormal leg passes through by bits or is solved like any other.
 *   an all-zero grf passes through by bits under every finite strength and every limit that is not negative, 0 and NaN
 *     included: c_j = +-0 == tau_j.  Under a negative limit c_j is the limit, so there even a zero-force leg is solved.
 *
 * Stated limits: the legs are massless, so swinging legs are not actuated by this rule (their grf is 0 and passes through);
 * there is no velocity-dependent limit, no back-EMF and no thermal model; near a singularity a bounded torque delivers an
 * unbounded force along the leg, as a rigid straight leg does; the angles read are the simulator's true ones, never a state
 * estimator's.  strength 1 with limit +inf is the identity.
 *
 * The draw (rg_srb_motor_draw) uses rg_stream.h's stream over the words (key, draw, purpose, index) with the purpose
 * RG_SRB_MOTOR_PURPOSE_STRENGTH, the first of block 4 of that header's registry, and the motor as the index.
 */
#ifndef RG_SRB_MOTOR_H
#define RG_SRB_MOTOR_H

#ifndef RG_SRB_H
#error "include rg_srb.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum { RG_SRB_MOTOR_PURPOSE_STRENGTH = 64 };

/* The rule above for every robot and leg of the handle's batch, with the leg chains of the handle's configuration.  The
 * conventions of rg_srb_step_friction: arguments are checked before the handle, the launch is enqueued on `stream`, nothing
 * synchronises, the caller owns every buffer (device memory).
 *   state          [RG_SRB_STATE_ROWS][B] float64: only rows RG_SRB_ROW_Q .. + 11 are read
 *   grf            [B][12] float32: the controller's output of this tick
 *   strength       [12][B] float64: the strength ratio of each motor
 *   torque_limit   [12][B] float64: the torque limit of each motor, N m; +inf: none
 *   grf_out        [B][12] float32: the delivered force.  It may be grf itself: a lane reads its three floats before it writes
 *                  them, and in place gives what out of place gives
 *   tau_cmd        [12][B] float64 or NULL: the torque the controller commands
 *   tau_out        [12][B] float64 or NULL: the torque the motor delivers
 * A NULL or bad argument is RG_SRB_ERR_INVALID and the text names it. */
int rg_srb_motor_apply(rg_srb_handle *h, const double *state, const float *grf, const double *strength, const double *torque_limit,
                       float *grf_out, double *tau_cmd, double *tau_out, void *stream);

/* Twelve strengths for each robot b with mask[b] != 0; a robot outside the mask is not written.  For m = 0 .. 11:
 *      strength[m][b] = lo + (hi - lo) * u(seed; word_of(key[b]), word_of(draws[b]), RG_SRB_MOTOR_PURPOSE_STRENGTH, m)
 * Device pointers: mask int32 [B]; key and draws float64 [B] (rows 0 and 1 of the state of rg_dr.h: call it BEFORE rg_dr_reset,
 * which counts the draw, so that both read the same draw count); strength float64 [12][B].  0 <= lo <= hi, both finite.  One
 * lane per robot; enqueued on `stream`, nothing waits. */
int rg_srb_motor_draw(rg_srb_handle *h, const int32_t *mask, const double *key, const double *draws, uint64_t seed, double lo,
                      double hi, double *strength, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_SRB_MOTOR_H */
