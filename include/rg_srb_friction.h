/*
 * rg_srb_friction.h -- the tick with Coulomb friction at the stance feet of the C-ABI of the batched single-rigid-body
 * simulator, and the per-episode draw of the coefficient.  Part of rg_srb.h, which includes this file at its end and states
 * the state, the tick, the ground and the conventions at its top; include rg_srb.h, not this file.
 *
 * In rg_srb_step and rg_srb_step_contact the stance-foot force the controller commands is applied whatever it is: the feet
 * never slip.  rg_srb_step_friction gives every robot a friction coefficient mu: a stance foot whose tangential force
 * exceeds mu times its normal force passes on only mu times the normal force, and slides.
 *
 * The rule: a third form of the force rule of step 2 of the tick of rg_srb.h.  Everything else is that tick unchanged: step 1
 * (measured = 0: step 1 of rg_srb.h on the handle's ground, the array being the controller's desired_state, a leg swung iff it
 * is SWING and a swung foot not tested against the ground; measured = 1: step 1 of rg_srb_contact.h, the array being the
 * controller's leg_state), the sub-steps and their order, the fall test, the observation.
 *   The rule applies to robot b iff 0 <= mu[b] < +inf.  Any other value (+inf, NaN, negative) means the robot GRIPS: every
 *   value of its tick is that of rg_srb_step (measured = 0) or rg_srb_step_contact (measured = 1), bit for bit, and its slip is 0.
 *   In every sub-step, for each leg whose stance is 1 after step 1, with f = R fbody as in rg_srb.h:
 *        n = fmax(f.z, 0);  f.z = n                           the ground does not pull
 *        t2 = f.x * f.x + f.y * f.y;  lim = mu * n
 *        t2 <= lim * lim:  the foot sticks, d = 0
 *        otherwise:        the foot slips:
 *                            tn = sqrt(t2);  s = lim / tn;  ux = f.x / tn;  uy = f.y / tn
 *                            d = dt * fmin(slip_gain * (tn - lim), slip_speed_max)
 *                            f.x = f.x * s;  f.y = f.y * s
 *      The torque arm r = foot_w - p of this sub-step uses the foot where it is.  After p is advanced, the slipping foot moves
 *      AGAINST the friction force: foot_w.x -= ux * d, foot_w.y -= uy * d, and slid += d.
 *   After the last sub-step a foot with slid > 0 takes foot_w.z = h(foot_w.xy) on the handle's ground (on the plane nothing
 *   changes): a third ground evaluation per lane.
 *   A NaN anywhere makes the comparison false and takes the slip branch; the foot then becomes non-finite, which the rule of
 *   rg_srb.h handles: the robot keeps its last state.
 *   slip [4][B] holds the metres each foot slid on this tick: a distance, not a flag, on purpose -- it is continuous across
 *   the stick / slip boundary, so the kernel and the model cannot disagree by a branch.
 *
 * slip_gain (m/s per N of excess) and slip_speed_max (m/s) are passed by value.  The Python layer's defaults, 0.01 and 1.0, are
 * CHOICES, NOT MEASUREMENTS: the legs are massless, so a slipping foot has no dynamics of its own and its speed is
 * regularised -- proportional to the force the ground could not hold, capped.
 *
 * Stated limits: the normal is the world z axis, whatever the ground's slope; static and kinetic coefficients are equal; a
 * regularised (viscous) slide, since the legs are massless; one coefficient per robot; no reach limit on a slid foot.  Still
 * not measured by any entry: late contact, a reach limit of the leg, collision of the body with the ground (rg_srb_contact.h).
 *
 * The draw (rg_srb_friction_draw) uses rg_stream.h's stream over the words (key, draw, purpose, index) with the purpose
 * RG_SRB_FRICTION_PURPOSE_MU, block 3 of that header's registry.
 */
#ifndef RG_SRB_FRICTION_H
#define RG_SRB_FRICTION_H

#ifndef RG_SRB_H
#error "include rg_srb.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RG_SRB_FRICTION_PURPOSE_MU 48

/* One control tick with friction for every robot, on whatever ground the handle has (rg_srb_set_terrain).  The conventions
 * of rg_srb_step: enqueued on `stream`, never synchronises, the caller owns every buffer.
 *   state          [RG_SRB_STATE_ROWS][B] float64, read and written
 *   grf            [B][12] float32, foot_target [B][12] float32: rg_mpc_out_ptrs of this tick
 *   leg_state      [B][4] int32: the controller's leg_state (measured = 1) or desired_state (measured = 0)
 *   measured       0 or 1: which step 1 (above)
 *   ext            [6][B] float64 world force and world torque about the CoM, or NULL
 *   obs            where the observation of the next tick goes
 *   mu             [B] float64 DEVICE row, caller-owned: the friction coefficient of each robot
 *   slip_gain      >= 0, finite;  slip_speed_max  >= 0, finite
 *   touch          [4][B] int32 DEVICE array or NULL: as in rg_srb_step_contact; all 0 with measured = 0
 *   slip           [4][B] float64 DEVICE array or NULL: the metres each foot slid on this tick (0 for a robot that is frozen
 *                  or keeps its last state); written for every robot on every tick
 * A NULL or bad argument is RG_SRB_ERR_INVALID and the text names it. */
int rg_srb_step_friction(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *leg_state,
                         int32_t measured, const double *ext, const rg_srb_obs_ptrs *obs, const double *mu, double slip_gain,
                         double slip_speed_max, int32_t *touch, double *slip, void *stream);

/* A coefficient for each robot b with mask[b] != 0; a robot outside the mask is not written:
 *      mu[b] = lo + (hi - lo) * u(seed; word_of(key[b]), word_of(draws[b]), RG_SRB_FRICTION_PURPOSE_MU, 0)
 * Device pointers: mask int32 [B]; key and draws float64 [B] (rows 0 and 1 of the state of rg_dr.h: call it BEFORE rg_dr_reset,
 * which counts the draw, so that both read the same draw count); mu float64 [B].  0 <= lo <= hi, both finite.  One lane per
 * robot; enqueued on `stream`, nothing waits. */
int rg_srb_friction_draw(rg_srb_handle *h, const int32_t *mask, const double *key, const double *draws, uint64_t seed, double lo,
                         double hi, double *mu, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_SRB_FRICTION_H */
