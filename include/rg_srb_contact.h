/*
 * rg_srb_contact.h -- the tick with measured foot contact of the C-ABI of the batched single-rigid-body simulator.  Part of
 * rg_srb.h, which includes this file at its end and states the state, the tick, the ground and the conventions at its top;
 * include rg_srb.h, not this file.
 *
 * In rg_srb_step contact is the gait schedule: a leg whose desired_state is SWING follows its target wherever that leads,
 * through the ground included, and obs.contact is desired_state one tick late.  rg_srb_step_contact MEASURES the early
 * touch-down of a swinging foot: the foot stops at the ground and reports contact, and the controller's own rule
 * (RG_LEG_EARLY_CONTACT, rg_mpc.h) reacts once the swing phase has passed contact_phase_thresh.
 *
 * The rule: a second form of step 1 and of the force rule of step 2 of the tick of rg_srb.h.  Everything else is that tick
 * unchanged: the sub-steps and their order, the fall test, the observation, settle.  The inputs are the controller's
 * leg_state (not desired_state), grf and foot_target of this tick.
 *   1. Feet.  A leg is SWUNG when leg_state is SWING (0) or LOSE_CONTACT (3): the legs for which the controller's swing
 *      action runs.
 *      For a swung leg: c = p + R foot_target and g = h(c.x, c.y) on the handle's ground (the plane: the literal 0).
 *        c.z <= g:   the foot touches: foot_w = (c.x, c.y, g), stance = 1, touch = 1
 *        otherwise:  foot_w = c, stance = 0, touch = 0
 *      For a leg that is not swung (STANCE 1 or EARLY_CONTACT 2) the rule of rg_srb.h: a foot whose stance was 0 lands
 *      where it is (foot_w.z = h(foot_w.xy), stance = 1), a foot on the ground stays; touch = 0.
 *      One ground evaluation per leg: at c.xy or at foot_w.xy.
 *   2. Forces.  f_l = R (-grf_l) for the legs whose stance is 1 AFTER step 1, zero for the others: the ground pushes only
 *      through a foot that is on it.  (In closed loop a touching swung leg has grf = 0 anyway; stated so that any stream of
 *      inputs has one answer.)
 *   obs.contact = stance, as in rg_srb_step: now a measurement.  While leg_state equals desired_state and no swung target
 *   comes to or below the ground, every value is rg_srb_step's, bit for bit.
 *
 * Stated limits.  Measured: the early touch-down of a swinging foot.  Slip is rg_srb_step_friction's (rg_srb_friction.h), in
 * either contact mode.  Still not measured: late contact, a reach limit
 * of the leg, collision of the body with the ground.  Late contact stays out on purpose: with a commanded-stance foot that
 * descends at a finite speed (1 m/s and 0.3 m/s were tried on the CPU model) and gets no force until it arrives, every
 * robot fell, on the plane too -- the LOSE_CONTACT branch of the controller swings such a leg along a swing curve evaluated
 * at the stance phase and the gait never recovers.  A massless leg under stance torque reaches the ground at once, which
 * is what the landing rule says; hence a commanded-stance foot is always planted and LOSE_CONTACT never occurs in closed
 * loop.
 */
#ifndef RG_SRB_CONTACT_H
#define RG_SRB_CONTACT_H

#ifndef RG_SRB_H
#error "include rg_srb.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* One control tick with measured contact for every robot, on whatever ground the handle has (rg_srb_set_terrain).  The
 * conventions of rg_srb_step: enqueued on `stream`, never synchronises, the caller owns every buffer.
 *   state          [RG_SRB_STATE_ROWS][B] float64, read and written
 *   grf            [B][12] float32, foot_target [B][12] float32, leg_state [B][4] int32: rg_mpc_out_ptrs of this tick
 *   ext            [6][B] float64 world force and world torque about the CoM, or NULL
 *   obs            where the observation of the next tick goes
 *   touch          [4][B] int32 DEVICE array or NULL: 1 where a swung foot touched the ground on this tick, else 0 (0 for a
 *                  robot that is frozen or keeps its last state); written for every robot on every tick
 * A NULL argument is RG_SRB_ERR_INVALID and the text names it. */
int rg_srb_step_contact(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *leg_state,
                        const double *ext, const rg_srb_obs_ptrs *obs, int32_t *touch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_SRB_CONTACT_H */
