// rg_front_kernel.inc -- per-(robot, leg) front kernel: gait, velocity filter, swing leg, stance record, binning
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// ------------------------------------------------------------------------------------
// front kernel
// ------------------------------------------------------------------------------------
// Gait timing of one (robot, leg): the config-wide constants, or the robot's own row of the arrays set by
// rg_mpc_set_gait (BASELINE config 5: per-robot random duty factor).
struct LegGait { double stance, duty, phase0; int init; };
// (address selects, not branches: the four loads leave with the front kernel's first block of loads)
__device__ __forceinline__ LegGait load_leg_gait(const DevCfg *c, const DevState &st, int leg, int b, int B) {
  LegGait g;
  const bool own = st.g_stance != nullptr;
  g.stance = *(own ? st.g_stance + (leg * B + b) : c->stance_dur + leg);
  g.duty = *(own ? st.g_duty + (leg * B + b) : c->duty + leg);
  g.phase0 = *(own ? st.g_phase + (leg * B + b) : c->init_phase + leg);
  g.init = *((own && st.g_init) ? st.g_init + (leg * B + b) : c->init_state + leg);
  return g;
}

// Open-loop gait, bit-exact with the float64 reference arithmetic: no FMA contraction.
__device__ inline void gait_leg(const LegGait &g, double thresh, double t, int contact, int &desired, int &leg_state, double &phase) {
#pragma clang fp contract(off)
  int init = g.init;
  int next = (init == RG_LEG_SWING) ? RG_LEG_STANCE : RG_LEG_SWING;
  double ratio = (init == RG_LEG_SWING) ? 1.0 - g.duty : g.duty;
  double full = g.stance / g.duty;
  double aug = t + g.phase0 * full;
  double ph = fmod(aug, full) / full;
  if (ph < ratio) { desired = init; phase = ph / ratio; }
  else { desired = next; phase = (ph - ratio) / (1.0 - ratio); }
  leg_state = desired;
  if (!(phase < thresh)) {
    if (leg_state == RG_LEG_SWING && contact) leg_state = RG_LEG_EARLY_CONTACT;
    if (leg_state == RG_LEG_STANCE && !contact) leg_state = RG_LEG_LOSE_CONTACT;
  }
}

// Open-loop desired state of one leg at horizon step k (contact-schedule extension): t + k*dt without FMA
// contraction, like the float64 CPU arithmetic.
__device__ inline int gait_desired_at(const LegGait &g, double thresh, double dt, double t, int k) {
  const double tk = __dadd_rn(t, __dmul_rn((double)k, dt));
  int desired, ls; double ph;
  gait_leg(g, thresh, tk, 1, desired, ls, ph);
  return desired;
}

// Swing-leg inverse kinematics of one (robot, leg) lane -- Newton steps with a forward-kinematics pass each, one dependent
// chain of ~7.5 us -- and the only consumer of its result: the q* entries of the command row for the leg's joints.  It used
// to sit in the middle of the front kernel (a third of that kernel's 20 us, and what put it at 256 VGPRs + 60 AGPRs of
// spill space); nothing between the front kernel and the end of the tick needs the angles, so the lanes now run as EXTRA
// workgroups at the end of the tick's QP launch (indices >= batch: dispatched last, into the idle tail of that launch) and
// own the q* entries of joints that emit a position command -- the QP output stage and the front kernel's no-stance-leg
// path write every other entry of the row.  A leg that does not swing this tick hands out its stored angles.
__device__ __forceinline__ void swing_ik_lane(const DevCfg *__restrict__ c, const DevState &st, const DevOut &out, const int B, const int gid) {
  if (gid >= 4 * B) return;
  const int b = gid >> 2, leg = gid & 3;
  const int emit = (int)st.rec[(size_t)b * RG_REC_N + REC_EMIT];
  const int flag = st.ik_flag[gid];
  double swq[3];
  if (flag & 1) {
    const size_t n4 = (size_t)4 * B;
    const double target[3] = {st.ik_in[gid], st.ik_in[n4 + gid], st.ik_in[2 * n4 + gid]};
    const double q0[3] = {st.ik_in[3 * n4 + gid], st.ik_in[4 * n4 + gid], st.ik_in[5 * n4 + gid]};
    leg_ik(c, leg, target, q0, swq);
    // a non-finite IK result (a target the Newton steps blow up on) must neither leave as a position command nor be stored --
    // a leg that does not swing re-emits the stored angles on the following ticks: counted as a failure of this tick, and the
    // leg holds its current joint angles
    if (!(fabs(swq[0]) + fabs(swq[1]) + fabs(swq[2]) <= 1.0e300)) {
      atomicAdd(&st.counts[7], 1);
#pragma unroll
      for (int j = 0; j < 3; j++) swq[j] = q0[j];
    } else {
#pragma unroll
      for (int j = 0; j < 3; j++) st.swing_q[(size_t)(3 * leg + j) * B + b] = swq[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 3; j++) swq[j] = st.swing_q[(size_t)(3 * leg + j) * B + b];
  }
#pragma unroll
  for (int j = 0; j < 3; j++)
    if ((emit >> (3 * leg + j)) & 1) out.action[(size_t)b * 60 + 5 * (3 * leg + j)] = (float)swq[j];
}
// the plan without a QP launch (exact solver under a contact schedule) runs the lanes as a launch of their own
__global__ void __launch_bounds__(64) rg_swing_ik_kernel(const DevCfg *__restrict__ c, DevState st, DevOut out, int B) {
  swing_ik_lane(c, st, out, B, blockIdx.x * blockDim.x + threadIdx.x);
}

// One lane per (robot, leg): the four lanes of a quad share a robot.  Per-leg work (gait state, swing
// target / trajectory / IK, FK, lever arms) runs in parallel; per-robot values are combined with
// quad ballots/shuffles and written by the leg-0 lane.  (A lane-per-robot version left 4096 robots
// on 64 waves with a ~290k-cycle serial chain each.)
// The kernel is one wave per CU and bound by its chain of DEPENDENT memory round trips, so it is ordered around them:
//   (1) every load whose address depends on nothing but (robot, leg) -- inputs, gait rows, the robot's persistent state
//       including what the swing and work-list code need much later -- is issued in the first block;
//   (2) the velocity window's oldest samples (address = the robot's ring head, a value of (1)) are requested as soon as (1) is in;
//   (3) the work-list slot (a returning device-scope atomic, ~1.5 us) is requested as soon as the stance legs are known --
//       its result is consumed at the very end, after the filter, swing and record arithmetic.
// The same loads in the order the arithmetic wants them were five to six round trips one after the other.
__global__ void __launch_bounds__(64)
rg_front_kernel(const DevCfg *__restrict__ c, DevState st, DevIn in, DevOut out, double t_now, int B) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gid >> 2, leg = gid & 3;
  if (gid < RG_NCOUNTS) st.counts_next[gid] = 0;
  if (gid == 0 && st.audit_k > 0) st.audit_cnt[st.audit_ring] = 0;   // audit lane: this tick's picks start from an empty ring entry
  if (b >= B) return;  // B*4 is padded to whole quads by construction (4 lanes per robot)
  const int lane = threadIdx.x & 63, qbase = lane & ~3;
  const int W = c->window;
  // ---- (1) inputs and persistent state ----
  double rpy[3], rate[3], vw[3], quat[4], q3[3], cmd[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { rpy[i] = in.rpy[i * B + b]; rate[i] = in.rpy_rate[i * B + b]; vw[i] = in.v_world[i * B + b]; }
#pragma unroll
  for (int i = 0; i < 4; i++) quat[i] = in.quat[i * B + b];
#pragma unroll
  for (int i = 0; i < 3; i++) q3[i] = in.q[(3 * leg + i) * B + b];
  const int contact = in.contact[leg * B + b];
  const float *cmdp = in.cmd ? in.cmd : st.cmd;
#pragma unroll
  for (int i = 0; i < 3; i++) cmd[i] = cmdp[i * B + b];
  const int flags = st.flags[b];
  const int rlen = st.ring_len[b], rhead = st.ring_head[b];
  const double t_reset = st.reset_time[b];
  double fsum[3], fcorr[3], lat[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { fsum[a] = st.fsum[a * B + b]; fcorr[a] = st.fcorr[a * B + b]; lat[a] = st.latched[(3 * leg + a) * B + b]; }
  const int last = st.last_desired[b];
  const int valid_old = st.swing_valid[b];
  // (optional arrays: the load goes to an array that always exists and the value is dropped -- a branch here would make the
  // loads above wait for it)
  const int hard_prev = st.hard[b], ncs_prev = st.ncs[b], it_prev = st.iters[b], ws_cnt_raw = (st.ws_cnt ? st.ws_cnt : st.ncs)[b];   // (work lists, below)
  const double t_rob_raw = (in.t_robot ? in.t_robot : st.reset_time)[b];
  const int sched_raw = (in.contact_sched ? in.contact_sched : in.contact)[leg * B + b];   // caller's contact schedule (contact_lookahead)
  // hip positions: the robot's body row (rg_mpc_set_body), else the config's
  double hip[3];
  if (c->body) {
#pragma unroll
    for (int a = 0; a < 3; a++) hip[a] = c->body[(size_t)b * RG_BODY_N + BODY_HIP + 3 * leg + a];
  } else {
#pragma unroll
    for (int a = 0; a < 3; a++) hip[a] = c->hip[3 * leg + a];
  }
  const LegGait gt = load_leg_gait(c, st, leg, b, B);
  double foot[3], jac[9];
  {
    static_assert(2 * RG_REC_N >= 36, "the record slab covers the indices of a [36][B] float array");
    const bool fk = c->kin_mode == 1;   // chain geometry on the device: the caller's arrays may be absent, the loads go to the record slab (never used)
    const float *fpp = fk ? (const float *)st.rec : in.foot_pos, *jpp = fk ? (const float *)st.rec : in.jac;
#pragma unroll
    for (int i = 0; i < 3; i++) foot[i] = fpp[(3 * leg + i) * B + b];
#pragma unroll
    for (int i = 0; i < 9; i++) jac[i] = jpp[(9 * leg + i) * B + b];
  }
  const int ws_cnt_prev = st.ws_cnt ? ws_cnt_raw : 0;
  const double t_rob = in.t_robot ? t_rob_raw : t_now;
  // ---- (2) the samples the velocity window drops this tick (read whether or not the window is full: the slot exists) ----
  double ring_old[3];
#pragma unroll
  for (int a = 0; a < 3; a++) ring_old[a] = (double)st.ring[((size_t)a * W + rhead) * B + b];
  // failure detection: a non-finite input would come out of the QP as finite nonsense (fmin/fmax in the projection
  // drop NaNs), so it is caught here: the robot is counted ONCE (rg_mpc_last_solver_stats().failures), gets an all-zero
  // command row, takes no QP slot and leaves its persistent state untouched (a NaN pushed into the velocity filter
  // would otherwise poison the next `window` ticks).  Same for a per-robot gait row that is out of range.
  if (c->kin_mode == 1) leg_fk(c, leg, q3, foot, jac);
  bool ok;
  {
    double chk = rpy[0] + rpy[1] + rpy[2] + rate[0] + rate[1] + rate[2] + vw[0] + vw[1] + vw[2] + quat[0] + quat[1] + quat[2] + quat[3]
               + q3[0] + q3[1] + q3[2] + cmd[0] + cmd[1] + cmd[2] + foot[0] + foot[1] + foot[2];
#pragma unroll
    for (int i = 0; i < 9; i++) chk += jac[i];
    if (in.t_robot) chk += t_rob;
    const bool gait_bad = !(gt.stance > 0.0 && gt.duty > 0.0 && gt.duty <= 1.0 && fabs(gt.phase0) <= 1.0e300) || (gt.init != RG_LEG_SWING && gt.init != RG_LEG_STANCE);
    const int quad_bad = (int)((__ballot(!(fabs(chk) <= 1.0e300) || gait_bad) >> qbase) & 0xF);
    ok = quad_bad == 0;
    if (leg == 0 && !ok) atomicAdd(&st.counts[7], 1);
  }
  // the latched foot position (start of the swing trajectory): kept in registers from here on, written back where it changes
  if ((flags & 1) && ok) {
#pragma unroll
    for (int i = 0; i < 3; i++) { lat[i] = foot[i]; st.latched[(3 * leg + i) * B + b] = foot[i]; }
  }
  // ---- gait (own leg) ----
  const double t = t_rob - t_reset;
  int desired, lstate;
  double phase;
  gait_leg(gt, c->contact_thresh, t, contact, desired, lstate, phase);
  // ---- swing update: latch at desired STANCE->SWING (skipped on the first update after reset) ----
  if (ok && (!(flags & 2) || c->conv_first_latch) && desired == RG_LEG_SWING && ((last >> leg) & 1) != RG_LEG_SWING) {
#pragma unroll
    for (int a = 0; a < 3; a++) { lat[a] = foot[a]; st.latched[(3 * leg + a) * B + b] = foot[a]; }
  }
  // the library sin / cos bodies carry a large-argument path that reads a table: at the point where that path joins, the
  // compiler waits for EVERY outstanding memory operation.  They are evaluated here, while nothing but the first block's
  // loads is outstanding -- behind the work-list atomic below they made the wave wait out its ~1.5 us.
  double sr, cr_, sp, cp;
  sincos(rpy[0], &sr, &cr_);
  sincos(rpy[1], &sp, &cp);
  double ph_swing;   // swing-phase shaping of the foot trajectory (used if the leg swings)
  if (phase <= 0.5) ph_swing = 0.8 * sin(phase * M_PI); else ph_swing = 0.8 + (phase - 0.5) * 0.4;
  const unsigned long long des_ballot = __ballot(desired == RG_LEG_STANCE);
  const int desired_bits = (int)((des_ballot >> qbase) & 0xF);   // bit l = leg l desired STANCE (== desired value)
  const int cmask = ok ? desired_bits : 0;   // contact for the MPC = desired STANCE
  const int nc = __builtin_popcount(cmask);
  // with a contact schedule every robot that has a stance leg now goes to the schedule body (rg_qp_sched_kernel.inc), which
  // works on all four legs' blocks and eliminates the (step, leg) pairs not in contact: one work-list "bin" (4) for all of them
  const int bin = c->lookahead ? (nc > 0 ? 4 : 0) : nc;
  // ---- (3) work lists: one slot per robot.  One atomic per wave and list (not per robot): 4096 same-address
  // device-scope atomics took longer than the rest of this kernel.
  // plan 0: list = stance-leg count.  plan 1 (fused QP launch): list = cost class predicted from the robot's
  // solver iterations in the previous tick, most expensive first -- the launch then starts its stragglers
  // first instead of finding a 170-iteration robot in its last round (the iteration count is unknown in
  // advance but strongly correlated from tick to tick).
  // Everything loaded above that the code BEHIND the atomic uses first is pinned as arrived here: once stores and the
  // returning atomic are in flight, the compiler's wait for any older load is a wait for all of them.
#pragma unroll
  for (int a = 0; a < 3; a++) asm volatile("" : : "v"(hip[a]), "v"(lat[a]), "v"(fsum[a]), "v"(fcorr[a]), "v"(ring_old[a]));
  asm volatile("" : : "v"(valid_old), "v"(sched_raw));
  int list = bin, entry = b, wl_leader = lane, wl_rank = 0, wl_base = 0;
  {
    // persistently hard robot (the exact solver took it over, same contact set since): straight to the exact list of its
    // stance-leg count -- ADMM would run to the cap again, and one such robot makes the whole launch wait for it.  Every
    // 16th tick it tries ADMM again (the body clears the mark when it converges).
    const bool direct = c->plan == 1 && bin > 0 && leg == 0 && st.direct_on && hard_prev == cmask + 1 && ((st.tick ^ b) & 15) != 0;
    if (c->plan == 1 && bin > 0 && leg == 0 && !direct) {
      // (a robot whose stance-leg count differs from the previous tick's runs another body, from a cold start: its previous count
      // says nothing -- a two-leg robot with 3 applications of G becomes a four-leg robot with ~65 ADMM iterations, and predicted
      // cheap it was dispatched last: these robots ended the launch, 80-95 us jobs starting at 70-85 us.  They get the
      // population's typical cold-start count instead.)
      const int ws_prev = c->exact12 ? ws_cnt_prev : 0;
      const int itp = (ncs_prev == bin) ? it_prev : (bin >= 3 ? (c->exact12 == 2 ? 30 : 70) : (c->exact12 ? 12 : 65));
      // cost in units of one two-leg ADMM iteration: set-up + sweep ~ 45, wrench-space iteration ~ 1.6
      // (under the exact body itp counts applications of G, ~1.5 us each under load = four ADMM iterations)
      const int cost = (bin >= 3) ? (c->exact12 == 2 ? 45 + 4 * itp : 55 + (itp * 8) / 5) : (c->exact12 ? 45 + 4 * itp : 45 + itp);
      int cls = (RG_COST_CLASSES - 1) - (cost - 45) / 12;
      cls = cls < 0 ? 0 : cls;
      list = 10 + cls;
      // exact body of the QP launch: a robot whose stored working set is close to that body's capacity runs the body with
      // the larger (packed) T straight away -- outgrowing the small one costs the tick a serial re-solve after the launch
      const bool big = bin <= 2 && ncs_prev == bin && ws_prev > RG_EXACT_BIG_WS;
      entry = b | (bin << 24) | (big ? 1 << 28 : 0);
    }
    const int cidx = list >= 10 ? 16 + (list - 10) : list;
    // group the wave's leg-0 lanes by list (ballots only), then ONE atomic instruction in which every group
    // leader adds its group's size; a returning device-scope atomic is ~1.5 us, so they must not be serial
    int cnt = 0;
    unsigned long long todo = __ballot(leg == 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int key = __shfl(list, leader);
      const unsigned long long m = __ballot(leg == 0 && list == key);
      if (leg == 0 && list == key) { wl_leader = leader; wl_rank = __popcll(m & ((1ull << lane) - 1ull)); cnt = __popcll(m); }
      todo &= ~m;
    }
    if (leg == 0 && lane == wl_leader) wl_base = atomicAdd(&st.counts[cidx], cnt);   // (consumed at the end of the kernel)
  }
  // ---- velocity estimator (all four lanes compute it, leg 0 stores it) ----
  double vf[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    double sm = fsum[a], cr = fcorr[a];
    if (rlen >= W) neumaier_add(sm, cr, -ring_old[a]);
    neumaier_add(sm, cr, vw[a]);
    vf[a] = (sm + cr) / (double)((c->conv_window_divide && rlen < W) ? rlen + 1 : W);   // (conv_window_divide: by the samples held while the window fills)
    // (every lane's reads of this robot's filter state were issued in the first block, before leg 0 overwrites it)
    if (leg == 0 && ok) { st.ring[((size_t)a * W + rhead) * B + b] = (float)vw[a]; st.fsum[a * B + b] = sm; st.fcorr[a * B + b] = cr; }
  }
  double vb[3];
  {
    double x = -quat[0], y = -quat[1], z = -quat[2], w = quat[3];
    double tx = 2 * (y * vf[2] - z * vf[1]), ty = 2 * (z * vf[0] - x * vf[2]), tz = 2 * (x * vf[1] - y * vf[0]);
    vb[0] = vf[0] + w * tx + (y * tz - z * ty);
    vb[1] = vf[1] + w * ty + (z * tx - x * tz);
    vb[2] = vf[2] + w * tz + (x * ty - y * tx);
  }
  // ---- swing get_action (own leg) ----
  double ftarget[3] = {0.0, 0.0, 0.0};
  const bool do_swing = ok && !(lstate == RG_LEG_STANCE || lstate == RG_LEG_EARLY_CONTACT);
  if (do_swing) {
    double tw[3] = {-hip[1], hip[0], 0.0};
    double cv[3] = {vb[0], vb[1], 0.0}, dv[3] = {cmd[0], cmd[1], 0.0};
    // (the robot's own body height is loaded here, behind the work-list atomic: only handles with body rows pay that wait)
    const double body_h = c->body ? c->body[(size_t)b * RG_BODY_N + BODY_HEIGHT] : c->body_height;
    double dh[3] = {0.0, 0.0, body_h - c->foot_clearance};
    double target[3], start[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      double hv = cv[a] + rate[2] * tw[a];
      double thv = dv[a] + cmd[2] * tw[a];
      target[a] = (hv * gt.stance / 2 - c->swing_kp[a] * (thv - hv)) - dh[a] + (a < 2 ? hip[a] : 0.0);
      start[a] = lat[a];
    }
    const double ph = ph_swing;
    double fp[3];
    fp[0] = (1 - ph) * start[0] + ph * target[0];
    fp[1] = (1 - ph) * start[1] + ph * target[1];
    {
      double mid = fmax(target[2], start[2]) + c->max_clearance;
      double d1 = mid - start[2], d2 = target[2] - start[2], d3 = 0.25 - 0.5;
      double ca = (d1 - d2 * 0.5) / d3, cb = (d2 * 0.25 - d1) / d3;
      fp[2] = ca * ph * ph + cb * ph + start[2];
    }
    // the IK of this target runs on the swing IK lanes at the end of the QP launch (swing_ik_lane)
    const size_t n4 = (size_t)4 * B;
#pragma unroll
    for (int j = 0; j < 3; j++) { st.ik_in[j * n4 + gid] = fp[j]; st.ik_in[(3 + j) * n4 + gid] = q3[j]; ftarget[j] = fp[j]; }
  }
  st.ik_flag[gid] = do_swing ? 1 : 0;
  const int swing_bits = (int)((__ballot(do_swing) >> qbase) & 0xF);
  int valid = valid_old;
#pragma unroll
  for (int l = 0; l < 4; l++) if ((swing_bits >> l) & 1) valid |= 7 << (3 * l);
  int emit = 0;
#pragma unroll
  for (int j = 0; j < 12; j++) if (((valid >> j) & 1) && !((desired_bits >> (j / 3)) & 1)) emit |= 1 << j;
  if (!ok) emit = 0;
  // ---- stance record ----
  // contact schedule: bit k = this leg in contact at horizon step k.  Upstream holds the current contacts over the
  // horizon (all bits = the contact flag).  With the contact_lookahead extension step 0 is still the controller's own
  // contact decision and steps 1..H-1 come from the caller's schedule when one is passed, else from the open-loop gait
  // evaluated at t + k dt_plan.
  const int hmask = (1 << c->H) - 1;
  int sched = ((cmask >> leg) & 1) ? hmask : 0;
  if (c->lookahead) {
    sched &= 1;
    if (in.contact_sched) sched |= sched_raw & (hmask - 1);
    else for (int k = 1; k < c->H; k++) sched |= (gait_desired_at(gt, c->contact_thresh, c->dt, t, k) == RG_LEG_STANCE) << k;
  }
  // own foot -> world-aligned frame with Rx(roll) Ry(pitch)   (yaw zeroed)
  // (conv_feet_rotation = 1: Ry(pitch) Rx(roll), the order the inertia below is rotated with)
  double fw[3];
  if (c->conv_feet_rotation) {
    const double y1 = cr_ * foot[1] - sr * foot[2], z1 = sr * foot[1] + cr_ * foot[2];
    fw[0] = cp * foot[0] + sp * z1; fw[1] = y1; fw[2] = -sp * foot[0] + cp * z1;
  } else {
    fw[0] = cp * foot[0] + sp * foot[2];
    fw[1] = sr * sp * foot[0] + cr_ * foot[1] - sr * cp * foot[2];
    fw[2] = -cr_ * sp * foot[0] + sr * foot[1] + cr_ * cp * foot[2];
  }
  // CoM height from the contact feet: |mean z| (conv_com_height = 1: mean |z|)
  double hz = ((cmask >> leg) & 1) ? (c->conv_com_height ? fabs(fw[2]) : fw[2]) : 0.0;
  hz += __shfl_xor(hz, 1);
  hz += __shfl_xor(hz, 2);
  double *rec = st.rec + (size_t)b * RG_REC_N;
#pragma unroll
  for (int i = 0; i < 3; i++) rec[REC_FEETW + 3 * leg + i] = fw[i];
#pragma unroll
  for (int i = 0; i < 9; i++) rec[REC_JAC + 9 * leg + i] = jac[i];
  rec[REC_SCHED + leg] = (double)sched;
  if (c->body_rec) {   // the body block of the record (REC_BODY), for the MU4 QP instantiations: two doubles per leg lane
    static_assert(RG_BODY_REC == 8 && REC_BODY + RG_BODY_REC <= REC_EMIT, "four lanes copy two doubles each into the record's body block");
    const double *br = c->body ? c->body + (size_t)b * RG_BODY_N : c->body_cfg;
    rec[REC_BODY + 2 * leg] = br[2 * leg]; rec[REC_BODY + 2 * leg + 1] = br[2 * leg + 1];
  }
  if (leg == 0) {
    rec[REC_ROLL] = rpy[0]; rec[REC_PITCH] = rpy[1];
    rec[REC_COMZ] = nc > 0 ? fabs(hz / nc) : 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) { rec[REC_OMEGA + i] = rate[i]; rec[REC_VBODY + i] = vb[i]; rec[REC_CMD + i] = cmd[i]; }
    // body rotation for the inertia: Ry(pitch) Rx(roll)
    double Rb[9] = {cp, sp * sr, sp * cr_, 0, cr_, -sr, -sp, cp * sr, cp * cr_};
    double T1[9], Rt[9], Iw[9], Ii[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Rt[3 * i + j] = Rb[3 * j + i];
    // body-frame inverse inertia: the robot's row (loaded here, by the leg-0 lanes only), or the config's (scalar loads)
    if (c->body) {
#pragma unroll
      for (int i = 0; i < 9; i++) Ii[i] = c->body[(size_t)b * RG_BODY_N + BODY_IINV + i];
    } else {
#pragma unroll
      for (int i = 0; i < 9; i++) Ii[i] = c->Iinv[i];
    }
    m3mul(Rb, Ii, T1);
    m3mul(T1, Rt, Iw);
#pragma unroll
    for (int i = 0; i < 9; i++) rec[REC_IWINV + i] = Iw[i];
    rec[REC_INVCP] = 1.0 / cp;
    rec[REC_TANP] = sp / cp;
    rec[REC_EMIT] = (double)emit;
    rec[REC_CONTACT] = (double)(c->lookahead ? 15 : cmask);
    // per-robot persistent scalars
    if (ok) {
      st.ring_head[b] = (rhead + 1) % W;
      if (rlen < W) st.ring_len[b] = rlen + 1;
      st.last_desired[b] = desired_bits;
      st.flags[b] = 0;
      st.swing_valid[b] = valid;
    }
    if (nc == 0) st.iters[b] = 0;
    if (out.v_body)
#pragma unroll
      for (int i = 0; i < 3; i++) out.v_body[b * 3 + i] = (float)vb[i];
  }
  // ---- optional outputs (per leg) ----
  if (out.leg_state) out.leg_state[b * 4 + leg] = lstate;
  if (out.desired_state) out.desired_state[b * 4 + leg] = desired;
  if (out.phase) out.phase[b * 4 + leg] = (float)phase;
  if (out.foot_target)
#pragma unroll
    for (int i = 0; i < 3; i++) out.foot_target[b * 12 + 3 * leg + i] = (float)ftarget[i];
  if (nc == 0) {
    // no stance leg: forces are zero, the action row is complete here
#pragma unroll
    for (int jj = 0; jj < 3; jj++) {
      const int j = 3 * leg + jj;
      float *a = out.action + (size_t)b * 60 + 5 * j;
      if ((emit >> j) & 1) { a[1] = (float)c->kp[j]; a[2] = 0.f; a[3] = (float)c->kd[j]; a[4] = 0.f; }   // a[0] = q*: swing_ik_lane
      else { a[0] = 0.f; a[1] = 0.f; a[2] = 0.f; a[3] = 0.f; a[4] = 0.f; }
      if (out.grf) out.grf[b * 12 + j] = 0.f;
      if (out.tau_stance) out.tau_stance[b * 12 + j] = 0.f;
    }
  }
  // ---- the robot's work-list entry: the slot requested in (3) ----
  {
    const int slot = __shfl(wl_base, wl_leader) + wl_rank;
    if (leg == 0) { st.bins[(size_t)list * B + slot] = entry; st.ncs[b] = bin; }
  }
}
