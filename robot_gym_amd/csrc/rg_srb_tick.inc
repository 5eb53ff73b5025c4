// rg_srb_tick.inc -- the body of a simulator tick (include/rg_srb.h), defined once for the four step kernels: rg_srb.hip (the
// plane), rg_srb_terrain.hip (the heightfield), rg_srb_contact.hip (measured contact) and the fourth unit, the one with its own
// force rule.  Included after `#pragma clang fp contract(off)`, rg_mpc_dev.h and rg_srb_dev.inc, inside the including file's
// anonymous namespace.  Plain functions over the kernels' local arrays, inlined into each kernel: a kernel keeps its signature,
// step 1 (the feet), its force rule, its ground queries and its own outputs, and its sub-step loop is quat_rot, rot, its rule,
// tick_wrench, tick_body, tick_quat.  The fourth unit's kernel types tick_wrench and tick_body out in its loop, where the calls
// measured slower than its former text (profiles/srb_tick_identity.txt): a change to either is made there too.
//
// Layout: lane = (robot, leg), four lanes per robot, 16 robots per wave, float64 throughout, no LDS.  Two functions here work
// across lanes: sum4 (inside tick_wrench) and tick_bad.  Their callers keep every lane of a wave with them: every lane is
// guarded by b < B and by the robot's status at its stores only (tick_store), lanes past the batch compute on the last robot and
// store nothing, and no branch or return goes around a cross-lane operation.

// sum over the four lanes of a robot: (x_0 + x_1) + (x_2 + x_3) in every lane, so the four lanes hold bit-identical sums and
// integrate the 13 body values redundantly -- the sub-step loop needs no broadcast
__device__ __forceinline__ double sum4(double x) {
  x = x + __shfl_xor(x, 1);
  return x + __shfl_xor(x, 2);
}

// the rows of state [RG_SRB_STATE_ROWS][B] a lane works on -> whether the robot is running (status 0)
__device__ __forceinline__ bool tick_load_state(const double *state, size_t sB, int b, int leg, double *p, double *qt, double *v, double *w,
                                                double *foot, double *q, double &stance, double &steps) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    p[i] = state[(RG_SRB_ROW_P + i) * sB + b];
    v[i] = state[(RG_SRB_ROW_V + i) * sB + b];
    w[i] = state[(RG_SRB_ROW_W + i) * sB + b];
    foot[i] = state[(RG_SRB_ROW_FOOT + 3 * leg + i) * sB + b];
    q[i] = state[(RG_SRB_ROW_Q + 3 * leg + i) * sB + b];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) qt[i] = state[(RG_SRB_ROW_QUAT + i) * sB + b];
  stance = state[(RG_SRB_ROW_STANCE + leg) * sB + b];
  steps = state[RG_SRB_ROW_STEPS * sB + b];
  return state[RG_SRB_ROW_STATUS * sB + b] == 0.0;
}

// the robot's rows of body [kSrbBodyRows][B]: the inertia and its inverse -> the mass
__device__ __forceinline__ double tick_load_body(const double *body, size_t sB, int b, double *I, double *Iinv) {
#pragma unroll
  for (int i = 0; i < 9; i++) { I[i] = body[(1 + i) * sB + b]; Iinv[i] = body[(10 + i) * sB + b]; }
  return body[b];
}

// the external wrench ext [6][B], or zero without one
__device__ __forceinline__ void tick_load_ext(const double *ext, size_t sB, int b, double *eF, double *eT) {
#pragma unroll
  for (int i = 0; i < 3; i++) { eF[i] = 0.0; eT[i] = 0.0; }
  if (ext) {
#pragma unroll
    for (int i = 0; i < 3; i++) { eF[i] = ext[i * sB + b]; eT[i] = ext[(3 + i) * sB + b]; }
  }
}

// the wrench of a sub-step on the body: the lane's foot force f (world) at its lever arm, summed over the robot's four lanes, plus
// the weight wz and the push
__device__ __forceinline__ void tick_wrench(const double *f, const double *foot, const double *p, const double *eF, const double *eT,
                                            double wz, double *F, double *T) {
  double r[3], tq[3];
  r[0] = foot[0] - p[0]; r[1] = foot[1] - p[1]; r[2] = foot[2] - p[2];
  tq[0] = r[1] * f[2] - r[2] * f[1];
  tq[1] = r[2] * f[0] - r[0] * f[2];
  tq[2] = r[0] * f[1] - r[1] * f[0];
#pragma unroll
  for (int i = 0; i < 3; i++) { F[i] = sum4(f[i]); T[i] = sum4(tq[i]); }
  F[0] = F[0] + eF[0]; F[1] = F[1] + eF[1]; F[2] = F[2] + wz + eF[2];
  T[0] = T[0] + eT[0]; T[1] = T[1] + eT[1]; T[2] = T[2] + eT[2];
}

// Euler's equation in the body frame, then w, v and p by semi-implicit Euler
__device__ __forceinline__ void tick_body(const double *R, const double *I, const double *Iinv, double mass, double dt, const double *F,
                                          const double *T, double *w, double *v, double *p) {
  double tb[3], wb[3], Iw[3], rhs[3], ab[3], aw[3];
  rot_t(R, T, tb);
  rot_t(R, w, wb);
  rot(I, wb, Iw);
  rhs[0] = tb[0] - (wb[1] * Iw[2] - wb[2] * Iw[1]);
  rhs[1] = tb[1] - (wb[2] * Iw[0] - wb[0] * Iw[2]);
  rhs[2] = tb[2] - (wb[0] * Iw[1] - wb[1] * Iw[0]);
  rot(Iinv, rhs, ab);
  rot(R, ab, aw);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    w[i] = w[i] + dt * aw[i];
    v[i] = v[i] + dt * F[i] / mass;
    p[i] = p[i] + dt * v[i];
  }
}

// qt <- normalised (qt + dt / 2 * (w, 0) qt)
__device__ __forceinline__ void tick_quat(double dt, const double *w, double *qt) {
  const double ax = 0.5 * dt * w[0], ay = 0.5 * dt * w[1], az = 0.5 * dt * w[2];
  const double dx = ax * qt[3] + ay * qt[2] - az * qt[1];
  const double dy = ay * qt[3] + az * qt[0] - ax * qt[2];
  const double dz = az * qt[3] + ax * qt[1] - ay * qt[0];
  const double dw = -(ax * qt[0]) - ay * qt[1] - az * qt[2];
  qt[0] = qt[0] + dx; qt[1] = qt[1] + dy; qt[2] = qt[2] + dz; qt[3] = qt[3] + dw;
  const double nrm = sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3]);
  qt[0] = qt[0] / nrm; qt[1] = qt[1] / nrm; qt[2] = qt[2] / nrm; qt[3] = qt[3] / nrm;
}

// non-zero in all four lanes of a robot when any value of its new state is not finite (the feet differ from lane to lane)
__device__ __forceinline__ int tick_bad(const double *p, const double *qt, const double *v, const double *w, const double *foot) {
  int bad = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) bad |= !isfinite(p[i]) || !isfinite(v[i]) || !isfinite(w[i]) || !isfinite(foot[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) bad |= !isfinite(qt[i]);
  bad |= __shfl_xor(bad, 1);
  bad |= __shfl_xor(bad, 2);
  return bad;
}

// Step 3 of rg_srb.h and the stores: the status of a running robot (fallen: a state that is not finite, the body `clearance`
// above the ground under fall_z, or tilted past cos_tilt), and the new state unless it is not finite -> whether the state was
// stored.  A frozen robot and a lane past the batch store nothing.
__device__ __forceinline__ bool tick_store(double *state, const SrbCfg &c, int b, int leg, bool live, int bad, double clearance,
                                           const double *p, const double *qt, const double *v, const double *w, const double *foot,
                                           double stance, double steps) {
  const size_t sB = (size_t)c.B;
  const bool fallen = bad || clearance < c.fall_z || (1 - 2 * (qt[0] * qt[0] + qt[1] * qt[1])) < c.cos_tilt;
  if (live && leg == 0) state[RG_SRB_ROW_STATUS * sB + b] = fallen ? 1.0 : 0.0;
  const bool store = live && !bad;
  if (store) {
#pragma unroll
    for (int i = 0; i < 3; i++) state[(RG_SRB_ROW_FOOT + 3 * leg + i) * sB + b] = foot[i];
    state[(RG_SRB_ROW_STANCE + leg) * sB + b] = stance;
    if (leg == 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        state[(RG_SRB_ROW_P + i) * sB + b] = p[i];
        state[(RG_SRB_ROW_V + i) * sB + b] = v[i];
        state[(RG_SRB_ROW_W + i) * sB + b] = w[i];
      }
#pragma unroll
      for (int i = 0; i < 4; i++) state[(RG_SRB_ROW_QUAT + i) * sB + b] = qt[i];
      state[RG_SRB_ROW_STEPS * sB + b] = steps;
    }
  }
  return store;
}
