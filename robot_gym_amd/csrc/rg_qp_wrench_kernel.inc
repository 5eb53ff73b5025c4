// rg_qp_wrench_kernel.inc -- ADMM QP body for 3 and 4 stance legs (contacts held over the horizon), solved in wrench coordinates.
// (Per-step contact schedules use the generalisation in rg_qp_sched_kernel.inc, which also reuses WrenchLane and
// wrench_admm_vote below; the tile primitives are in rg_qp_tile.inc.)
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// ------------------------------------------------------------------------------------
// With nc >= 3 stance legs the 3 nc force components of one horizon step act on the single rigid
// body only through a 6-vector (angular and linear acceleration), so the condensed Hessian
//     P = alpha I + (I_H (x) C)' K (I_H (x) C),      C = [ Iw^-1 [r_j]x ; I3 ]   (6 x 3 nc)
// has a 6H-dimensional range and the rest of R^(3 nc H) sees only alpha.  Factor C C' = L L' and put
// Ch = L^-1 C (orthonormal rows), K' = 2 (N (x) L' A_U L + S (x) L' A_V L) (6H x 6H).  Then, exactly,
//     (P + rho I)^-1 v = v / a + Ch~' [ (a I + K')^-1 - I / a ] Ch~ v,        a = alpha + rho,
// so the matrix to invert is 60 x 60 (H = 10) for three and four legs alike -- the size of the
// two-leg problem -- instead of 90 x 90 / 120 x 120: 3.4x / 8x less elimination work, a 64-lane
// workgroup (one wave) per robot instead of 256 lanes, and no workgroup barrier in the ADMM loop.
// The ADMM iterates are the same as the force-space kernel's up to rounding.
//
// Lane roles inside the LC x LC lane grid (LC = 8 for H = 10):
//   tile lane (lr, lc): the 8 x 8 register tile of -(a I + K')^-1 (sweep-inverse, as rg_qp_tile_kernel)
//   owner lane of wrench row io: finishes (T' w)_io after the cross-lane reduce-scatter
//   block lane 4 k + j: horizon step k, stance-leg slot j: the 3-vector z, y of that foot force, its
//     6 x 3 block of Ch, and the friction-pyramid projection -- all in registers, no gather needed.
// Per iteration: 18 FMAs + quad reduce (DPP) -> LDS -> 64 FMAs + reduce-scatter (DPP) -> LDS -> 18 FMAs
// + projection.
// ------------------------------------------------------------------------------------

// Roles of one lane in the ADMM iteration of the wrench-space bodies (see the header comment), derived from its index in
// the workgroup.  The bodies derive them AFTER the sweep, from a fresh opaque lane index (wg_lane), and once more in the
// epilogue: computed once at the top they stay live across the sweep, where every VGPR is taken, and were spilled (eight
// scratch stores and reloads per robot and stage).
template <int H, int LG, int T = 8>
struct WrenchLane {
  static constexpr int TS = TileShape<T>::TS, LC = 1 << LG, NW = 6 * H;
  int io, iov_pad;          // owner lane of wrench row io (after the reduce-scatter); its slot in the padded mat-vec input
  bool own_real;
  int bk, bj;               // block lane: horizon step bk, stance-leg slot bj
  bool quad_real;
  int b0, b1, rA, rB, padA, padB, ubase0, ubase1;
  __device__ __forceinline__ explicit WrenchLane(const int tid) {
    const int lr = tid >> LG, lc = tid & (LC - 1);
    const int own_a = TileShape<T>::own_a(lc);
    io = lr * T + own_a;
    own_real = lc < T && io < NW;
    iov_pad = lr * TS + own_a;
    bk = tid >> 2; bj = tid & 3;
    quad_real = bk < H;
    // after the quad reduce-scatter this lane holds wrench components {3 b0, 3 b0 + 1, 3 b0 + 2} of step bk and publishes
    // one or two of them
    b0 = tid & 1; b1 = (tid >> 1) & 1;
    rA = 6 * bk + 3 * b0 + (b1 ? 2 : 0); rB = 6 * bk + 3 * b0 + 1;
    padA = TileShape<T>::pad(rA); padB = TileShape<T>::pad(rB);
    ubase0 = 6 * bk + 3 * b0; ubase1 = 6 * bk + 3 * (1 - b0);   // u6 rows 0..2 and 3..5 in this lane's order
  }
};

// The convergence vote of the wrench-space bodies (qp_wrench_robot, qp_sched_robot), every admm_check iterations; the rules
// are those of qp_tile_robot (explained there), on the block lane's 3-vectors.  zck / yck: forces and multipliers at the last
// vote, yst / dyq: their movement over the window before ([axis][lane] in LDS: touched once per window, not six more VGPRs of a
// loop at the register limit), sum3: the workgroup sums' slots, [12] the largest extrapolation gain of the stage, [13] the
// remaining-distance factor of the last vote.  `hist`: valid windows of displacement history (0 at the stage start and right
// after a jump).  Returns true when nobody moves any more (the caller leaves the loop); otherwise (z, y) may have been
// extrapolated along the dominant mode (extrapolation_gain).
template <int NT>
__device__ __forceinline__ bool wrench_admm_vote(const DevCfg *__restrict__ c, const int tid, const bool active, double (&zb)[3], double (&yb)[3], double *zck, double *yst,
                                                 double *yck, double *dyq, double *sum3, const double pres, const double atol, const double etol, const double ptol,
                                                 const int it, int &hist) {
  // movement over this window, and the geometric estimate of the distance still to go
  double mmax = 0.0, emax = 0.0, d11 = 0.0, d00 = 0.0, d10 = 0.0;   // d..: dot products of the rate / extrapolation test (lanes without a block hold zeros)
  const double gst = sum3[12], rfac = gst > 0.0 ? fmax(gst, sum3[13]) : 0.0;   // the extra distance estimates apply to robots that have jumped in this stage
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double dz = zb[d] - zck[d * NT + tid], dzp = yst[d * NT + tid];
    const double dy = yb[d] - yck[d * NT + tid], dyp = dyq[d * NT + tid];
    const double m = fabs(dz), mp = fabs(dzp);
    const double est = fmax((mp > m && mp < 1.0e300) ? m * m * fast_rcp(mp - m) : 0.0, m * rfac);   // first window, or not shrinking: no per-entry estimate
    yst[d * NT + tid] = dz; dyq[d * NT + tid] = dy;
    zck[d * NT + tid] = zb[d]; yck[d * NT + tid] = yb[d];
    mmax = fmax(mmax, m); emax = fmax(emax, est);
    if (gst > 0.0 && mp > 4.0 * atol) mmax = INFINITY;   // jumped robots pass only with two consecutive quiet windows
    d11 = fma(dz, dz, fma(dy, dy, d11));
    if (hist >= 1) { d00 = fma(dzp, dzp, fma(dyp, dyp, d00)); d10 = fma(dz, dzp, fma(dy, dyp, d10)); }
  }
  const int moving = (active && (mmax > atol || emax > etol || pres > ptol)) || (gst > 0.0 && hist <= 0);
  const bool rate_now = hist >= 1 && c->accel_from > 0 && it + 1 >= c->accel_from;   // dominant-mode rate / extrapolation of (z, y)
  if (rate_now) sum3_publish<NT>(d11, d00, d10, sum3);
  if (!workgroup_any<NT>(moving)) return true;
  if (rate_now) {
    sum3_collect<NT>(d11, d00, d10, sum3);
    const double g = extrapolation_gain(c->accel_k, d11, d00, d10);
    const bool jump = __builtin_amdgcn_readfirstlane(g > 0.0);   // same g in every lane: keep the branch (and hist) scalar
    if (tid == 0) { sum3[13] = jump ? 0.0 : remaining_distance_factor(c->accel_k, d11, d00, d10); if (jump) sum3[12] = fmax(gst, g); }
    if (jump) {
#pragma unroll
      for (int d = 0; d < 3; d++) {   // the window's displacements were just stored: yst = dz, dyq = dy
        zb[d] = fma(g, yst[d * NT + tid], zb[d]); yb[d] = fma(g, dyq[d * NT + tid], yb[d]);
        zck[d * NT + tid] = zb[d]; yck[d * NT + tid] = yb[d];
      }
      hist = -1;
    }
  }
  hist++;
  return false;
}

// The vote as qp_wrench_robot takes it on the one-wave grid with uniform friction: the same rules, stores, result and extrapolation
// as wrench_admm_vote, in another order.  The distance estimates and the primal residual -- three reciprocals behind exec-masked
// branches, and |x - z| -- can only turn a vote that nobody's movement has decided already, so they are evaluated behind a first
// ballot on the movement alone: a robot that still iterates, nine votes of ten, never gets there.  xr: the unprojected forces x
// of this iteration (the primal residual is |xr - zb|).  A function of its own: the schedule bodies' kernels, at the register
// limit with pinned scratch frames, compile differently when wrench_admm_vote's text changes.
__device__ __forceinline__ bool wrench_admm_vote_late(const DevCfg *__restrict__ c, const int tid, const bool active, double (&zb)[3], double (&yb)[3], double *zck, double *yst,
                                                      double *yck, double *dyq, double *sum3, const double (&xr)[3], const double atol, const double etol, const double ptol,
                                                      const int it, int &hist) {
  constexpr int NT = 64;
  double mmax = 0.0, d11 = 0.0, d00 = 0.0, d10 = 0.0, mpk[3];   // mpk: the window before's |movement|, for the estimates
  const double gst = sum3[12];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double dz = zb[d] - zck[d * NT + tid], dzp = yst[d * NT + tid];
    const double dy = yb[d] - yck[d * NT + tid], dyp = dyq[d * NT + tid];
    const double m = fabs(dz), mp = fabs(dzp);
    mpk[d] = mp;
    yst[d * NT + tid] = dz; dyq[d * NT + tid] = dy;
    zck[d * NT + tid] = zb[d]; yck[d * NT + tid] = yb[d];
    mmax = fmax(mmax, m);
    if (gst > 0.0 && mp > 4.0 * atol) mmax = INFINITY;   // jumped robots pass only with two consecutive quiet windows
    d11 = fma(dz, dz, fma(dy, dy, d11));
    if (hist >= 1) { d00 = fma(dzp, dzp, fma(dyp, dyp, d00)); d10 = fma(dz, dzp, fma(dy, dyp, d10)); }
  }
  if (__ballot((active && mmax > atol) || (gst > 0.0 && hist <= 0)) == 0ull) {   // nobody's movement keeps the robot going: the estimates and |x - z| decide
    const double rfac = gst > 0.0 ? fmax(gst, sum3[13]) : 0.0;   // the extra distance estimates apply to robots that have jumped in this stage
    double emax = 0.0, pr = 0.0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const double m = fabs(yst[d * NT + tid]), mp = mpk[d];   // (yst: this window's movement, stored above)
      emax = fmax(emax, fmax((mp > m && mp < 1.0e300) ? m * m * fast_rcp(mp - m) : 0.0, m * rfac));   // first window, or not shrinking: no per-entry estimate
      pr = fmax(pr, fabs(xr[d] - zb[d]));
    }
    if (__ballot(active && (emax > etol || pr > ptol)) == 0ull) return true;
  }
  if (hist >= 1 && c->accel_from > 0 && it + 1 >= c->accel_from) {   // dominant-mode rate / extrapolation of (z, y)
    sum3_collect<NT>(d11, d00, d10, sum3);
    const double g = extrapolation_gain(c->accel_k, d11, d00, d10);
    const bool jump = __builtin_amdgcn_readfirstlane(g > 0.0);   // same g in every lane: keep the branch (and hist) scalar
    if (tid == 0) { sum3[13] = jump ? 0.0 : remaining_distance_factor(c->accel_k, d11, d00, d10); if (jump) sum3[12] = fmax(gst, g); }
    if (jump) {
#pragma unroll
      for (int d = 0; d < 3; d++) {
        zb[d] = fma(g, yst[d * NT + tid], zb[d]); yb[d] = fma(g, dyq[d * NT + tid], yb[d]);
        zck[d * NT + tid] = zb[d]; yck[d * NT + tid] = yb[d];
      }
      hist = -1;
    }
  }
  hist++;
  return false;
}

// LDS of qp_wrench_robot (doubles).  What lives through the stages comes first; the rest is set-up data and per-stage state, and
// on the one-wave grid -- where the matrix is swept with every 6 x 6 block held once (rg_qp_sym6.inc) -- the staging area of the
// move into the 8 x 8 tiles covers all of it (nothing there is live at that moment: the iterate of a robot that goes into its
// second stage stays in registers across the sweep).
template <int NC, int H, int LG, int T>
struct WrenchLds {
  static_assert(H == 10 && ((LG == 3 && T == 8) || (LG == 4 && T == 4)), "the wrench-space ADMM body runs at horizon 10, on 8 x 8 lanes with 8 x 8 tiles or 16 x 16 lanes with 4 x 4 tiles");
  static constexpr int m3 = 3 * NC, NW = 6 * H, LC = 1 << LG, NP = T * LC, NT = LC * LC, TS = TileShape<T>::TS, NPAD = TS * LC, NPB = NPAD + 2;
  static constexpr bool SYM6 = T == 8;   // the one-wave grid
  static constexpr int rec = 0;                   // RG_REC_N
  static constexpr int grf = rec + RG_REC_N;      // 24
  static constexpr int Ch = grf + 24;             // 6 * m3  L^-1 C
  static constexpr int AU = Ch + 6 * m3;          // 36  L' A_U L
  static constexpr int AV = AU + 36;              // 36  L' A_V L
  static constexpr int qh = AV + 36;              // NW  L' q_w
  static constexpr int sum3 = qh + NW;            // 16  sum3_publish / _collect slots [0..11], largest extrapolation gain of the stage [12], remaining_distance_factor of the last vote [13]
  static constexpr int stage = sum3 + 16;         // ---- from here on: dead while the swept matrix is moved into the tiles ----
  static constexpr int pbuf = stage;              // the sweep's ping-pong pivot buffers
  static constexpr int PBUF = SYM6 ? 2 * Sym6<10>::PB : 2 * NPB;
  static constexpr int vv = pbuf + PBUF;          // NPAD  mat-vec input w (padded groups)
  static constexpr int uv = vv + NPAD;            // NP    mat-vec output u
  static constexpr int Cm = uv + NP;              // 6 * m3  C
  static constexpr int Qm = Cm + 6 * m3;          // 36  C C'
  static constexpr int Lm = Qm + 36;              // 36  L (lower)
  static constexpr int qw = Lm + 36;              // NW
  static constexpr int zck = qw + NW;             // 3 * NT  forces at the previous convergence vote
  static constexpr int yst = zck + 3 * NT;        // 3 * NT  movement of the forces over the window before
  static constexpr int yck = yst + 3 * NT;        // 3 * NT  multipliers at the previous convergence vote
  static constexpr int dyq = yck + 3 * NT;        // 3 * NT  their movement over the window before (extrapolation test)
  static constexpr int end = dyq + 3 * NT;
  static constexpr int total = (SYM6 && stage + Sym6<10>::STG > end) ? stage + Sym6<10>::STG : end;
  // what stays live through sym6_to_tile8 ends where the staging area starts, and the staging area fits the layout
  static_assert(!SYM6 || (rec + RG_REC_N <= stage && grf + 24 <= stage && Ch + 6 * m3 <= stage && AU + 36 <= stage && AV + 36 <= stage &&
                          qh + NW <= stage && sum3 + 16 <= stage), "sym6_to_tile8 stages over live LDS");
  static_assert(!SYM6 || stage + Sym6<10>::STG <= total, "the staging area of sym6_to_tile8 fits the layout");
};

// Lane grids (LG, T): (3, 8) one wave (horizon 10), (4, 4) 256 lanes with 4 x 4 tiles (horizon 10, small batches: a quarter of
// the FMAs per lane in the sweep and in the iteration's mat-vec, workgroup barriers where the one-wave body has fences).
template <int NC, int H, int LG, int T = 8, bool MU4 = false>
__device__ __forceinline__ void qp_wrench_robot(const DevCfg *__restrict__ c, const DevState &st, const DevOut &out, const int B, const int b,
                                                const double *tabN, const double *tabS, double *lds) {
  constexpr int m3 = 3 * NC;
  constexpr int NW = 6 * H;          // wrench-space variables
  constexpr int LC = 1 << LG, NP = T * LC, NT = LC * LC;
  static_assert(NP >= NW && 4 * H <= NT && NC >= 3, "lane grid must cover the wrench problem and the (step, leg) blocks");
  // opaque copy: the lane-role integers below are recomputed per robot instead of being hoisted out of the
  // caller's work loop for all bodies at once and spilled (43 scratch stores in the fused kernel's preamble)
  const int tid = wg_lane<NT>();
  using LY = WrenchLds<NC, H, LG, T>;
  constexpr bool SYM6 = LY::SYM6;
  double *rec = lds + LY::rec, *grf = lds + LY::grf, *Ch = lds + LY::Ch, *AU = lds + LY::AU, *AV = lds + LY::AV, *qh = lds + LY::qh, *sum3 = lds + LY::sum3;
  double *pbuf = lds + LY::pbuf, *vv = lds + LY::vv, *uv = lds + LY::uv, *Cm = lds + LY::Cm, *Qm = lds + LY::Qm, *Lm = lds + LY::Lm, *qw = lds + LY::qw;
  double *zck = lds + LY::zck, *yst = lds + LY::yst, *yck = lds + LY::yck, *dyq = lds + LY::dyq;
  // first-stage rho of this body: admm_rho x admm_rho34_scale (the wrench-space iteration converges in fewer iterations at a
  // lower rho than the force-space one, at every percentile of the population); second ADMM stage: c->rho2 (stage loop below)
  double rho = c->rho * c->rho34_scale;
  const double relax = c->relax, dt = c->dt;
  double lo = c->fz_min, hi = c->fz_max;   // (MU4: the robot's, once its record is in LDS)

  {
    __syncthreads();
    for (int e = tid; e < RG_REC_N; e += NT) rec[e] = st.rec[(size_t)b * RG_REC_N + e];
    if (tid < 24) grf[tid] = 0.0;
    if (tid >= NW && tid < NP) vv[TileShape<T>::pad(tid)] = 0.0;   // padding of the mat-vec input: never written again, must not hold NaN bits
    __syncthreads();
    const int cmask = (int)rec[REC_CONTACT];
    if constexpr (MU4) { lo = body_val<MU4>(c, rec, BODY_FZ_MIN); hi = body_val<MU4>(c, rec, BODY_FZ_MAX); }
    if (tid < m3) {
      const int l = nth_leg(cmask, tid / 3), d = tid % 3;
      const double *rr = &rec[REC_FEETW + 3 * l];
      const double s0 = (d == 0) ? 0.0 : (d == 1 ? -rr[2] : rr[1]);
      const double s1 = (d == 0) ? rr[2] : (d == 1 ? 0.0 : -rr[0]);
      const double s2 = (d == 0) ? -rr[1] : (d == 1 ? rr[0] : 0.0);
      const double *Iw = &rec[REC_IWINV];
      Cm[tid] = Iw[0] * s0 + Iw[1] * s1 + Iw[2] * s2;
      Cm[m3 + tid] = Iw[3] * s0 + Iw[4] * s1 + Iw[5] * s2;
      Cm[2 * m3 + tid] = Iw[6] * s0 + Iw[7] * s1 + Iw[8] * s2;
      Cm[3 * m3 + tid] = (d == 0) ? 1.0 : 0.0;
      Cm[4 * m3 + tid] = (d == 1) ? 1.0 : 0.0;
      Cm[5 * m3 + tid] = (d == 2) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < 36) {
      const int i = tid / 6, j = tid % 6;
      double s = 0.0;
#pragma unroll
      for (int e = 0; e < m3; e++) s = fma(Cm[i * m3 + e], Cm[j * m3 + e], s);
      Qm[tid] = s;
    }
    __syncthreads();
    // Cholesky C C' = L L' in registers, redundantly on every lane (static indices only)
    double L[6][6], Li[6];
    bool degenerate = false;
    {
      double Q[6][6];
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) Q[i][j] = Qm[i * 6 + j];
#pragma unroll
      for (int j = 0; j < 6; j++) {
        double s = Q[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s = fma(-L[j][k], L[j][k], s);
        if (!(s > 1e-12 * Q[j][j])) { degenerate = true; s = 1.0; }   // (near-)collinear feet: rank C < 6
        const double d = sqrt(s);
        L[j][j] = d;
        Li[j] = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
          double t = Q[i][j];
#pragma unroll
          for (int k = 0; k < j; k++) t = fma(-L[i][k], L[j][k], t);
          L[i][j] = t * Li[j];
        }
      }
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) Lm[i * 6 + j] = (j <= i) ? L[i][j] : 0.0;
    }
    if (tid < m3) {   // column tid of Ch = L^-1 C
      double y[6];
#pragma unroll
      for (int r = 0; r < 6; r++) {
        double t = Cm[r * m3 + tid];
#pragma unroll
        for (int k = 0; k < r; k++) t = fma(-L[r][k], y[k], t);
        y[r] = t * Li[r];
        Ch[r * m3 + tid] = y[r];
      }
    }
    // q_w(a) = 2 sum_{k >= a} [ dt g1(k) + (k - a + 1/2) dt^2 R6' g2(k) ]   (the force-space q is C' q_w)
    // g1 and R6' g2 are polynomials in the look-ahead time kd = (k + 1) dt: g1 = p0 + p1 kd, g2 = r0 + r1 kd + r2 kd^2.
    // The coefficients are set up once per lane; the k loop is then arithmetic on registers (it used to re-read
    // the record from LDS and branch on the component every step: 8 us of an alone-on-the-CU robot's 74).
    for (int e = tid; e < NW; e += NT) {
      const int a = e / 6, cc = e % 6;
      const double *om = &rec[REC_OMEGA], *vb = &rec[REC_VBODY], *cm = &rec[REC_CMD];
      const double icp = rec[REC_INVCP], tnp = rec[REC_TANP], yawr = tnp * om[0] + om[2] - cm[2];
      double p0, p1 = 0.0, r0 = 0.0, r1, r2 = 0.0;
      if (cc == 0) { p0 = c->w[6] * om[0]; r0 = icp * c->w[0] * rec[REC_ROLL]; r1 = icp * c->w[0] * icp * om[0] + tnp * c->w[2] * yawr; }
      else if (cc == 1) { p0 = c->w[7] * om[1]; r0 = c->w[1] * rec[REC_PITCH]; r1 = c->w[1] * om[1]; }
      else if (cc == 2) { p0 = c->w[8] * (om[2] - cm[2]); r1 = c->w[2] * yawr; }
      else if (cc < 5) { const double ev = vb[cc - 3] - cm[cc - 3]; p0 = c->w[9 + cc - 3] * ev * body_val<MU4>(c, rec, BODY_INV_MASS); r1 = c->w[3 + cc - 3] * ev * body_val<MU4>(c, rec, BODY_INV_MASS); }
      else {
        p0 = c->w[11] * vb[2] * body_val<MU4>(c, rec, BODY_INV_MASS); p1 = -c->w[11] * c->g * body_val<MU4>(c, rec, BODY_INV_MASS);
        r0 = c->w[5] * (rec[REC_COMZ] - body_val<MU4>(c, rec, BODY_HEIGHT)) * body_val<MU4>(c, rec, BODY_INV_MASS); r1 = c->w[5] * vb[2] * body_val<MU4>(c, rec, BODY_INV_MASS); r2 = -0.5 * c->w[5] * c->g * body_val<MU4>(c, rec, BODY_INV_MASS);
      }
      double acc = 0.0;
      for (int k = a; k < H; k++) {
        const double kd = (double)(k + 1) * dt;
        const double g1 = fma(p1, kd, p0), g2 = fma(fma(r2, kd, r1), kd, r0);
        acc += dt * g1 + ((double)(k - a) + 0.5) * dt * dt * g2;
      }
      qw[e] = 2.0 * acc;
    }
    __syncthreads();
    if (tid < 36) {
      const int i = tid / 6, j = tid % 6;
      const double im2 = body_val<MU4>(c, rec, BODY_INV_MASS) * body_val<MU4>(c, rec, BODY_INV_MASS);
      double su = 0.0, sv = 0.0;
#pragma unroll
      for (int r = 0; r < 6; r++) {
        const double li = Lm[r * 6 + i], lj = Lm[r * 6 + j];
        su = fma((r < 3 ? c->w[6 + r] : c->w[9 + r - 3] * im2) * li, lj, su);
        // rows of R6 L: (invcp L0, L1, tanp L0 + L2, L3, L4, L5)
        double ri = li, rj = lj;
        if (r == 0) { ri = rec[REC_INVCP] * li; rj = rec[REC_INVCP] * lj; }
        if (r == 2) { ri = fma(rec[REC_TANP], Lm[i], li); rj = fma(rec[REC_TANP], Lm[j], lj); }
        sv = fma((r < 3 ? c->w[r] : c->w[3 + r - 3] * im2) * ri, rj, sv);
      }
      AU[tid] = su * dt * dt;
      AV[tid] = sv * dt * dt * dt * dt;
    }
    for (int e = tid; e < NW; e += NT) {   // qh = L' q_w per step
      const int a = e / 6, cc = e % 6;
      double s = 0.0;
      for (int r = cc; r < 6; r++) s = fma(Lm[r * 6 + cc], qw[a * 6 + r], s);
      qh[e] = s;
    }
    __syncthreads();
    // Up to two ADMM stages with their own factorisation (rho, then rho2 for the robots still moving after admm_switch
    // iterations), as in qp_tile_robot; z and y are parked across the second sweep: the 256-lane grid parks them in LDS, the
    // one-wave grid -- whose sweep leaves the room and whose staging area takes the LDS -- keeps them in registers.
    double ypark[3] = {0.0, 0.0, 0.0};
    int it = 0, stage = 0;
    int it_limit = (c->rho2 > 0.0 && c->admm_abs_tol > 0.0 && c->admm_switch < c->admm_iters) ? c->admm_switch : c->admm_iters;
    bool converged = false;
    double zb[3] = {0.0, 0.0, ((tid >> 2) < H && (tid & 3) < NC) ? lo : 0.0};
    for (bool again = true; again;) {
    again = false;
    const double aa = uniform_f64(c->alpha + rho), inv_aa = uniform_f64(1.0 / aa), rho_aa = uniform_f64(rho * inv_aa);
    // ---- my T x T tile of a I + K' (identity in the padding) ----
    double tile[T][T];
    {   // on its own copy of the lane index: (lr, lc) are not kept across the ADMM loop of the stage before
      const int ts = wg_lane<NT>();
      if (stage == 0) stamp_phase(0);
      if constexpr (SYM6) {
        // every 6 x 6 block of a I + K' once: build (a lane below the block diagonal starts with the mirror image of its block),
        // symmetric sweep, move into the 8 x 8 tiles (rows in the reduce-scatter's order, diagonal offset removed)
        double X[6][6];
        int sbr, sbc;
        bool son;
        sym6_lane<10>(ts, sbr, sbc, son);
        sym6_build_kron6<H>(X, tabN, tabS, AU, AV, sbc, sbr, son, aa);
        if (stage == 0) stamp_phase(1);
        sym6_sweep<10, 10, NT>(X, pbuf, sbr, sbc, son);
        if (stage == 0) stamp_phase(2);
        sym6_to_tile8<10, 10, LG, NT>(X, sbr, sbc, son, tile, lds + LY::stage, ts);
        __syncthreads();
        if (ts >= NW && ts < NP) vv[TileShape<T>::pad(ts)] = 0.0;   // padding of the mat-vec input (the staging area went over it): must not hold NaN bits
      } else {
        const int lr = ts >> LG, lc = ts & (LC - 1);
        build_tile_entries<T, H, 6>(tile, tabN, tabS, AU, AV, lr, lc, NW, aa);
        if (stage == 0) stamp_phase(1);
        tile_sweep<T, LG, NW>(tile, pbuf, lr, lc);
        if (stage == 0) stamp_phase(2);
        finish_swept_tile4(tile, lr, lc);
      }
    }
    // lane roles of the iteration, from a fresh lane index (WrenchLane)
    const int tid = wg_lane<NT>();
    const WrenchLane<H, LG, T> L(tid);
    const int io = L.io, iov_pad = L.iov_pad, bk = L.bk, bj = L.bj, b0 = L.b0, b1 = L.b1, rA = L.rA, rB = L.rB, padA = L.padA, padB = L.padB;
    const bool own_real = L.own_real, quad_real = L.quad_real, blk_real = L.quad_real && L.bj < NC;
    const int lr = tid >> LG, lc = tid & (LC - 1);
    // ---- block-lane state ----
    // Lanes with b0 = 1 keep the second half of the six wrench sums in the quad reduce-scatter, so they hold the
    // rows of their Ch block rotated by three: "keep the first three, send the last three" is then right for
    // every lane (12 v_cndmask per iteration less); they read u rotated the same way.
    double Cb[6][3];
#pragma unroll
    for (int cc = 0; cc < 6; cc++) {
      const int src = b0 ? (cc + 3) % 6 : cc;
#pragma unroll
      for (int d = 0; d < 3; d++) Cb[cc][d] = blk_real ? Ch[src * m3 + 3 * bj + d] : 0.0;
    }
    const int ubase0 = L.ubase0, ubase1 = L.ubase1;   // u6 rows 0..2 and 3..5 in this lane's order
    // friction coefficient of this block lane's leg and the projection's constants (one scalar set unless MU4)
    const double mu = leg_mu<MU4>(c, rec, MU4 ? nth_leg(cmask, bj) : 0);
    double kA, kB;
    if constexpr (MU4) { kA = 1.0 / (1.0 + 2.0 * mu * mu); kB = 1.0 / (1.0 + mu * mu); }
    else { kA = c->proj_kA; kB = c->proj_kB; }   // uniform friction: divided once, when the configuration was uploaded
    // (the constant terms qh[rA], qh[rB], qh[io] are re-read from LDS inside the loop: three more LDS reads per
    // iteration cost less than the scratch reloads six more live VGPRs caused)
    double yb[3] = {0.0, 0.0, 0.0};
    if (stage == 0) {
      if (c->warm) {
        if (st.warm_key[b] == cmask && blk_real) {
#pragma unroll
          for (int d = 0; d < 3; d++) { zb[d] = st.warm_z[(size_t)b * RG_WARM_N + bk * m3 + 3 * bj + d]; yb[d] = st.warm_y[(size_t)b * RG_WARM_N + bk * m3 + 3 * bj + d] * (c->rho / rho); /* stored in units of admm_rho */ }
        }
      }
    } else if constexpr (SYM6) {
#pragma unroll
      for (int d = 0; d < 3; d++) yb[d] = ypark[d];   // (zb is still the iterate)
    } else {
#pragma unroll
      for (int d = 0; d < 3; d++) { zb[d] = zck[d * NT + tid]; yb[d] = yst[d * NT + tid]; }
    }
    // the same movement of z means a dual residual rho times as large: the second stage (rho2 > rho) tests proportionally
    // tighter, so both stages stop at the same stationarity error (a seeded configuration sweep found a stage-2 robot
    // stopping 5x farther from the optimum than stage-1 robots do)
    const double tsc = uniform_f64(rho > c->rho ? c->rho / rho : 1.0);   // (a first stage below admm_rho -- admm_rho34_scale < 1 -- keeps the nominal tolerance)
    const double atol = c->admm_abs_tol * tsc, ptol = c->admm_prim_tol * tsc;
    const int chk = c->admm_check;
    const double etol = c->admm_extrap * atol;
    yst[tid] = INFINITY; yst[NT + tid] = INFINITY; yst[2 * NT + tid] = INFINITY;   // between stage switches yst holds the previous window's movement
    // forces at the previous convergence vote: touched once per admm_check iterations, so they live in LDS
    // ([axis][lane]), not in six VGPRs of a loop that is already at the register limit
    zck[tid] = zb[0]; zck[NT + tid] = zb[1]; zck[2 * NT + tid] = zb[2];
    yck[tid] = yb[0]; yck[NT + tid] = yb[1]; yck[2 * NT + tid] = yb[2];
    dyq[tid] = 0.0; dyq[NT + tid] = 0.0; dyq[2 * NT + tid] = 0.0;
    if (tid == 0) { sum3[12] = 0.0; sum3[13] = 0.0; }   // [12] largest extrapolation gain applied in this stage, [13] remaining_distance_factor of the last vote (see qp_tile_robot)
    // valid windows of displacement history before the current one (0 at the stage start and right after an extrapolation):
    // the rate estimate and a jump need one; the vote right after a jump cannot pass
    int hist = 0;
    it = __builtin_amdgcn_readfirstlane(it);   // wave-uniform: keep the loop control scalar (see qp_tile_robot)
    const int it_end = __builtin_amdgcn_readfirstlane(it_limit);
    int next_chk = it + chk;
    for (; it < it_end; it++) {
      // w = rho Ch~ (z - y) - qh : 6 x 3 block product, then reduce over the four leg lanes of the step
      const double d0 = zb[0] - yb[0], d1 = zb[1] - yb[1], d2 = zb[2] - yb[2];
      double cw[6];
#pragma unroll
      for (int cc = 0; cc < 6; cc++) cw[cc] = fma(Cb[cc][2], d2, fma(Cb[cc][1], d1, Cb[cc][0] * d0));
      double keep[3];
#pragma unroll
      for (int h2 = 0; h2 < 3; h2++) keep[h2] = cw[h2] + dpp_f64<0xB1>(cw[3 + h2]);
#pragma unroll
      for (int h2 = 0; h2 < 3; h2++) keep[h2] += dpp_f64<0x4E>(keep[h2]);
      if (quad_real) {
        vv[padA] = fma(rho, b1 ? keep[2] : keep[0], -qh[rA]);
        if (!b1) vv[padB] = fma(rho, keep[1], -qh[rB]);
      }
      __syncthreads();
      const double tw = tile_matvec<T, LG>(tile, vv, lr, lc);   // (a I + K')^-1 w
      if (own_real) uv[io] = fma(-(vv[iov_pad] + qh[io]), inv_aa, tw);
      __syncthreads();
      constexpr bool LATE = NT == 64 && !MU4;   // wrench_admm_vote_late: the vote looks at the estimates and at |x - z| only when the movement leaves it open
      double pres = 0.0, xr[3] = {0.0, 0.0, 0.0};
      const bool vote_now = atol > 0.0 && it + 1 == next_chk;   // uniform: the primal residual is only needed on vote iterations
      if (blk_real) {
        const double u6[6] = {uv[ubase0], uv[ubase0 + 1], uv[ubase0 + 2], uv[ubase1], uv[ubase1 + 1], uv[ubase1 + 2]};
        double x[3] = {rho_aa * d0, rho_aa * d1, rho_aa * d2};
#pragma unroll
        for (int cc = 0; cc < 6; cc++) {
#pragma unroll
          for (int d = 0; d < 3; d++) x[d] = fma(Cb[cc][d], u6[cc], x[d]);
        }
        const double w0 = relax * x[0] + (1.0 - relax) * zb[0] + yb[0];
        const double w1 = relax * x[1] + (1.0 - relax) * zb[1] + yb[1];
        const double w2 = relax * x[2] + (1.0 - relax) * zb[2] + yb[2];
        double px, py, pz;
        proj_pyramid(w0, w1, w2, mu, lo, hi, kA, kB, px, py, pz);
        if constexpr (LATE) { xr[0] = x[0]; xr[1] = x[1]; xr[2] = x[2]; }
        else if (vote_now) pres = fmax(fmax(fabs(x[0] - px), fabs(x[1] - py)), fabs(x[2] - pz));   // primal residual |x - z|
        yb[0] = w0 - px; yb[1] = w1 - py; yb[2] = w2 - pz;
        zb[0] = px; zb[1] = py; zb[2] = pz;
      }
      if (vote_now) {
        next_chk += chk;
        bool done;
        if constexpr (LATE) done = wrench_admm_vote_late(c, tid, blk_real, zb, yb, zck, yst, yck, dyq, sum3, xr, atol, etol, ptol, it, hist);
        else done = wrench_admm_vote<NT>(c, tid, blk_real, zb, yb, zck, yst, yck, dyq, sum3, pres, atol, etol, ptol, it, hist);
        if (done) { it++; converged = true; break; }
      }
    }
    if (!converged && atol > 0.0 && it < c->admm_iters) {   // second stage
      const double sc = rho / c->rho2;
#pragma unroll
      for (int d = 0; d < 3; d++) {
        if constexpr (SYM6) ypark[d] = yb[d] * sc;
        else { zck[d * NT + tid] = zb[d]; yst[d * NT + tid] = yb[d] * sc; }
      }
      rho = c->rho2;
      it_limit = c->admm_iters;
      stage = 1;
      again = true;
      __syncthreads();
      continue;
    }
    stamp_phase(3);
    const QpKernArgsP ka = reread_kernel_args();
    // (block-lane indices from a fresh lane index: the warm-start addresses of the load above are then not kept -- spilled --
    // across the ADMM loop)
    const int te = wg_lane<NT>(), bke = te >> 2, bje = te & 3;
    const bool blk_e = bke < H && bje < NC;
    if (c->warm) {
      if (blk_e) {
#pragma unroll
        for (int d = 0; d < 3; d++) { ka->st.warm_z[(size_t)b * RG_WARM_N + bke * m3 + 3 * bje + d] = (float)zb[d]; ka->st.warm_y[(size_t)b * RG_WARM_N + bke * m3 + 3 * bje + d] = (float)(yb[d] * (rho / c->rho)); /* first-stage units */ }
      }
      __syncthreads();
      if (te == 0) ka->st.warm_key[b] = ((converged && !degenerate) || atol == 0.0) ? cmask : -1;   // never warm-start from an unconverged iterate
    }
    if (te == 0) {
      if (degenerate) converged = false;
      if (c->solver == RG_SOLVER_AUTO && atol > 0.0 && !converged) {   // hand the robot to the exact solver
        const int slot = atomicAdd(&ka->st.counts[8 + NC], 1);
        ka->st.bins[(size_t)(5 + NC) * ka->B + slot] = b;
      } else if (degenerate || (atol > 0.0 && !converged)) atomicAdd(&ka->st.counts[7], 1);   // no exact pass: a failure
      ka->st.iters[b] = it;
      if (converged) ka->st.hard[b] = 0;   // direct routing (front kernel): ADMM solves this robot again
    }
    if (blk_e && bke == 0) {
      const int leg = nth_leg(cmask, bje);
      grf[3 * leg] = -zb[0]; grf[3 * leg + 1] = -zb[1]; grf[3 * leg + 2] = -zb[2];
    }
    }   // stage loop
    const int tid = wg_lane<NT>();
    __syncthreads();
    audit_capture<NT>(converged && !degenerate, b, NC, rec, grf);
    qp_write_outputs<NT>(c, rec, grf, b, tid, RG_QP_SOLVE);
  }
}

template <int NC, int H, int LG, int T = 8>
constexpr size_t qp_wrench_lds_doubles() { return (size_t)WrenchLds<NC, H, LG, T>::total; }
