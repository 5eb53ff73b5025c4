// rg_qp_tile_kernel.inc -- force-space ADMM QP body on 2-D register tiles (one and two stance legs) and its LDS layout.  (The
// tile primitives it shares with the other bodies are in rg_qp_tile.inc; the exact active-set bodies are in
// rg_qp_exact_kernel.inc / rg_qp_sched_kernel.inc.)
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// One robot's QP on the LC x LC lanes of the calling workgroup.  tabN / tabS: 2 N_ab, 2 S_ab in LDS
// (loaded by the caller once per workgroup); lds: this body's scratch, qp_tile_lds_doubles() long.
template <int NC, int H, int T, int LG, bool MU4 = false>
__device__ __forceinline__ void qp_tile_robot(const DevCfg *__restrict__ c, const DevState &st, const DevOut &out, const int B, const int b,
                                              const double *tabN, const double *tabS, double *lds) {
  constexpr int m3 = 3 * NC;
  constexpr int N = m3 * H;          // real QP variables
  constexpr int LC = 1 << LG;        // lanes per side
  constexpr int NP = T * LC;         // padded size
  constexpr int NT = LC * LC;
  static_assert(T == 4 || T == 8, "tile sizes with a reduce-scatter below: 8 and 4");
  static_assert(NP >= N && T <= LC, "tile/grid must cover the problem");
  // opaque copy: the lane-role integers below are recomputed per robot instead of being hoisted out of the
  // caller's work loop for all bodies at once and spilled (43 scratch stores in the fused kernel's preamble)
  const int tid = wg_lane<NT>();
  const int lr = tid >> LG, lc = tid & (LC - 1);
  // LDS vectors read as T-wide groups (one group per lane-column) use a padded group stride TS so the
  // 16-B reads of different groups never share a bank (T = 8: 64-B groups are 2-way conflicting,
  // rocprof SQ_LDS_BANK_CONFLICT = 30-55 % of LDS cycles; stride 80 B is conflict-free for 8 and 16 groups).
  constexpr int TS = (T == 8) ? 10 : T;
  constexpr int NPAD = TS * LC;
  constexpr int NPB = NPAD + 2;
  double *pbuf = lds;                // 2 * NPB  ping-pong pivot row (padded); [NPAD] = pivot d
  double *vv = pbuf + 2 * NPB;       // NPAD rhs vector (padded)
  double *wv = vv + NPAD;            // NP projection input (unpadded, scalar accesses)
  double *GU = wv + NP;              // m3*m3
  double *GV = GU + m3 * m3;
  double *c1 = GV + m3 * m3;         // N
  double *c2 = c1 + N;               // N
  double *Bw = c2 + N;               // 3*m3
  double *TBw = Bw + 3 * m3;         // 3*m3
  double *rec = TBw + 3 * m3;        // RG_REC_N
  double *grf = rec + RG_REC_N;      // 24
  constexpr bool KRON6 = (m3 == 6 && T == 8);   // branch-free tile build from periodic 6 x 6 tables (ADMM, two legs)
  double *EU = grf + 24;             // RG_E6_DOUBLES when KRON6
  double *EV = EU + (KRON6 ? RG_E6_DOUBLES : 0);
  double *mprev = EV + (KRON6 ? RG_E6_DOUBLES : 0);   // NP (ADMM only): each row's (signed) movement of z over the previous vote window
  double *ychk = mprev + NP;         // NP (ADMM only): y at the last vote
  double *dyprev = ychk + NP;        // NP (ADMM only): movement of y over the previous vote window
  double *sum3 = dyprev + NP;        // 16 (ADMM only): sum3_publish / _collect slots [0..11], largest extrapolation gain of the stage [12], remaining_distance_factor of the last vote [13]
  double rho = c->rho;   // second ADMM stage: c->rho2 (see the stage loop below)
  const double relax = c->relax;
  double lo = c->fz_min, hi = c->fz_max;   // (MU4: the robot's, once its record is in LDS)
  // the one matrix row whose scalar ADMM state this lane owns after the reduce-scatter
  const bool owner = lc < T;
  // T == 8: the reduce-scatter below pairs lanes as (7-i), (i^1), (i^2) -> kept row 4*b2 + 2*b0 + b1; T == 4: 2*b0 + b1
  const int own_a = TileShape<T>::own_a(lc);
  const int io = lr * T + own_a;
  const bool own_real = owner && io < N;
  const int iov_pad = lr * TS + own_a;   // position of row io in the padded vectors

  {
    __syncthreads();
    for (int e = tid; e < RG_REC_N; e += NT) rec[e] = st.rec[(size_t)b * RG_REC_N + e];
    if (tid < 24) grf[tid] = 0.0;
    __syncthreads();
    const int cmask = (int)rec[REC_CONTACT];
    if constexpr (MU4) { lo = body_val<MU4>(c, rec, BODY_FZ_MIN); hi = body_val<MU4>(c, rec, BODY_FZ_MAX); }
    force_space_tables<NC, H, NT, KRON6, MU4>(c, rec, cmask, tid, Bw, TBw, GU, GV, EU, EV, c1, c2);
    __syncthreads();
    // ADMM runs in up to two stages with their own factorisation: robots that have not converged after admm_switch
    // iterations at rho are stragglers with many constraints active in stiff directions; they re-factorise with the larger
    // rho2 and carry their iterate over (the scaled multiplier y = lambda / rho is rescaled) instead of crawling to the cap
    // and going through the exact re-solve launch -- one such robot used to cost the whole tick ~50 us of latency.
    double z = 0.0;
    int it = 0;
    int stage = 0;
    bool audit_ok = false;    // ADMM converged: the robot may be picked by the audit lane
    int it_limit = (c->rho2 > 0.0 && c->admm_abs_tol > 0.0 && c->admm_switch < c->admm_iters) ? c->admm_switch : c->admm_iters;
    for (bool again = true; again;) {
    again = false;
    // ---- my T x T tile of (P + rho I) (identity in the padding), and q of the row I own ----
    double tile[T][T];
    double qi = 0.0;
    {
      int lrv = lr, lcv = lc, iov = io;   // opaque copies defeat LICM of ~4 T^2 LDS addresses
      asm volatile("" : "+v"(lrv), "+v"(lcv), "+v"(iov));
      if (own_real) {
        const int a = iov / m3, i = iov - a * m3;
        for (int kq = a; kq < H; kq++) qi += c1[kq * m3 + i] + ((double)(kq - a) + 0.5) * c2[kq * m3 + i];
        qi *= 2.0;
      }
      // (one leg: the loop of build_tile_entries, written out -- called, it compiles to different code in the fused kernels)
      if constexpr (KRON6) build_tile_kron6<H>(tile, tabN, tabS, EU, EV, lrv, lcv, N, c->alpha + rho);
      else
#pragma unroll
      for (int ta = 0; ta < T; ta++) {
        const int row = lrv * T + ta;
        const int a = row / m3, i = row - a * m3;
        const bool rreal = row < N;
        const double *tN = tabN + (rreal ? a : 0) * H, *tS = tabS + (rreal ? a : 0) * H, *gu = GU + (rreal ? i : 0), *gv = GV + (rreal ? i : 0);
#pragma unroll
        for (int tb = 0; tb < T; tb++) {
          const int col = lcv * T + tb;
          const int bb = col / m3, j = col - bb * m3;
          double v;
          if (rreal && col < N) {
            v = tN[bb] * gu[j * m3] + tS[bb] * gv[j * m3];
            if (col == row) v += c->alpha + rho;
          } else v = (col == row) ? 1.0 : 0.0;
          tile[ta][tb] = v;
        }
        __builtin_amdgcn_sched_barrier(0);  // one tile row at a time: bounds the LDS loads in flight (VGPR pressure)
      }
    }
    // ---- symmetric sweep: tile <- entries of -(P + rho I)^-1, diagonal entries offset by +2 ----
    tile_sweep<T, LG, N>(tile, pbuf, lr, lc);
    // the sweep leaves +2 on every diagonal entry (patch trick above); remove it once: tile = -G
    if (lr == lc) {
#pragma unroll
      for (int ta = 0; ta < T; ta++) tile[ta][ta] -= 2.0;
    }
    if constexpr (T == 8) permute_tile_rows_for_reduce(tile, lc);
    {
    // ---- over-relaxed ADMM; scalar state lives on the owner lane of each row ----
    // (contact schedules never come here: rg_qp_sched_kernel.inc solves them with the absent blocks eliminated)
    double y = 0.0;
    if (stage == 0) {
      z = (own_real && (io % 3) == 2) ? lo : 0.0;
      if (c->warm) {   // previous tick's iterate of this robot, valid while its contact set is unchanged
        if (st.warm_key[b] == cmask && own_real) { z = st.warm_z[(size_t)b * RG_WARM_N + io]; y = st.warm_y[(size_t)b * RG_WARM_N + io]; }
      }
    } else if (own_real) { z = wv[io]; y = vv[iov_pad]; }   // second stage: the iterate parked by the first
    __syncthreads();
    const int blk = own_real ? io - io % 3 : 0, dax = io % 3;
    // friction coefficient of the leg of this lane's force block (block = step * NC + stance-leg slot) and the projection's constants
    const double mu = leg_mu<MU4>(c, rec, MU4 ? nth_leg(cmask, (blk / 3) % NC) : 0);
    const double kA = 1.0 / (1.0 + 2.0 * mu * mu), kB = 1.0 / (1.0 + mu * mu);
    if (owner) vv[iov_pad] = own_real ? rho * (z - y) - qi : 0.0;
    __syncthreads();
    // the same movement of z means a dual residual rho times as large: the second stage (rho2 > rho) tests proportionally
    // tighter, so both stages stop at the same stationarity error (a seeded configuration sweep found a stage-2 robot
    // stopping 5x farther from the optimum than stage-1 robots do)
    const double tsc = uniform_f64(c->rho / rho);
    const double atol = c->admm_abs_tol * tsc, ptol = c->admm_prim_tol * tsc;
    const int chk = c->admm_check;
    const double etol = c->admm_extrap * atol;
    double zchk = z;
    if (owner) { mprev[io] = INFINITY; ychk[io] = y; dyprev[io] = 0.0; }
    if (tid == 0) { sum3[12] = 0.0; sum3[13] = 0.0; }   // [12] largest extrapolation gain applied in this stage; [13] remaining_distance_factor of the last vote
    // valid windows of displacement history before the current one (0 at the stage start and right after an extrapolation):
    // the rate estimate and a jump need one; the vote right after a jump cannot pass
    int hist = 0;
    // (it and it_limit are wave-uniform, but carried around the stage loop the compiler keeps them in VGPRs and turns the
    // loop control below into exec-mask arithmetic: +10 instructions per iteration.  Pin them back into SGPRs.)
    it = __builtin_amdgcn_readfirstlane(it);
    const int it_end = __builtin_amdgcn_readfirstlane(it_limit);
    int next_chk = it + chk;
    bool converged = false;
    for (; it < it_end; it++) {
      double acc[T];
      {
        double vloc[T];
#pragma unroll
        for (int t2 = 0; t2 < T; t2 += 2) {
          double2 v2 = *reinterpret_cast<const double2 *>(&vv[lc * TS + t2]);
          vloc[t2] = v2.x; vloc[t2 + 1] = v2.y;
        }
#pragma unroll
        for (int ta = 0; ta < T; ta++) {
          double a0 = 0.0;
#pragma unroll
          for (int tb = 0; tb < T; tb++) a0 = fma(tile[ta][tb], vloc[tb], a0);
          acc[ta] = a0;
        }
      }
      // reduce over the LC lanes of this lane-row
      double tot;
      if constexpr (T == 8) {
        // reduce-scatter over the 8 lanes of a half-row, all in DPP (no LDS round trips): step 1 pairs
        // i <-> 7-i (row_half_mirror), step 2 i^1, step 3 i^2; the tile rows were reordered after the sweep
        // so every lane keeps its low half.  Lane-rows of 16/32 lanes finish with all-reduce steps.
        tot = reduce_scatter8_permuted<LG>(acc, lc);
      } else {
        // reduce-scatter: after step k (xor 2^k) a lane keeps the half selected by bit k of lc
        constexpr int LT = 2;   // log2 T
#pragma unroll
        for (int k = 0; k < LT; k++) {
          const int half = T >> (k + 1);
          const bool up = (lc >> k) & 1;
#pragma unroll
          for (int h2 = 0; h2 < half; h2++) {
            double keep = up ? acc[half + h2] : acc[h2];
            double send = up ? acc[h2] : acc[half + h2];
            acc[h2] = keep + __shfl_xor(send, 1 << k);
          }
        }
        tot = acc[0];
#pragma unroll
        for (int k = LT; k < LG; k++) tot += __shfl_xor(tot, 1 << k);
      }
      const double u = -tot;
      const double w = relax * u + (1.0 - relax) * z + y;
      if (own_real) wv[io] = w;
      __syncthreads();
      if (own_real) {
        double px, py, pz;
        proj_pyramid(wv[blk], wv[blk + 1], wv[blk + 2], mu, lo, hi, kA, kB, px, py, pz);
        const double zn = (dax == 0) ? px : (dax == 1 ? py : pz);
        y = w - zn;
        z = zn;
        vv[iov_pad] = rho * (z - y) - qi;
      }
      if (atol > 0.0 && it + 1 == next_chk) {
        // one robot per workgroup: a data-dependent exit costs no divergence, only this vote
        // converged = the forces stopped moving AND the unprojected iterate agrees with them: a z pinned on
        // its bounds while the multipliers still drift (statically unbalanced gaits) must not pass
        // ... AND, third, the distance still to go is small if the window movements keep shrinking geometrically:
        // m r / (1 - r) with r = m / m_prev.  A crawling robot (r ~ 0.9) moves less than the tolerance per window
        // while it is still 10 windows' worth away; this is what let rare robots stop 1e-4 off in a 300k robot-tick run.
        const double dz = z - zchk, dzp = owner ? mprev[io] : INFINITY;
        const double m = fabs(dz), mp = fabs(dzp);
        double est = (mp > m && mp < 1.0e300) ? m * m * fast_rcp(mp - m) : 0.0;   // first window, or not shrinking: no estimate, the plain tests decide
        // a robot that was extrapolated has a mode of known shrink rate r = g / (1 + g): whatever is left of it after the
        // jump moves by (1 - r) of its size per window, so the same estimate with the known rate is m g (a single-leg robot
        // that used to go to the exact solver "stopped" 1e-4 off after its jumps without this)
        const double gst = sum3[12];
        if (gst > 0.0) est = fmax(est, m * fmax(gst, sum3[13]));   // ... and, once it has jumped, with the rate of the whole iterate measured at the previous vote
        // after an extrapolation the sequence is no longer one geometric decay: the movement can collapse within one window
        // when z lands on a new face and then creep on at a rate nobody has measured (seed 97 of the configuration sweep:
        // 2.5e-3 -> 1e-4 N in one window, then still 3e-2 N from the optimum).  A robot that has jumped in this stage passes
        // only with TWO consecutive quiet windows (the previous one within 4x the tolerance), so that the rate between them
        // means something -- and never in the vote right after the jump.
        const int moving = (own_real && (m > atol || est > etol || fabs(u - z) > ptol || (gst > 0.0 && mp > 4.0 * atol))) || (gst > 0.0 && hist <= 0);
        const double dy = owner ? y - ychk[io] : 0.0, dyp = owner ? dyprev[io] : 0.0;
        if (owner) { mprev[io] = dz; ychk[io] = y; dyprev[io] = dy; }
        zchk = z;
        next_chk += chk;
        // dominant-mode rate / extrapolation of (z, y), see extrapolation_gain(): from the iteration count typical robots need
        // on, with one full window of history before the current one (all of it wave-uniform)
        // (not for a single stance leg: that QP is degenerate -- one foot cannot balance the body -- its ADMM iterates drift
        // rather than decay, and an extrapolated one can sit still 1e-4 away from the optimum with every residual inside
        // its tolerance (seeds 4 and 235 of the configuration sweep).  Left alone such robots run to the cap and are solved
        // exactly, as before.)
        const bool rate_now = NC >= 2 && hist >= 1 && c->accel_from > 0 && it + 1 >= c->accel_from;
        double d11 = own_real ? dz * dz + dy * dy : 0.0, d00 = (own_real && hist >= 1) ? dzp * dzp + dyp * dyp : 0.0, d10 = (own_real && hist >= 1) ? dz * dzp + dy * dyp : 0.0;
        if (rate_now) sum3_publish<NT>(d11, d00, d10, sum3);
        if (!workgroup_any<NT>(moving)) { it++; converged = true; break; }
        if (rate_now) {
          sum3_collect<NT>(d11, d00, d10, sum3);
          const double g = extrapolation_gain(c->accel_k, d11, d00, d10);
          const bool jump = __builtin_amdgcn_readfirstlane(g > 0.0);   // same g in every lane: keep the branch (and hist) scalar
          if (tid == 0) { sum3[13] = jump ? 0.0 : remaining_distance_factor(c->accel_k, d11, d00, d10); if (jump) sum3[12] = fmax(gst, g); }
          if (jump) {
            if (own_real) {
              z = fma(g, dz, z); y = fma(g, dy, y);
              vv[iov_pad] = rho * (z - y) - qi;
              ychk[io] = y;
            }
            zchk = z;
            hist = -1;
            if constexpr (NT > 64) __syncthreads();   // vv was rewritten after the vote's barriers
          }
        }
        hist++;
      } else __syncthreads();
    }
    if (!converged && atol > 0.0 && it < c->admm_iters) {   // second stage: re-factorise with rho2, carry (z, y) over through LDS
      __syncthreads();
      if (own_real) { wv[io] = z; vv[iov_pad] = y * (rho / c->rho2); }
      rho = c->rho2;
      it_limit = c->admm_iters;
      stage = 1;
      again = true;
      __syncthreads();
      continue;
    }
    const QpKernArgsP ka = reread_kernel_args();
    if (c->warm) {
      if (own_real) { ka->st.warm_z[(size_t)b * RG_WARM_N + io] = (float)z; ka->st.warm_y[(size_t)b * RG_WARM_N + io] = (float)(y * (rho / c->rho)); /* y = lambda / rho, stored in first-stage units */ }
      __syncthreads();   // all reads of warm_key above are done before it is rewritten
      // an iterate that did not converge is no starting point: the next tick would crawl from it and pass the "stopped moving"
      // test far from the optimum (found by a 80k robot-tick parity run: 1.3e-4 torque error right after a re-solved tick)
      if (tid == 0) ka->st.warm_key[b] = (converged || atol == 0.0) ? cmask : -1;
    }
    audit_ok = converged;
    if (c->solver == RG_SOLVER_AUTO && atol > 0.0 && !converged && tid == 0) {   // hand the robot to the exact solver
      const int slot = atomicAdd(&ka->st.counts[8 + NC], 1);
      ka->st.bins[(size_t)(5 + NC) * ka->B + slot] = b;
    } else if (atol > 0.0 && !converged && tid == 0) atomicAdd(&ka->st.counts[7], 1);   // RG_SOLVER_ADMM: reported as a failure
    }
    }   // stage loop
    const QpKernArgsP kb = reread_kernel_args();
    if (tid == 0) {
      kb->st.iters[b] = it;
      // the front kernel's direct routing: marked while the exact solver has to solve this robot, cleared when ADMM converges
      if (audit_ok) kb->st.hard[b] = 0;
    }
    if (own_real && io < m3) grf[3 * nth_leg(cmask, io / 3) + io % 3] = -z;
    __syncthreads();
    audit_capture<NT>(audit_ok, b, NC, rec, grf);
    qp_write_outputs<NT>(c, rec, grf, b, tid, RG_QP_SOLVE);
  }
}

template <int NC, int H, int T, int LG>
constexpr size_t qp_tile_lds_doubles() {
  constexpr int m3 = 3 * NC, N = m3 * H, LC = 1 << LG, NP = T * LC;
  constexpr int TS = (T == 8) ? 10 : T, NPAD = TS * LC;
  size_t n = (size_t)(2 * (NPAD + 2) + NPAD + NP + 2 * m3 * m3 + 2 * N + 6 * m3 + RG_REC_N + 24);
  if (m3 == 6 && T == 8) n += 2 * RG_E6_DOUBLES;
  return n + 3 * NP + 16;
}
