// rg_qp_sched_kernel.inc -- QP body for per-step contact schedules (contact_lookahead), solved in wrench coordinates.
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// ------------------------------------------------------------------------------------
// With a contact schedule the set S_k of legs in contact differs from horizon step to horizon step.  A (step, leg)
// pair that is not in contact carries no force: it is not a variable of the QP.  (Round 1 kept every robot on the
// four-leg problem and pinned such blocks to zero in the ADMM projection; a pinned block is a constraint that is
// active in a stiff direction of P, exactly the case fixed-rho ADMM crawls on: with BASELINE config 5's randomised
// schedule a quarter of the robots hit the iteration cap.)  Eliminating them exactly keeps the wrench-space reduction
// of rg_qp_wrench_kernel.inc, with one factor per step:
//     C_k = [ Iw^-1 [r_l]x ; I3 ]_{l in S_k}   (6 x 3|S_k|),     C_k C_k' = L_k L_k'   (semidefinite Cholesky:
//     rank 3 / 5 / 6 for one / two / three-four legs; a zero pivot gives a zero column of L_k),
//     Ch_k = L_k^+ C_k  (orthonormal non-zero rows),     P = alpha I + X K' X',   X = blockdiag(Ch_k)',
//     K'[(a,i),(b,j)] = 2 N_ab (L_a' A_U L_b)_ij + 2 S_ab (L_a' A_V L_b)_ij          (6H x 6H, no longer Kronecker),
//     (P + rho I)^-1 v = v / a + X [ (a I + K')^-1 - I / a ] X' v,    a = alpha + rho    (exact also when rank L_k < 6:
//     X'X is then a 0/1 diagonal projector and K' has zero rows/columns there).
// The matrix to invert stays 6H x 6H (one wave at H = 10, 256 lanes at H = 20) whatever the schedule; a rank-deficient
// stance (collinear feet, one or two legs) needs no special case.  A_U = dt^2 diag(wU) and A_V = dt^4 R6' diag(wV) R6
// factor, so with LU_k = sqrt(wU) dt L_k and MV_k = sqrt(wV) dt^2 R6 L_k (6 x 6 per step, in LDS)
//     K' block (a,b) = 2 N_ab LU_a' LU_b + 2 S_ab MV_a' MV_b :  12 FMAs per tile entry.
// Lane roles are those of qp_wrench_robot: tile lane (8 x 8 register tile), owner lane of a wrench row, block lane
// 4 k + j = (horizon step k, leg j) holding z, y and its 6 x 3 block of Ch_k in registers.
// AS = true: exact dual active-set method on the same reduced inverse (rho = 0), for the robots ADMM leaves unconverged.
// ------------------------------------------------------------------------------------

// Cholesky of a positive SEMI-definite 6 x 6 matrix (registers, static indices): zero pivots give zero columns.
// `maxrank` is the rank the contact count allows (3 / 5 / 6): once that many pivots were taken the rest are zero by
// construction, whatever rounding left in them (a two-leg step's sixth pivot comes out as ~1e-12 of garbage).
// The caller hands the matrix over in an elimination order in which every pivot that is not zero by construction is well
// away from zero (see the per-step factors in qp_sched_robot), so the test only has to tell rounding residue (<= 1e-13 of
// the diagonal entry) from a pivot.  It used to be 1e-9 in the natural order: a diagonal pair of feet whose line passes
// within ~1e-5 m of the centre of mass (horizontal projection) has a fifth pivot of 5.6e-10 of its diagonal entry there --
// dropped, and the first-step forces came out 2e-5 off (one case of a 2000-seed configuration sweep, 1.6e-4 on one joint).
__device__ __forceinline__ void semidefinite_cholesky6(const double (&Q)[6][6], const int maxrank, double (&L)[6][6], double (&Li)[6]) {
  int rank = 0;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double s = Q[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) s = fma(-L[j][k], L[j][k], s);
    const bool take = rank < maxrank && s > 1e-11 * Q[j][j];
    rank += take ? 1 : 0;
    const double d = take ? sqrt(s) : 0.0;
    L[j][j] = d;
    Li[j] = take ? 1.0 / d : 0.0;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double t = Q[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) t = fma(-L[i][k], L[j][k], t);
      L[i][j] = t * Li[j];
    }
#pragma unroll
    for (int i = 0; i < j; i++) L[i][j] = 0.0;
  }
}

// My 8 x 8 tile of  a I + K'  as a sum of twelve scaled outer products.  LUr / MVr hold LU_k and MV_k by ROW of the 6 x 6
// factors: LUr[r][6 k + i] = LU_k[r][i] (NP doubles per r, zero in the padding), so for a fixed r a lane reads its eight
// row entries and its eight column entries as two 64-byte runs, and
//     tile[ta][tb] += 2 N_ab LUr[r][row] LUr[r][col] + 2 S_ab MVr[r][row] MVr[r][col]        for r = 0..5.
// A range of eight rows or columns straddles at most two 6-wide blocks at an even offset, so four N and four S table
// values cover the tile (as in build_tile_kron6); which of them an entry takes is static except for rows / columns 2..5.
// The r loop stays rolled: 192 LDS doubles, 768 FMAs and ~200 VGPRs.  (The first version dotted 6-vectors per entry, fully
// unrolled: the compiler kept most of the 480 loaded values live -- 3.7 KB of scratch per lane.)
template <int H, int NP>
__device__ __forceinline__ void build_tile_sched(double (&tile)[8][8], const double *tabN, const double *tabS, const double *LUr, const double *MVr,
                                                 const int lr, const int lc, const int nreal, const double diag_real) {
  const int r0 = 8 * lr, c0 = 8 * lc;
  const int a0r = r0 / 6, i0 = r0 - 6 * a0r, b0r = c0 / 6, j0 = c0 - 6 * b0r;   // i0, j0 in {0, 2, 4}
  const int a0 = a0r < H ? a0r : H - 1, a1 = a0r + 1 < H ? a0r + 1 : H - 1;
  const int b0 = b0r < H ? b0r : H - 1, b1 = b0r + 1 < H ? b0r + 1 : H - 1;
  const double n00 = tabN[a0 * H + b0], n01 = tabN[a0 * H + b1], n10 = tabN[a1 * H + b0], n11 = tabN[a1 * H + b1];
  const double s00 = tabS[a0 * H + b0], s01 = tabS[a0 * H + b1], s10 = tabS[a1 * H + b0], s11 = tabS[a1 * H + b1];
#pragma unroll
  for (int ta = 0; ta < 8; ta++)
#pragma unroll
    for (int tb = 0; tb < 8; tb++) tile[ta][tb] = 0.0;
  // the N (x) LU'LU part and the S (x) MV'MV part in turn: with both row/column sets live at once (32 more doubles) the
  // loop spilled ~140 values per lane and stage -- 500 MB of scratch traffic per config-5 launch
#pragma unroll 1
  for (int part = 0; part < 2; part++) {
    const double *tab = part ? MVr : LUr;
    const double f00 = part ? s00 : n00, f01 = part ? s01 : n01, f10 = part ? s10 : n10, f11 = part ? s11 : n11;
#pragma unroll 1
    for (int r = 0; r < 6; r++) {
      double rw[8], cl[8];
#pragma unroll
      for (int t2 = 0; t2 < 8; t2 += 2) {
        const double2 a2 = *reinterpret_cast<const double2 *>(tab + r * NP + r0 + t2), c2 = *reinterpret_cast<const double2 *>(tab + r * NP + c0 + t2);
        rw[t2] = a2.x; rw[t2 + 1] = a2.y; cl[t2] = c2.x; cl[t2 + 1] = c2.y;
      }
#pragma unroll
      for (int ta = 0; ta < 8; ta++) {
        const bool rhi = ta < 2 ? false : (ta >= 6 ? true : i0 + ta >= 6);
        const double lo = (rhi ? f10 : f00) * rw[ta], hi = (rhi ? f11 : f01) * rw[ta];
#pragma unroll
        for (int tb = 0; tb < 8; tb++) {
          const bool chi = tb < 2 ? false : (tb >= 6 ? true : j0 + tb >= 6);
          tile[ta][tb] = fma(chi ? hi : lo, cl[tb], tile[ta][tb]);
        }
      }
    }
  }
  if (lr == lc) {
#pragma unroll
    for (int ta = 0; ta < 8; ta++) tile[ta][ta] += diag_real;
  }
  // padding (only the last lane-row / lane-column has any; the tables are zero there): 1 on the diagonal
  if (r0 + 8 > nreal && lr == lc) {
#pragma unroll
    for (int ta = 0; ta < 8; ta++)
      if (r0 + ta >= nreal) tile[ta][ta] = 1.0;
  }
}

// ... and the same sum for ONE 6 x 6 block (gr, gc) of a I + K' (rg_qp_sym6.inc: every block held once; a lane below the block
// diagonal asks for the mirror image of its block, i.e. block (bc, br)):
//     X[i][j] = sum_r  2 N_ab LU_a[r][i] LU_b[r][j] + 2 S_ab MV_a[r][i] MV_b[r][j],   a = gr, b = gc  (+ a on the diagonal)
// 12 x (6 products + 36 FMAs); the r loop stays rolled like the one above.
template <int H, int NP>
__device__ __forceinline__ void sym6_build_sched(double (&X)[6][6], const double *tabN, const double *tabS, const double *LUr, const double *MVr,
                                                 const int gr, const int gc, const bool on, const double diag) {
  const double n = on ? tabN[gr * H + gc] : 0.0, s = on ? tabS[gr * H + gc] : 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) X[i][j] = (i == j && on && gr == gc) ? diag : 0.0;
#pragma unroll 1
  for (int part = 0; part < 2; part++) {
    const double *tab = part ? MVr : LUr;
    const double f = part ? s : n;
#pragma unroll 1
    for (int r = 0; r < 6; r++) {
      double rw[6], cl[6];
#pragma unroll
      for (int e = 0; e < 6; e += 2) {
        const double2 a2 = *reinterpret_cast<const double2 *>(tab + r * NP + 6 * gr + e), c2 = *reinterpret_cast<const double2 *>(tab + r * NP + 6 * gc + e);
        rw[e] = f * a2.x; rw[e + 1] = f * a2.y; cl[e] = c2.x; cl[e + 1] = c2.y;
      }
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) X[i][j] = fma(rw[i], cl[j], X[i][j]);
    }
  }
}

template <int H, int LG, bool AS>
struct SchedLds {
  static constexpr int T = 8, TS = 10, NW = 6 * H, LC = 1 << LG, NP = T * LC, NT = LC * LC, NPAD = TS * LC, NPB = NPAD + 2;
  static constexpr int NV = 12 * H;                 // force variables, (step, leg, axis); blocks not in contact stay unused
  static constexpr int QMAX = AS ? NV : 0;                      // active constraints the solver has room for: as many as there are variables
  static constexpr int QLDS = AS ? (NV < 160 ? NV : 160) : 0;   // rows of the packed (C_A G C_A')^-1 held in LDS; rows QLDS .. QMAX-1 live in global memory (SPILL doubles per workgroup)
  static constexpr int SPILL = QMAX * (QMAX + 1) / 2 - QLDS * (QLDS + 1) / 2;
  // The ADMM form (AS = false) sweeps the matrix with every 6 x 6 block held once (rg_qp_sym6.inc) and moves it into the 8 x 8
  // tiles through a staging area: what lives through the stages comes first, and the staging area covers the rest (set-up
  // tables, the factor tables LUr / MVr -- rebuilt per stage --, the vote state, which each stage initialises after the move;
  // the iterate of a robot that enters its second stage stays in registers across the sweep).
  static constexpr bool SYM6 = !AS;
  static constexpr int NBS = NW / 6;   // block rows of the symmetric sweep (= H)
  // offsets in doubles
  static constexpr int rec = 0, grf = rec + RG_REC_N, qh = grf + 24, Lk = qh + NW, Lik = Lk + 36 * H /* 1 / pivot by elimination position [H][6], then the coordinate eliminated last [H] */,
                       Cm = Lik + 7 * H, sum3 = Cm + 72, stage = sum3 + (AS ? 0 : 16),
                       pbuf = stage, vv = pbuf + (SYM6 ? 2 * Sym6<NBS>::PB : 2 * NPB), uv = vv + NPAD, Ql = uv + NP, LUr = Ql + 144,
                       MVr = LUr + 6 * NP, qw = MVr + 6 * NP,
                       zck = qw + NW, yst = zck + (AS ? 0 : 3 * NT), yck = yst + (AS ? 0 : 3 * NT), dyq = yck + (AS ? 0 : 3 * NT),
                       stage_end = dyq + (AS ? 0 : 3 * NT),   // yck / dyq / sum3: extrapolation state, see qp_tile_robot
                       as0 = (SYM6 && stage + Sym6<NBS>::STG > stage_end) ? stage + Sym6<NBS>::STG : stage_end;
  // active-set state (AS only)
  static constexpr int as_x = as0, as_g = as_x + NV, as_z = as_g + NV, as_w = as_z + NV, as_lam = as_w + NV, as_sv = as_lam + QMAX, as_r = as_sv + QMAX,
                       as_v0 = as_r + QMAX, as_v1 = as_v0 + QMAX, as_T = as_v1 + QMAX, as_int = as_T + QLDS * (QLDS + 1) / 2,
                       as_sc = as_int + (3 * QMAX + 4 * H + 1) / 2 + 1, total = AS ? as_sc + 8 : as0;
  // what stays live through sym6_to_tile8 ends where the staging area starts, and the staging area fits the layout
  static_assert(!SYM6 || (rec + RG_REC_N <= stage && grf + 24 <= stage && qh + NW <= stage && Lk + 36 * H <= stage && Lik + 7 * H <= stage &&
                          Cm + 72 <= stage && sum3 + 16 <= stage), "sym6_to_tile8 stages over live LDS");
  static_assert(!SYM6 || stage + Sym6<NBS>::STG <= total, "the staging area of sym6_to_tile8 fits the layout");
};

template <int H, int LG, bool AS>
constexpr size_t qp_sched_lds_doubles() { return (size_t)SchedLds<H, LG, AS>::total; }

// Exact dual active-set method of the schedule body (range-space form) on G = P^-1 = I / alpha + X M X', see qp_sched_robot.
// Same method and constraint numbering as the force-space solver in rg_qp_exact_kernel.inc (id = 6 * block + type), with block =
// (step, leg) lane index 4 k + j and variable index 3 * block + axis.  apply_G(in, out, in_is_qh): out = G in on the enabled
// block lanes (G is applied, never formed); the state lives in the AS part of the body's LDS (SchedLds).  Leaves the optimum in
// as_x (LDS); returns false on a breakdown (iteration cap, more than QMAX active constraints); `it` counts constraint additions.
// mu_of(block, row): friction coefficient of cone row `row` of the block (block = 4 k + leg; row_mu)
template <int H, int LG, class ApplyG, class MuOf>
__device__ __forceinline__ bool sched_active_set(double *lds, volatile double *gT, ApplyG &&apply_G, MuOf &&mu_of, const int tid, const bool enabled, const double lo, const double hi, int &it) {
  using LY = SchedLds<H, LG, true>;
  constexpr int NT = LY::NT, NV = LY::NV, QMAX = LY::QMAX, QLDS = LY::QLDS, GOFF = QLDS * (QLDS + 1) / 2, NB = 4 * H;
  double *as_x = lds + LY::as_x, *as_g = lds + LY::as_g, *as_z = lds + LY::as_z, *as_w = lds + LY::as_w, *as_lam = lds + LY::as_lam;
  double *as_sv = lds + LY::as_sv, *as_r = lds + LY::as_r, *as_v0 = lds + LY::as_v0, *as_v1 = lds + LY::as_v1, *as_T = lds + LY::as_T, *as_sc = lds + LY::as_sc;
  int *as_i0 = reinterpret_cast<int *>(lds + LY::as_int), *as_i1 = as_i0 + QMAX, *as_id = as_i1 + QMAX, *as_am = as_id + QMAX;
  // Packed symmetric T, row i = entries (i, 0..i).  Rows below QLDS are in LDS; the rows beyond -- a working set larger than
  // QLDS: forces on fz_min and a friction edge in nearly every block, seen for two robots of a 9000-seed sweep -- in the
  // workgroup's slab of global memory (gT; null where QLDS == QMAX).  Every loop below is written once per home so that the
  // LDS rows keep their ds_ instructions (the slab is accessed as volatile: merged into one loop over a pointer that is
  // LDS or global, the two homes cost every row a flat access -- and that merge does not survive this compiler's back end).
  constexpr bool SP = LY::SPILL > 0;   // (instantiations whose LDS holds every row carry no global-memory path at all)
  auto t_get = [&](const int i, const int j) -> double { if (!SP || i < QLDS) return as_T[i * (i + 1) / 2 + j]; return gT[i * (i + 1) / 2 - GOFF + j]; };   // i >= j
  auto t_put = [&](const int i, const int j, const double v) { if (!SP || i < QLDS) as_T[i * (i + 1) / 2 + j] = v; else gT[i * (i + 1) / 2 - GOFF + j] = v; };
  if (tid < NB) as_am[tid] = enabled ? 0 : 0x3F;   // a block that is not a variable has nothing to search
  for (int e = tid; e < NV; e += NT) { as_x[e] = 0.0; as_g[e] = 0.0; as_z[e] = 0.0; as_w[e] = 0.0; }
  __syncthreads();
  // x0 = -G q,  q = X qh  =>  G q = X (alpha I + K')^-1 qh
  apply_G(nullptr, as_x, true);
  if (enabled) { as_x[3 * tid] = -as_x[3 * tid]; as_x[3 * tid + 1] = -as_x[3 * tid + 1]; as_x[3 * tid + 2] = -as_x[3 * tid + 2]; }
  __syncthreads();
  double s_p = 0.0, lam_p = 0.0, sigma = 0.0, pv0 = 0.0, pv1 = 0.0;
  int q = 0, pid = -1, pi0 = 0, pi1 = 0, pblk = 0, pty = 0;
  const double vtol = 1e-9 * (1.0 + hi * 1e-3);
  const int it_cap = 8 * NV + 80;
  bool failed = false, need_search = true;
  for (int passes = 0;; passes++) {
    if (passes > it_cap) { failed = true; break; }
    if (need_search) {
      // --- most violated inactive constraint (wave 0) ---
      if (tid < 64) {
        double best = 0.0; int bid = -1;
        for (int blk2 = tid; blk2 < NB; blk2 += 64) {
          const int am = as_am[blk2];
          if (am == 0x3F) continue;
          const double fx = as_x[3 * blk2], fy = as_x[3 * blk2 + 1], fz = as_x[3 * blk2 + 2];
          const double sv6[6] = {-fx + mu_of(blk2, 0) * fz, fx + mu_of(blk2, 1) * fz, -fy + mu_of(blk2, 2) * fz, fy + mu_of(blk2, 3) * fz, fz - lo, hi - fz};
#pragma unroll
          for (int ty = 0; ty < 6; ty++) if (!((am >> ty) & 1) && sv6[ty] < best) { best = sv6[ty]; bid = 6 * blk2 + ty; }
        }
        const double bmin = wave_min_f64(best);
        const unsigned long long hit = __ballot(best == bmin && bid >= 0);
        bid = hit ? __builtin_amdgcn_readlane(bid, __ffsll((long long)hit) - 1) : -1;
        if (tid == 0) { as_sc[0] = bmin; as_sc[1] = (double)bid; }
      }
      __syncthreads();
      s_p = as_sc[0];
      pid = (int)as_sc[1];
      if (pid < 0 || s_p >= -vtol) break;
      if (q >= QMAX || (SP && q >= QLDS && gT == nullptr)) { failed = true; break; }   // no room left (cannot happen with the slab: a working set is linearly independent, <= NV rows): reported as a failure, never silent
      pblk = pid / 6; pty = pid % 6;
      pi0 = (pty < 2) ? 3 * pblk : (pty < 4 ? 3 * pblk + 1 : 3 * pblk + 2);
      pi1 = 3 * pblk + 2;
      pv0 = (pty == 0 || pty == 2 || pty == 5) ? -1.0 : 1.0;
      pv1 = (pty < 4) ? mu_of(pblk, pty) : 0.0;
      lam_p = 0.0;
      // g = G c_p
      if (tid == pblk) { as_w[3 * tid] = 0.0; as_w[3 * tid + 1] = 0.0; as_w[3 * tid + 2] = 0.0; as_w[pi0] += pv0; as_w[pi1] += pv1; }
      __syncthreads();
      apply_G(as_w, as_g, false);
      if (tid == pblk) { as_w[3 * tid] = 0.0; as_w[3 * tid + 1] = 0.0; as_w[3 * tid + 2] = 0.0; }
      sigma = pv0 * as_g[pi0] + pv1 * as_g[pi1];
      need_search = false;
      __syncthreads();
    }
    // sv = C_A g ; r = T sv (packed symmetric T, row k on lane k) ; w = c_p - C_A' r
    for (int k2 = tid; k2 < q; k2 += NT) as_sv[k2] = as_v0[k2] * as_g[as_i0[k2]] + as_v1[k2] * as_g[as_i1[k2]];
    __syncthreads();
    for (int k2 = tid; k2 < q; k2 += NT) {
      double rk = 0.0;
      const int base = k2 * (k2 + 1) / 2;
      if (!SP || k2 < QLDS) { for (int j = 0; j <= k2; j++) rk = fma(as_T[base + j], as_sv[j], rk); }
      else { const volatile double *Tg = gT + (base - GOFF); for (int j = 0; j <= k2; j++) rk = fma(Tg[j], as_sv[j], rk); }
      const int qa = (!SP || q < QLDS) ? q : QLDS;
      for (int j = k2 + 1; j < qa; j++) rk = fma(as_T[j * (j + 1) / 2 + k2], as_sv[j], rk);
      if constexpr (SP) { for (int j = (k2 + 1 > QLDS ? k2 + 1 : QLDS); j < q; j++) rk = fma(gT[j * (j + 1) / 2 - GOFF + k2], as_sv[j], rk); }
      as_r[k2] = rk;
    }
    if (tid == pblk) { as_w[pi0] += pv0; as_w[pi1] += pv1; }
    __syncthreads();
    for (int k2 = tid; k2 < q; k2 += NT) {
      const double rk = as_r[k2];
      atomicAdd(&as_w[as_i0[k2]], -rk * as_v0[k2]);
      if (as_v1[k2] != 0.0) atomicAdd(&as_w[as_i1[k2]], -rk * as_v1[k2]);
    }
    __syncthreads();
    apply_G(as_w, as_z, false);   // z = G (c_p - C_A' r)
    // clear w for the next pass (only entries of active blocks and of p's block were touched)
    if (enabled) { as_w[3 * tid] = 0.0; as_w[3 * tid + 1] = 0.0; as_w[3 * tid + 2] = 0.0; }
    // step lengths (dual bound t1 on wave 0)
    if (tid < 64) {
      double t1 = INFINITY; int lsel = -1;
      for (int kq = tid; kq < q; kq += 64) {
        const double rk = as_r[kq];
        if (rk > 0.0) { const double cand = as_lam[kq] / rk; if (cand < t1) { t1 = cand; lsel = kq; } }
      }
      const double tmin = wave_min_f64(t1);
      const unsigned long long hit = __ballot(t1 == tmin && lsel >= 0);
      lsel = hit ? __builtin_amdgcn_readlane(lsel, __ffsll((long long)hit) - 1) : -1;
      if (tid == 0) { as_sc[2] = tmin; as_sc[3] = (double)lsel; }
    }
    __syncthreads();
    const double dz = pv0 * as_z[pi0] + pv1 * as_z[pi1];   // c_p' z = sigma - sv' r  (>= 0)
    const double t1 = as_sc[2];
    const int lsel = (int)as_sc[3];
    const bool have_z = dz > 1e-13 * (1.0 + fabs(sigma));
    const double t2 = have_z ? -s_p / dz : INFINITY;
    const double tt = fmin(t1, t2);
    if (!(tt < INFINITY)) { failed = true; break; }
    if (have_z) {
      if (enabled) {
#pragma unroll
        for (int d = 0; d < 3; d++) as_x[3 * tid + d] = fma(tt, as_z[3 * tid + d], as_x[3 * tid + d]);
      }
      s_p = fma(tt, dz, s_p);
    }
    for (int k2 = tid; k2 < q; k2 += NT) as_lam[k2] -= tt * as_r[k2];
    lam_p += tt;
    const bool full = have_z && (t2 <= t1);
    __syncthreads();
    if (full) {
      // add p: T <- [[T + r r'/dz, -r/dz], [-r'/dz, 1/dz]]
      const double idz = 1.0 / dz;
      for (int i2 = tid; i2 < q; i2 += NT) {
        const double ri = as_r[i2] * idz;
        if (!SP || i2 < QLDS) { double *Trow = as_T + i2 * (i2 + 1) / 2; for (int j2 = 0; j2 <= i2; j2++) Trow[j2] = fma(ri, as_r[j2], Trow[j2]); }
        else { volatile double *Trow = gT + (i2 * (i2 + 1) / 2 - GOFF); for (int j2 = 0; j2 <= i2; j2++) Trow[j2] = fma(ri, as_r[j2], Trow[j2]); }
      }
      for (int k2 = tid; k2 < q; k2 += NT) t_put(q, k2, -as_r[k2] * idz);
      if (tid == 0) {
        t_put(q, q, idz);
        as_i0[q] = pi0; as_i1[q] = pi1; as_v0[q] = pv0; as_v1[q] = pv1; as_id[q] = pid; as_lam[q] = lam_p;
        as_am[pblk] |= 1 << pty;
      }
      q++;
      it++;
      need_search = true;
      __syncthreads();
    } else {
      // partial step: drop constraint l = lsel (its multiplier reached 0), keep working on p
      const int l = lsel, last = q - 1;
      const double itau = 1.0 / t_get(l, l);
      for (int k2 = tid; k2 < q; k2 += NT) as_sv[k2] = (k2 <= l) ? t_get(l, k2) : t_get(k2, l);   // column l
      __syncthreads();
      for (int i2 = tid; i2 < q; i2 += NT) {
        if (i2 == l) continue;
        const double ci = -as_sv[i2] * itau;
        if (!SP || i2 < QLDS) { double *Trow = as_T + i2 * (i2 + 1) / 2; for (int j2 = 0; j2 <= i2; j2++) Trow[j2] = fma(ci, as_sv[j2], Trow[j2]); }   // entries in row/column l are dead after the drop
        else { volatile double *Trow = gT + (i2 * (i2 + 1) / 2 - GOFF); for (int j2 = 0; j2 <= i2; j2++) Trow[j2] = fma(ci, as_sv[j2], Trow[j2]); }
      }
      __syncthreads();
      if (l != last) {   // move the last active constraint into slot l
        for (int k2 = tid; k2 < last; k2 += NT) {
          if (k2 == l) continue;
          const double v = t_get(last, k2);
          if (k2 < l) t_put(l, k2, v); else t_put(k2, l, v);
        }
        if (tid == 0) t_put(l, l, t_get(last, last));
      }
      if (tid == 0) {
        const int did = as_id[l];
        as_am[did / 6] &= ~(1 << (did % 6));
        if (l != last) { as_i0[l] = as_i0[last]; as_i1[l] = as_i1[last]; as_v0[l] = as_v0[last]; as_v1[l] = as_v1[last]; as_id[l] = as_id[last]; as_lam[l] = as_lam[last]; }
      }
      q--;
      __syncthreads();
      // g is unchanged (same p); the loop recomputes sv, r, w, z for the smaller active set
    }
  }
  return !failed;
}
template <int H, int LG, bool AS, bool MU4 = false>
__device__ __forceinline__ void qp_sched_robot(const DevCfg *__restrict__ c, const DevState &st, const DevOut &out, const int B, const int b,
                                               const double *tabN, const double *tabS, double *lds, const int mode = RG_QP_SOLVE) {
  // mode: RG_QP_SOLVE / RG_QP_RETRY / RG_QP_AUDIT (see qp_tile_robot)
  using LY = SchedLds<H, LG, AS>;
  constexpr int T = 8, TS = 10, NW = LY::NW, LC = LY::LC, NP = LY::NP, NT = LY::NT;
  static_assert(NP >= NW && 4 * H <= NT, "lane grid must cover the wrench problem and the (step, leg) blocks");
  // opaque copy: lane-role integers are recomputed per robot, not hoisted out of the caller's work loop
  const int tid = wg_lane<NT>();
  double *pbuf = lds + LY::pbuf, *vv = lds + LY::vv, *uv = lds + LY::uv, *Cm = lds + LY::Cm, *Ql = lds + LY::Ql, *Lk = lds + LY::Lk;
  double *LUr = lds + LY::LUr, *MVr = lds + LY::MVr, *Lik = lds + LY::Lik, *qw = lds + LY::qw, *qh = lds + LY::qh, *rec = lds + LY::rec;
  double *grf = lds + LY::grf, *zck = lds + LY::zck, *yst = lds + LY::yst, *yck = lds + LY::yck, *dyq = lds + LY::dyq, *sum3 = lds + LY::sum3;
  const double dt = c->dt;
  // (the lane roles of the iteration -- owner lane of a wrench row, block lane (horizon step, leg) -- and the projection
  // constants are derived after the sweep, inside the stage loop: see WrenchLane in rg_qp_wrench_kernel.inc)

  __syncthreads();
  for (int e = tid; e < RG_REC_N; e += NT) rec[e] = st.rec[(size_t)b * RG_REC_N + e];
  if (tid < 24) grf[tid] = 0.0;
  if (tid >= NW && tid < NP) vv[(tid >> 3) * TS + (tid & 7)] = 0.0;   // padding of the mat-vec input: never written again, must not hold NaN bits
  __syncthreads();
  const int sm0 = (int)rec[REC_SCHED], sm1 = (int)rec[REC_SCHED + 1], sm2 = (int)rec[REC_SCHED + 2], sm3 = (int)rec[REC_SCHED + 3];
  // block lane tid = (horizon step, leg): is the pair in contact (a variable of the QP)?
  auto lane_enabled = [&](const int t) { return (t >> 2) < H && ((((int)rec[REC_SCHED + (t & 3)]) >> (t >> 2)) & 1); };
  if (tid < 12) {   // C for all four legs, 6 x 12
    const int l = tid / 3, d = tid % 3;
    const double *rr = &rec[REC_FEETW + 3 * l];
    const double s0 = (d == 0) ? 0.0 : (d == 1 ? -rr[2] : rr[1]);
    const double s1 = (d == 0) ? rr[2] : (d == 1 ? 0.0 : -rr[0]);
    const double s2 = (d == 0) ? -rr[1] : (d == 1 ? rr[0] : 0.0);
    const double *Iw = &rec[REC_IWINV];
    Cm[tid] = Iw[0] * s0 + Iw[1] * s1 + Iw[2] * s2;
    Cm[12 + tid] = Iw[3] * s0 + Iw[4] * s1 + Iw[5] * s2;
    Cm[24 + tid] = Iw[6] * s0 + Iw[7] * s1 + Iw[8] * s2;
    Cm[36 + tid] = (d == 0) ? 1.0 : 0.0;
    Cm[48 + tid] = (d == 1) ? 1.0 : 0.0;
    Cm[60 + tid] = (d == 2) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < 144; e += NT) {   // per-leg C_l C_l'
    const int l = e / 36, ij = e - 36 * l, i = ij / 6, j = ij - 6 * i;
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < 3; d++) s = fma(Cm[i * 12 + 3 * l + d], Cm[j * 12 + 3 * l + d], s);
    Ql[e] = s;
  }
  // q_w(a) = 2 sum_{k >= a} [ dt g1(k) + (k - a + 1/2) dt^2 R6' g2(k) ]: does not depend on the contacts (see qp_wrench_robot)
  for (int e = tid; e < NW; e += NT) {
    const int a = e / 6, cc = e % 6;
    const double *om = &rec[REC_OMEGA], *vb = &rec[REC_VBODY], *cm = &rec[REC_CMD];
    const double icp = rec[REC_INVCP], tnp = rec[REC_TANP], yawr = tnp * om[0] + om[2] - cm[2];
    double p0, p1 = 0.0, r0 = 0.0, r1, r2 = 0.0;
    if (cc == 0) { p0 = c->w[6] * om[0]; r0 = icp * c->w[0] * rec[REC_ROLL]; r1 = icp * c->w[0] * icp * om[0] + tnp * c->w[2] * yawr; }
    else if (cc == 1) { p0 = c->w[7] * om[1]; r0 = c->w[1] * rec[REC_PITCH]; r1 = c->w[1] * om[1]; }
    else if (cc == 2) { p0 = c->w[8] * (om[2] - cm[2]); r1 = c->w[2] * yawr; }
    else if (cc < 5) { const double ev = vb[cc - 3] - cm[cc - 3]; p0 = c->w[9 + cc - 3] * ev * (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass); r1 = c->w[3 + cc - 3] * ev * (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass); }
    else {
      p0 = c->w[11] * vb[2] * (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass); p1 = -c->w[11] * c->g * (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass);
      r0 = c->w[5] * (rec[REC_COMZ] - (MU4 ? rec[REC_BODY + BODY_HEIGHT] : c->body_height)) * (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass); r1 = c->w[5] * vb[2] * (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass); r2 = -0.5 * c->w[5] * c->g * (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass);
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
  // ---- per-step factors: lane k < H does horizon step k ----
  if (tid < H) {
    const int k = tid;
    const int on0 = (sm0 >> k) & 1, on1 = (sm1 >> k) & 1, on2 = (sm2 >> k) & 1, on3 = (sm3 >> k) & 1;
    const int nck = on0 + on1 + on2 + on3;
    // Elimination order.  Coordinates: (torque x, y, z; force x, y, z).  One leg (rank 3) and three / four legs (rank 6): the
    // natural order -- the pivots that must be taken are O(0.01 .. 1) of their diagonal entries for any foot a leg can reach.
    // Two legs (rank 5): the null vector of C_k C_k' is (I_w n, r_1 x n) with n the direction of the line through the two
    // feet; the zero pivot lands on the coordinate eliminated LAST, and the other pivots are only as far from zero as that
    // coordinate's share of the null vector.  In the natural order that share is (r_1 x n)_z, the horizontal distance of
    // the centre of mass from the feet line: ~0 for every diagonal pair of a trot.  The torque coordinate along the larger
    // of |I_xx n_x|, |I_yy n_y| always carries a tenth of the vector or more (n is never vertical): it goes last.
    int plast = 5;
    if (nck == 2) {
      int la = -1, lb = -1;
#pragma unroll
      for (int l = 0; l < 4; l++) if ((l == 0 ? on0 : l == 1 ? on1 : l == 2 ? on2 : on3)) { if (la < 0) la = l; else lb = l; }
      const double nx = rec[REC_FEETW + 3 * lb] - rec[REC_FEETW + 3 * la], ny = rec[REC_FEETW + 3 * lb + 1] - rec[REC_FEETW + 3 * la + 1];
      plast = (fabs(nx) * rec[REC_IWINV + 4] > fabs(ny) * rec[REC_IWINV]) ? 0 : 1;   // |n_x| / Iw^-1_xx against |n_y| / Iw^-1_yy
    }
    auto phys = [&](const int pos) { return pos == 5 ? plast : (pos == plast ? 5 : pos); };   // coordinate at an elimination position
    double Q[6][6], L[6][6], Li[6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) {
        const int e = phys(i) * 6 + phys(j);
        Q[i][j] = (on0 ? Ql[e] : 0.0) + (on1 ? Ql[36 + e] : 0.0) + (on2 ? Ql[72 + e] : 0.0) + (on3 ? Ql[108 + e] : 0.0);
      }
    semidefinite_cholesky6(Q, nck == 0 ? 0 : (nck == 1 ? 3 : (nck == 2 ? 5 : 6)), L, Li);
    // stored with the ROWS back in coordinate order (a row-permuted triangular factor M_k, M_k M_k' = C_k C_k'): the weights
    // of the tile build go by coordinate; the columns stay in elimination order
#pragma unroll
    for (int r = 0; r < 6; r++) {
      Lik[k * 6 + r] = Li[r];
#pragma unroll
      for (int i = 0; i < 6; i++) Lk[k * 36 + phys(r) * 6 + i] = L[r][i];
    }
    Lik[6 * H + k] = (double)plast;
  }
  __syncthreads();
  for (int e = tid; e < NW; e += NT) {   // qh = L_a' q_w per step
    const int a = e / 6, cc = e - 6 * a;
    double s = 0.0;
    for (int r = 0; r < 6; r++) s = fma(Lk[a * 36 + r * 6 + cc], qw[a * 6 + r], s);   // (all rows: M_a is triangular only up to its row order)
    qh[e] = s;
  }
  const QpKernArgsP ka = reread_kernel_args();
  // (the robot's bounds for the ADMM iteration; the active-set form solves in the config's force units, see below)
  double zb[3] = {0.0, 0.0, lane_enabled(tid) ? ((MU4 && !AS) ? rec[REC_BODY + BODY_FZ_MIN] : c->fz_min) : 0.0};
  int it = 0;
  // ADMM runs in up to two stages with their own factorisation: rho first, and for the robots that have not converged
  // after admm_switch iterations rho2 (larger).  With a randomised schedule the iteration count is bimodal: nine robots
  // in ten converge in ~70 iterations at rho = 1e-4, the rest -- many constraints active in stiff directions -- take 300
  // to 1500 there but ~100 more at 4e-4 (where the easy ones would need 170).  The iterate carries over; the scaled
  // multiplier y = lambda / rho is rescaled.  Between stages z stays in zb and y is parked in ypark, both in registers (the
  // staging area of the next sweep goes over the vote state in LDS).
  double rho = AS ? 0.0 : c->rho * c->rho_sched_scale;   // first stage: admm_rho x admm_rho_sched_scale (the wrench-space iteration likes a lower rho, see qp_wrench_robot)
  int it_limit = (!AS && c->rho2 > 0.0 && c->admm_abs_tol > 0.0 && c->admm_switch < c->admm_iters) ? c->admm_switch : c->admm_iters;
  int next_chk = c->admm_check;
  bool converged = false;
  bool as_failed = false;   // exact solver broke down
  double ypark[3] = {0.0, 0.0, 0.0};   // ADMM form: the scaled multipliers between the two stages (z stays in zb)
  for (bool again = true; again;) {
  again = false;
  const double aa = uniform_f64(c->alpha + rho), inv_aa = uniform_f64(1.0 / aa), rho_aa = uniform_f64(rho * inv_aa);
  double tile[T][T];
  {   // tile build and sweep on their own copy of the lane index: (lr, lc) are not kept across the ADMM loop of the stage before
  const int ts = wg_lane<NT>();
  const int lr = ts >> LG, lc = ts & (LC - 1);
  // ---- scaled factor tables for the tile build (rebuilt per stage: their LDS is reused below for half of the Ch blocks) ----
  for (int e = ts; e < 6 * NP; e += NT) {
    const int r = e / NP, ki = e - r * NP;
    if (ki >= NW) { LUr[e] = 0.0; MVr[e] = 0.0; continue; }   // padding read by the tile build (the region is reused below, so every stage clears it)
    const int k = ki / 6, i = ki - 6 * k;
    const double im = (MU4 ? rec[REC_BODY + BODY_INV_MASS] : c->inv_mass);   // (MU4: plain LDS reads in this set-up -- as SGPR pairs they were kept across the solve)
    const double wu = r == 0 ? c->w[6] : r == 1 ? c->w[7] : r == 2 ? c->w[8] : r == 3 ? c->w[9] : r == 4 ? c->w[10] : c->w[11];
    const double wv = r == 0 ? c->w[0] : r == 1 ? c->w[1] : r == 2 ? c->w[2] : r == 3 ? c->w[3] : r == 4 ? c->w[4] : c->w[5];
    const double sc = r < 3 ? dt : im * dt;
    const double l = Lk[k * 36 + r * 6 + i], l0 = Lk[k * 36 + i];
    // rows of R6 L: (invcp L0, L1, tanp L0 + L2, L3, L4, L5)
    const double m = (r == 0) ? rec[REC_INVCP] * l0 : (r == 2 ? fma(rec[REC_TANP], l0, l) : l);
    LUr[e] = sqrt(wu) * sc * l;
    MVr[e] = sqrt(wv) * sc * dt * m;
  }
  __syncthreads();
  if constexpr (LY::SYM6) {
    // ---- every 6 x 6 block of a I + K' once: build (a lane below the block diagonal starts with the mirror image of its
    // block), symmetric sweep, move into the 8 x 8 tiles (rows in the reduce-scatter's order, diagonal offset removed) ----
    constexpr int NBS = LY::NBS;
    double X[6][6];
    int sbr, sbc;
    bool son;
    sym6_lane<NBS>(ts, sbr, sbc, son);
    sym6_build_sched<H, NP>(X, tabN, tabS, LUr, MVr, sbc, sbr, son, aa);
    sym6_sweep<NBS, NBS, NT>(X, pbuf, sbr, sbc, son);
    sym6_to_tile8<NBS, NBS, LG, NT>(X, sbr, sbc, son, tile, lds + LY::stage, ts);
    __syncthreads();
    if (ts >= NW && ts < NP) vv[(ts >> 3) * TS + (ts & 7)] = 0.0;   // padding of the mat-vec input (the staging area went over it): must not hold NaN bits
  } else {
  // ---- my 8 x 8 tile of a I + K' (identity in the padding), swept to -(a I + K')^-1 ----
  build_tile_sched<H, NP>(tile, tabN, tabS, LUr, MVr, lr, lc, NW, aa);
  tile_sweep<8, LG, NW>(tile, pbuf, lr, lc);
  if (lr == lc) {   // remove the sweep's +2 diagonal offset
#pragma unroll
    for (int ta = 0; ta < T; ta++) tile[ta][ta] -= 2.0;
  }
  permute_tile_rows_for_reduce(tile, lc);
  }
  }
  // lane roles of the iteration and the projection constants, from a fresh lane index (WrenchLane): nothing of them is live
  // -- spilled -- across the sweep
  const int tid = wg_lane<NT>();
  const WrenchLane<H, LG> L(tid);
  const int io = L.io, iov_pad = L.iov_pad, bk = L.bk, bj = L.bj, b0 = L.b0, b1 = L.b1, rA = L.rA, rB = L.rB, padA = L.padA, padB = L.padB;
  const int ubase0 = L.ubase0, ubase1 = L.ubase1;
  const bool own_real = L.own_real, quad_real = L.quad_real, enabled = lane_enabled(tid);
  const int lr = tid >> LG, lc = tid & (LC - 1);
  const double relax = c->relax, lo = (MU4 && !AS) ? body_val<MU4>(c, rec, BODY_FZ_MIN) : c->fz_min, hi = (MU4 && !AS) ? body_val<MU4>(c, rec, BODY_FZ_MAX) : c->fz_max;
  const double mu = leg_mu<MU4>(c, rec, bj);   // this block lane's leg (block = 4 k + leg): one scalar unless MU4
  const double kA = 1.0 / (1.0 + 2.0 * mu * mu), kB = 1.0 / (1.0 + mu * mu);
  // ---- block-lane state: Ch block = L_k^+ C_leg by forward substitution (zero pivots give zero rows) ----
  // Lanes with b0 = 1 hold the rows rotated by three (see qp_wrench_robot).
  // Rows 0..2 (in the lane's order) stay in registers; rows 3..5 go to LDS, [9][4 H] in the factor tables that are dead after
  // the tile build: with all eighteen in VGPRs the ADMM loop spilled (12 scratch reloads per iteration, 450 MB of HBM
  // traffic per config-5 launch); the LDS pipe is the idle one in this body (19 % busy).
  double Cb[3][3];
  double *cbs = LUr;                      // 9 * 4 H doubles <= the 12 * NP of LUr + MVr
  static_assert(9 * 4 * H <= 12 * NP, "Ch half-blocks fit the dead factor tables");
  const int slot = quad_real ? tid : 0;   // lanes that are no block lane read lane 0's entries; their results are never used
  {
    double y[6][3];
    const int kk = quad_real ? bk : 0;
    const int plast = (int)Lik[6 * H + kk];   // forward substitution in the step's elimination order (rows of M_k by coordinate)
#pragma unroll
    for (int r = 0; r < 6; r++) {
      const double li = Lik[kk * 6 + r];
      const int row = r == 5 ? plast : (r == plast ? 5 : r);
#pragma unroll
      for (int d = 0; d < 3; d++) {
        double t = Cm[row * 12 + 3 * bj + d];
#pragma unroll
        for (int m = 0; m < r; m++) t = fma(-Lk[kk * 36 + row * 6 + m], y[m][d], t);
        y[r][d] = t * li;
      }
    }
    __syncthreads();   // every lane is done reading LUr / MVr (tile build) and Lk before the table is overwritten
#pragma unroll
    for (int cc = 0; cc < 3; cc++)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const double lo3 = y[cc][d], hi3 = y[cc + 3][d];
        Cb[cc][d] = enabled ? (b0 ? hi3 : lo3) : 0.0;
        if (quad_real) cbs[(cc * 3 + d) * (4 * H) + tid] = enabled ? (b0 ? lo3 : hi3) : 0.0;
      }
  }
  auto cb_hi = [&](int cc, int d) { return cbs[((cc - 3) * 3 + d) * (4 * H) + slot]; };   // rows 3..5, own slot: no barrier needed
  if constexpr (!AS) {
    // ================= over-relaxed ADMM (same iteration as qp_wrench_robot) =================
    double yb[3] = {ypark[0], ypark[1], ypark[2]};
    zck[tid] = zb[0]; zck[NT + tid] = zb[1]; zck[2 * NT + tid] = zb[2];   // the forces at the "previous vote" of the stage's first window
    // the same movement of z means a dual residual rho times as large: the second stage (rho2 > rho) tests proportionally
    // tighter, so both stages stop at the same stationarity error (a seeded configuration sweep found a stage-2 robot
    // stopping 5x farther from the optimum than stage-1 robots do)
    const double tsc = uniform_f64(rho > c->rho ? c->rho / rho : 1.0);   // (a first stage below admm_rho keeps the nominal tolerance)
    const double atol = c->admm_abs_tol * tsc, ptol = c->admm_prim_tol * tsc;
    const int chk = c->admm_check;
    const double etol = c->admm_extrap * atol;
    yst[tid] = INFINITY; yst[NT + tid] = INFINITY; yst[2 * NT + tid] = INFINITY;   // between stage switches yst holds the previous window's movement
    yck[tid] = yb[0]; yck[NT + tid] = yb[1]; yck[2 * NT + tid] = yb[2];
    dyq[tid] = 0.0; dyq[NT + tid] = 0.0; dyq[2 * NT + tid] = 0.0;
    if (tid == 0) { sum3[12] = 0.0; sum3[13] = 0.0; sum3[14] = inv_aa; }   // [12] largest extrapolation gain applied in this stage, [13] remaining_distance_factor of the last vote (see qp_tile_robot)
    // [14]: 1 / (alpha + rho) for the iteration loop, read back from LDS every iteration: kept in a register pair across this
    // loop it was the value the allocator spilled (a scratch reload per iteration, in front of the fma that needs it)
    // valid windows of displacement history before the current one (0 at the stage start and right after an extrapolation):
    // the rate estimate and a jump need one; the vote right after a jump cannot pass
    int hist = 0;
    it = __builtin_amdgcn_readfirstlane(it);   // wave-uniform: keep the loop control scalar (see qp_tile_robot)
    const int it_end = __builtin_amdgcn_readfirstlane(it_limit);
    for (; it < it_end; it++) {
      const double d0 = zb[0] - yb[0], d1 = zb[1] - yb[1], d2 = zb[2] - yb[2];
      double cw[6];
#pragma unroll
      for (int cc = 0; cc < 3; cc++) cw[cc] = fma(Cb[cc][2], d2, fma(Cb[cc][1], d1, Cb[cc][0] * d0));
#pragma unroll
      for (int cc = 3; cc < 6; cc++) cw[cc] = fma(cb_hi(cc, 2), d2, fma(cb_hi(cc, 1), d1, cb_hi(cc, 0) * d0));
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
      const double tw = tile8_matvec<LG>(tile, vv, lr, lc);   // (a I + K')^-1 w
      if (own_real) uv[io] = fma(-(vv[iov_pad] + qh[io]), sum3[14], tw);
      __syncthreads();
      double pres = 0.0;
      const bool vote_now = atol > 0.0 && it + 1 == next_chk;   // uniform
      if (enabled) {
        const double u6[6] = {uv[ubase0], uv[ubase0 + 1], uv[ubase0 + 2], uv[ubase1], uv[ubase1 + 1], uv[ubase1 + 2]};
        double x[3] = {rho_aa * d0, rho_aa * d1, rho_aa * d2};
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
#pragma unroll
          for (int d = 0; d < 3; d++) x[d] = fma(Cb[cc][d], u6[cc], x[d]);
        }
#pragma unroll
        for (int cc = 3; cc < 6; cc++) {
#pragma unroll
          for (int d = 0; d < 3; d++) x[d] = fma(cb_hi(cc, d), u6[cc], x[d]);
        }
        const double w0 = relax * x[0] + (1.0 - relax) * zb[0] + yb[0];
        const double w1 = relax * x[1] + (1.0 - relax) * zb[1] + yb[1];
        const double w2 = relax * x[2] + (1.0 - relax) * zb[2] + yb[2];
        double px, py, pz;
        proj_pyramid(w0, w1, w2, mu, lo, hi, kA, kB, px, py, pz);
        if (vote_now) pres = fmax(fmax(fabs(x[0] - px), fabs(x[1] - py)), fabs(x[2] - pz));   // primal residual |x - z|
        yb[0] = w0 - px; yb[1] = w1 - py; yb[2] = w2 - pz;
        zb[0] = px; zb[1] = py; zb[2] = pz;
      }
      if (vote_now) {
        next_chk += chk;
        if (wrench_admm_vote<NT>(c, tid, enabled, zb, yb, zck, yst, yck, dyq, sum3, pres, atol, etol, ptol, it, hist)) { it++; converged = true; break; }
      }
    }
    if (!converged && atol > 0.0 && it < c->admm_iters) {   // second stage: re-factorise with rho2 and carry the iterate over
      const double sc = rho / c->rho2;
      ypark[0] = yb[0] * sc; ypark[1] = yb[1] * sc; ypark[2] = yb[2] * sc;   // (registers: the staging area of the next sweep goes over the vote state)
      rho = c->rho2;
      it_limit = c->admm_iters;
      again = true;
      __syncthreads();
      continue;
    }
    if (tid == 0) {
      if (c->solver == RG_SOLVER_AUTO && atol > 0.0 && !converged) {   // hand the robot to the exact solver (list of the four-leg bin)
        const int slot = atomicAdd(&ka->st.counts[8 + 4], 1);
        ka->st.bins[(size_t)(5 + 4) * ka->B + slot] = b;
      } else if (atol > 0.0 && !converged) atomicAdd(&ka->st.counts[7], 1);   // RG_SOLVER_ADMM: a failure
      ka->st.iters[b] = it;
    }
  } else {
    // ================= exact dual active-set method (range-space form) on G = P^-1 = I / alpha + X M X' =================
    // Same method and constraint numbering as the force-space body in rg_qp_exact_kernel.inc (id = 6 * block + type), with
    // block = (step, leg) lane index 4 k + j and variable index 3 * block + axis.  G is applied, never formed:
    //   G w = w / alpha + X [ (alpha I + K')^-1 - I / alpha ] X' w   -- the ADMM iteration's linear algebra with rho = 0.
    double *as_x = lds + LY::as_x;   // the solver's state lives in the AS part of this body's LDS (SchedLds); it leaves the optimum here
    // out[3 * block + d] = (G in)[...] on the enabled block lanes; `in` is read from LDS (NV doubles, indexed by variable)
    auto apply_G = [&](const double *in, double *outv, const bool in_is_qh) {
      if (!in_is_qh) {
        const double d0 = enabled ? in[3 * tid] : 0.0, d1 = enabled ? in[3 * tid + 1] : 0.0, d2 = enabled ? in[3 * tid + 2] : 0.0;
        double cw[6];
#pragma unroll
        for (int cc = 0; cc < 3; cc++) cw[cc] = fma(Cb[cc][2], d2, fma(Cb[cc][1], d1, Cb[cc][0] * d0));
#pragma unroll
        for (int cc = 3; cc < 6; cc++) cw[cc] = fma(cb_hi(cc, 2), d2, fma(cb_hi(cc, 1), d1, cb_hi(cc, 0) * d0));
        double keep[3];
#pragma unroll
        for (int h2 = 0; h2 < 3; h2++) keep[h2] = cw[h2] + dpp_f64<0xB1>(cw[3 + h2]);
#pragma unroll
        for (int h2 = 0; h2 < 3; h2++) keep[h2] += dpp_f64<0x4E>(keep[h2]);
        if (quad_real) {
          vv[padA] = b1 ? keep[2] : keep[0];
          if (!b1) vv[padB] = keep[1];
        }
      } else if (own_real) vv[iov_pad] = qh[io];
      __syncthreads();
      const double tw = tile8_matvec<LG>(tile, vv, lr, lc);
      if (own_real) uv[io] = in_is_qh ? tw : fma(-vv[iov_pad], inv_aa, tw);
      __syncthreads();
      if (enabled) {
        const double u6[6] = {uv[ubase0], uv[ubase0 + 1], uv[ubase0 + 2], uv[ubase1], uv[ubase1 + 1], uv[ubase1 + 2]};
        double x[3];
#pragma unroll
        for (int d = 0; d < 3; d++) x[d] = in_is_qh ? 0.0 : in[3 * tid + d] * inv_aa;
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
#pragma unroll
          for (int d = 0; d < 3; d++) x[d] = fma(Cb[cc][d], u6[cc], x[d]);
        }
#pragma unroll
        for (int cc = 3; cc < 6; cc++) {
#pragma unroll
          for (int d = 0; d < 3; d++) x[d] = fma(cb_hi(cc, d), u6[cc], x[d]);
        }
        outv[3 * tid] = x[0]; outv[3 * tid + 1] = x[1]; outv[3 * tid + 2] = x[2];
      }
      __syncthreads();
    };
    auto mu_of = [&](const int blk, const int ty) -> double { return row_mu<MU4>(c, rec, blk & 3, ty); };
    // rows of the packed inverse beyond the LDS part: this workgroup's slab (the audit launch, which may run beside a re-solve launch, has its own range)
    double *gT = (LY::SPILL > 0 && c->as_spill) ? c->as_spill + (size_t)((int)blockIdx.x + (mode == RG_QP_AUDIT ? c->as_spill_audit_base : 0)) * LY::SPILL : nullptr;
    bool as_ok;
    if constexpr (MU4) {
      // The robot's own mass m_b, solved in the config's force units: with f = k f~, k = m_b / m (config mass), the normal-force
      // bounds scale * m_b * g become the config's (lo, hi: the config's in the AS instantiations), the friction cone is unchanged,
      // and the minimiser of 1/2 f'Pf + q'f is k times that of 1/2 f~'Pf~ + (q / k)'f~.  So q (qh, LDS) is scaled by 1 / k before
      // the solve and the solution (as_x, LDS) by k after it: no per-robot value is live across the active-set loop, which sits
      // at the register limit of the re-solve kernels.
      { const double kinv = c->mass * rec[REC_BODY + BODY_INV_MASS]; for (int e = tid; e < NW; e += NT) qh[e] *= kinv; }
      __syncthreads();
      as_ok = sched_active_set<H, LG>(lds, gT, apply_G, mu_of, tid, enabled, lo, hi, it);
      { const double k = 1.0 / (c->mass * rec[REC_BODY + BODY_INV_MASS]); for (int e = tid; e < LY::NV; e += NT) as_x[e] *= k; }
      __syncthreads();
    }
    else as_ok = sched_active_set<H, LG>(lds, gT, apply_G, mu_of, tid, enabled, lo, hi, it);
    const bool failed = !as_ok;
    if (failed && tid == 0 && mode != RG_QP_AUDIT) atomicAdd(&ka->st.counts[7], 1);
    as_failed = failed;
    if (enabled) { zb[0] = as_x[3 * tid]; zb[1] = as_x[3 * tid + 1]; zb[2] = as_x[3 * tid + 2]; }
    if (tid == 0 && mode != RG_QP_AUDIT) ka->st.iters[b] = mode == RG_QP_RETRY ? ka->st.iters[b] + it : it;
    // the front kernel's direct routing (horizon 10, constant contacts): marked while the exact solver has to solve this robot
    if (tid == 0 && mode != RG_QP_AUDIT && H == 10) ka->st.hard[b] = failed ? 0 : (int)rec[REC_CONTACT] + 1;
  }
  }   // stage loop
  // ---- epilogue: first-step forces (negated), tau = J' f * MOTOR_DIRECTION, merge with the swing tuples ----
  {
    const int te = wg_lane<NT>();   // block lane (step 0, leg te)
    if (te < 4 && lane_enabled(te)) { grf[3 * te] = -zb[0]; grf[3 * te + 1] = -zb[1]; grf[3 * te + 2] = -zb[2]; }
  }
  __syncthreads();
  if constexpr (!AS) audit_capture<NT>(converged, b, 4, rec, grf);
  qp_write_outputs<NT>(c, rec, grf, b, tid, mode);
  if (AS && mode == RG_QP_AUDIT) audit_compare(c, rec, grf, b, as_failed);
}

// One launch for every robot with a stance leg (all of them run this body under a contact schedule); work order =
// the front kernel's cost classes, most expensive first, like rg_qp_fused_kernel.
template <int H, int MINW, bool MU4 = false>
__global__ void __launch_bounds__((1 << FusedShape<H>::LG) * (1 << FusedShape<H>::LG), MINW)
rg_qp_sched_kernel(const DevCfg *__restrict__ c, DevState st, DevOut out, int B) {
  constexpr int LG = FusedShape<H>::LG, NT = (1 << LG) * (1 << LG);
  const int wg = (int)blockIdx.x;
  double *tabN = smem, *tabS = smem + H * H, *lds = smem + 2 * H * H;
  // workgroups beyond the batch: the swing-leg IK lanes of this tick (rg_front_kernel.inc: swing_ik_lane), dispatched last
  if (wg >= B) { swing_ik_lane(c, st, out, B, (wg - B) * NT + (int)threadIdx.x); return; }
  stamp_start();
  check_kernel_args(c, B);
  load_horizon_tables<H>(c, tabN, tabS, wg_lane<NT>(), NT);
  // one work item per workgroup (the grid is the batch), no work loop: see rg_qp_fused_kernel
  const int work = wg;
  int cls = 0, first = 0, run = 0;
#pragma unroll
  for (int k = 0; k < RG_COST_CLASSES; k++) { const int n = st.counts[16 + k]; if (k > 0 && work >= run) { cls = k; first = run; } run += n; }
  if (work >= run) return;
  const int entry = __builtin_amdgcn_readfirstlane(st.bins[(size_t)(10 + cls) * B + (work - first)]);
  qp_sched_robot<H, LG, false, MU4>(c, st, out, B, entry & 0xFFFFFF, tabN, tabS, lds);
}

template <int H, bool MU4>
static hipError_t launch_qp_sched(const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, hipStream_t s) {
  constexpr int LG = FusedShape<H>::LG, NT = (1 << LG) * (1 << LG);
  const size_t lds = sizeof(double) * (qp_sched_lds_doubles<H, LG, false>() + 2 * H * H);
  static_assert(sizeof(double) * (qp_sched_lds_doubles<H, LG, false>() + 2 * H * H) <= 80 * 1024, "two 256-lane workgroups per CU at horizon 20");
  static bool attr_done[64] = {};
  if (lds > 64 * 1024 && lds_attr_needed(attr_done)) {
    hipError_t e = hipFuncSetAttribute((const void *)rg_qp_sched_kernel<H, 2, MU4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  RG_CHECK_KERNARGS(rg_qp_sched_kernel<H, 2, MU4>);
  rg_qp_sched_kernel<H, 2, MU4><<<dim3(B + (4 * B + NT - 1) / NT), dim3(NT), lds, s>>>(dcfg, st, dout, B);   // one workgroup per robot, then the swing IK lanes
  return hipGetLastError();
}

static hipError_t launch_qp_sched_any(int H, bool mu4, const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, hipStream_t s) {
  if (H == 10) return mu4 ? launch_qp_sched<10, true>(dcfg, st, dout, B, s) : launch_qp_sched<10, false>(dcfg, st, dout, B, s);
  if (H == 20) return mu4 ? launch_qp_sched<20, true>(dcfg, st, dout, B, s) : launch_qp_sched<20, false>(dcfg, st, dout, B, s);
  return hipErrorInvalidValue;
}

// Exact re-solves at horizon 20 (RG_SOLVER_AUTO), one launch over three lists -- like rg_qp_resolve_kernel at horizon 10,
// normally empty -- and ONE body: the wrench-space active-set body of the schedule QP, which handles any set of (step, leg)
// pairs in contact and therefore every stance-leg count: (list 9) robots of the schedule body -- any contact schedule, and
// three / four legs with constant contacts; (lists 7, 6) two- and one-leg robots of the force-space ADMM body, whose per-leg
// schedule words the front kernel writes as all-ones / zero.  (Round 3 inlined two more 256-lane force-space bodies for those
// two lists: 256 VGPRs + 81 AGPRs of spill space; see rg_qp_resolve_kernel.)
template <int H, bool MU4 = false>
__global__ void __launch_bounds__(256, 1)
rg_qp_sched_retry_kernel(const DevCfg *__restrict__ c, DevState st, DevOut out, int B, const int audit) {
  static_assert(FusedShape<H>::LG == 4, "256-lane bodies");
  // list 9 (counter 12) takes every robot of the schedule body, three- and four-leg ones alike; list 8 (counter 11, the
  // three-leg list of the horizon-10 plan) is never written at this horizon
  const int rs = st.counts[12], r2 = st.counts[10], r1 = st.counts[9];
  int total = rs + r2 + r1;
  if (audit) { total = st.audit_cnt[st.audit_ring]; total = total < RG_AUDIT_SLOTS ? total : RG_AUDIT_SLOTS; }   // audit lane, see rg_qp_resolve_kernel
  if ((int)blockIdx.x >= total) return;   // the usual case: nothing to re-solve
  double *tabN = smem, *tabS = smem + H * H, *lds = smem + 2 * H * H;
  check_kernel_args(c, B);
  load_horizon_tables<H>(c, tabN, tabS, threadIdx.x, 256);
  const int mode = audit ? RG_QP_AUDIT : RG_QP_RETRY;
  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    // (each work item's own view of the arguments, through the opaque kernarg pointer: see rg_qp_resolve_kernel)
    const QpKernArgsP ka = reread_kernel_args();
    const DevCfg *c = ka->c;
    DevState sw = *(const DevState *)&ka->st;
    if (audit) sw.rec = sw.audit_rec + (size_t)sw.audit_ring * RG_AUDIT_SLOTS * RG_REC_N;
    int idx;
    if (audit) idx = work;
    else {
      int w = work;
      if (w < rs) idx = st.bins[(size_t)9 * B + w];
      else if ((w -= rs) < r2) idx = st.bins[(size_t)7 * B + w];
      else idx = st.bins[(size_t)6 * B + (w - r2)];
    }
    qp_sched_robot<H, 4, true, MU4>(c, sw, out, B, idx, tabN, tabS, lds, mode);
  }
}

// Workgroups of the horizon-20 re-solve launch (audit: of its audit-lane form, with `audit_k` expected picks).  rg_mpc_create
// sizes the per-workgroup slabs of DevCfg::as_spill with the same rule.
static int sched_retry_grid(const int cu_count, const int B, const bool audit, const int audit_k) {
  int grid = cu_count;   // one large-LDS workgroup per CU
  if (grid > B) grid = B;
  if (audit) { grid = audit_k + audit_k / 4; if (grid > RG_AUDIT_SLOTS) grid = RG_AUDIT_SLOTS; }
  return grid < 1 ? 1 : grid;
}
template <bool MU4>
static hipError_t launch_qp_sched_retry_h20_impl(const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, int cu_count, hipStream_t s, int audit) {
  constexpr int H = 20;
  const size_t lds = sizeof(double) * (qp_sched_lds_doubles<H, 4, true>() + 2 * H * H);
  static_assert(sizeof(double) * (qp_sched_lds_doubles<H, 4, true>() + 2 * H * H) <= 160 * 1024, "active-set state must fit the CU's LDS");
  static bool attr_done[64] = {};
  if (lds_attr_needed(attr_done)) {
    hipError_t e = hipFuncSetAttribute((const void *)rg_qp_sched_retry_kernel<H, MU4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int grid = sched_retry_grid(cu_count, B, audit != 0, st.audit_k);
  RG_CHECK_KERNARGS(rg_qp_sched_retry_kernel<H, MU4>);
  rg_qp_sched_retry_kernel<H, MU4><<<dim3(grid), dim3(256), lds, s>>>(dcfg, st, dout, B, audit);
  return hipGetLastError();
}
static hipError_t launch_qp_sched_retry_h20(bool mu4, const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, int cu_count, hipStream_t s, int audit) {
  return mu4 ? launch_qp_sched_retry_h20_impl<true>(dcfg, st, dout, B, cu_count, s, audit) : launch_qp_sched_retry_h20_impl<false>(dcfg, st, dout, B, cu_count, s, audit);
}
