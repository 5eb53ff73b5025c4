// rg_qp_exact_kernel.inc -- exact QP bodies: dual active-set method on one wave, warm-started from the robot's working set of
// the previous tick.  Force space for one and two stance legs, wrench space for three and four.
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// ------------------------------------------------------------------------------------
// What the reference's default solver computes is the EXACT minimiser (mpc_controller.py:47-56 passes no solver: upstream
// qpOASES, an online active-set method).  On the bench workload a trot robot's QP (60 variables, 120 inequality rows) has
// one or two active constraints at the optimum (mean 1.6, p90 3) and a four-leg robot's ~11 (p90 25, largest seen 39), and
// the set is the same as in the tick before for 85 % / 50 % of the robots (tests/studies/gi_model.py) -- an active-set method
// needs a handful of steps where the friction-cone ADMM needs ~50 iterations, and it ends AT the optimum: no stopping rule to
// tune, nothing to audit.
//
// Method: Goldfarb-Idnani dual active set in range-space form on G = P^-1 (explicit in force space: the same in-register
// symmetric sweep as the ADMM body, swept with rho = 0; applied through the wrench-space identity for three and four legs).
// With A the working set (q rows C_A, right-hand sides b_A):
//     x = x0 + G C_A' lambda,   x0 = -G q,   T = (C_A G C_A')^-1  (LDS, row k on lane k).
// Adding the most violated constraint p:  d = G c_p,  sv = C_A d,  r = T sv,  dz = c_p'd - sv'r  (the Schur complement);
// step lengths t1 = min lambda_k / r_k over r_k > 0 (dual feasibility) and t2 = -s_p / dz (constraint p becomes active);
// a partial step drops the blocking constraint (rank-1 downdate of T) and repeats with the same d, a full step borders T
// with (r, dz).  The primal iterate is NOT updated per partial step: only the multipliers are, and x is recomputed from
// them once per added constraint -- two applications of G per iteration, whatever happens in between.
// Warm start: the constraints of the stored working set are added as equalities (one application of G each; linearly
// dependent ones are skipped), the multipliers of that equality-constrained minimiser follow from T, and constraints with a
// negative multiplier are dropped one at a time until none is left: (x, A) is then a valid start (x minimises over A as
// equalities, lambda >= 0) and the method continues from there.
//
// One wave per robot.  Per-constraint state (id, multiplier) lives on lane k < q, the active-type mask of force block b on
// lane b; vectors (x0, x, d) and the dense multiplier table live in LDS.  All synchronisation is wave-level (a one-wave
// workgroup's barrier is a scheduling fence).  Variable index = 3 * block + axis, constraint id = 6 * block + type on the
// 3-vector (fx, fy, fz) of a (horizon step, stance leg) block:
//     0: -fx + mu fz >= 0    1: fx + mu fz >= 0    2: -fy + mu fz >= 0    3: fy + mu fz >= 0    4: fz >= lo    5: -fz >= -hi
// The body's cost unit is one application of G (~1.1 us alone, ~1.6 us with two waves per SIMD): st.iters reports their
// number and the front kernel predicts the robot's cost class from it.
// ------------------------------------------------------------------------------------

// per-robot working-set store: RG_WS_MAX constraint ids (one byte each: ids < 6 * 40) and the count
#define RG_WS_MAX 64

struct ExactCon { int i0, i1; double v0, v1, rhs; };
__device__ __forceinline__ ExactCon exact_constraint(const int id, const double mu, const double lo, const double hi) {
  const int blk = id / 6, ty = id - 6 * blk;
  ExactCon k;
  k.i0 = 3 * blk + (ty < 2 ? 0 : (ty < 4 ? 1 : 2));
  k.i1 = 3 * blk + 2;
  k.v0 = (ty == 0 || ty == 2 || ty == 5) ? -1.0 : 1.0;
  k.v1 = ty < 4 ? mu : 0.0;
  k.rhs = ty == 4 ? lo : (ty == 5 ? -hi : 0.0);
  return k;
}
__device__ __forceinline__ double readlane_f64(const double v, const int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// ---- T = (C_A G C_A')^-1 in LDS, row k on lane k < q ----
// Row loops walk a row in groups of 8 (q rounded up: everything outside the q x q block is kept at zero), the second operand
// being a per-slot vector in LDS read at a uniform address (broadcast): every load of a group is independent of the others,
// so a row costs one LDS latency, not one per entry.  (The first version looped over readlane + one 8-byte read per entry:
// ~130 cycles each, 10 k cycles per constraint at q = 40 -- robots with large working sets were the launch's tail.)
//   PACKED = false: full symmetric storage, row stride QS = Q + 2 (even: 16-byte row starts; 2 QS mod 64 banks spreads 16
//                   rows over all banks): rows are contiguous, 16-byte loads.  Q x QS doubles.
//   PACKED = true:  lower triangle, entry (k, j <= k) at k (k + 1) / 2 + j: half the LDS (what lets the wrench-space body,
//                   which needs room for ~48 constraints, keep eight workgroups per CU); the part of a row right of the
//                   diagonal is read down a column (8-byte loads), updates touch only the stored triangle.
template <int Q, bool PACKED>
struct ExactT {
  static constexpr int QS = Q + 2;
  static constexpr int doubles = PACKED ? ((Q * (Q + 1) / 2 + 1) & ~1) : Q * QS;
  static __device__ __forceinline__ int tri(const int k) { return k * (k + 1) / 2; }
  static __device__ __forceinline__ int at(const int k, const int j) {   // entry (k, j) of the symmetric matrix
    if constexpr (PACKED) return k >= j ? tri(k) + j : tri(j) + k;
    else return k * QS + j;
  }
  // r_k = sum_j T[k][j] s_j on lane k < q (s zero beyond q), 0 elsewhere
  static __device__ __forceinline__ double row_dot(const double *Tm, const double *s, const int lane, const int q) {
    double r0 = 0.0, r1 = 0.0;
    if (lane < q) {
      for (int j = 0; j < q; j += 8) {
        double t[8];
        if constexpr (PACKED) {
#pragma unroll
          for (int e = 0; e < 8; e++) t[e] = Tm[at(lane, j + e)];
        } else {
#pragma unroll
          for (int e = 0; e < 8; e += 2) { const double2 v = *reinterpret_cast<const double2 *>(Tm + lane * QS + j + e); t[e] = v.x; t[e + 1] = v.y; }
        }
        const double2 s0 = *reinterpret_cast<const double2 *>(s + j), s1 = *reinterpret_cast<const double2 *>(s + j + 2);
        const double2 s2 = *reinterpret_cast<const double2 *>(s + j + 4), s3 = *reinterpret_cast<const double2 *>(s + j + 6);
        r0 = fma(t[0], s0.x, r0); r1 = fma(t[1], s0.y, r1); r0 = fma(t[2], s1.x, r0); r1 = fma(t[3], s1.y, r1);
        r0 = fma(t[4], s2.x, r0); r1 = fma(t[5], s2.y, r1); r0 = fma(t[6], s3.x, r0); r1 = fma(t[7], s3.y, r1);
      }
    }
    return r0 + r1;
  }
  // T[k][.] += a_k v' on the lanes k < q that take part (v zero beyond q)
  static __device__ __forceinline__ void rank1(double *Tm, const double *v, const int lane, const int q, const double ak, const bool take) {
    if (lane < q && take) {
      for (int j = 0; j < q; j += 8) {
        const double2 v0 = *reinterpret_cast<const double2 *>(v + j), v1 = *reinterpret_cast<const double2 *>(v + j + 2);
        const double2 v2 = *reinterpret_cast<const double2 *>(v + j + 4), v3 = *reinterpret_cast<const double2 *>(v + j + 6);
        const double vs[8] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, v3.x, v3.y};
        if constexpr (PACKED) {
          double *row = Tm + tri(lane) + j;
          double t[8];
#pragma unroll
          for (int e = 0; e < 8; e++) t[e] = (j + e <= lane) ? row[e] : 0.0;
#pragma unroll
          for (int e = 0; e < 8; e++) if (j + e <= lane) row[e] = fma(ak, vs[e], t[e]);
        } else {
          double *row = Tm + lane * QS + j;
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            double2 t = *reinterpret_cast<const double2 *>(row + e);
            t.x = fma(ak, vs[e], t.x); t.y = fma(ak, vs[e + 1], t.y);
            *reinterpret_cast<double2 *>(row + e) = t;
          }
        }
      }
    }
  }
};

// The solve.  In: T / sv / rv / lamc zeroed; `blk_on`: this lane is a block lane whose block is a variable (its six constraints
// are searched).  column_of_G(p, dq) -> sigma = c_p' G c_p with d = G c_p left in dv (and, when dq is given, *dq = d'q);
// recompute_x() turns the dense multiplier table lamc into xv = x0 + G C_A' lambda.  Returns false on a breakdown (working
// set full, iteration cap, no step); q / cid: the final working set (slot k on lane k); its: applications of G.
//   DEFER = false: the caller has x0 = -G q in LDS (also copied to xv).
//   DEFER = true:  x0 is never formed.  The only use of x0 besides x itself is the residual c_p'x0 - b_p of a warm-start
//                  constraint, and c_p'x0 = -(G c_p)'q comes out of the column the warm start computes anyway; recompute_x
//                  applies G to C_A' lambda - q.  One application of G less per solve (of ~4 for a trot robot).
// NT: threads of the workgroup.  The solve itself is ONE wave's work (slot k on lane k); in a larger workgroup the other waves
// only serve the tile mat-vecs behind column_of_G / recompute_x (qp_exact_robot), so the synchronisation points inside the
// solve are wave-level there: a wave's LDS operations execute in order, the fence only stops the compiler from moving them.
template <int NT>
__device__ __forceinline__ void solver_sync() {
  if constexpr (NT == 64) __syncthreads();
  else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
}
// mu_of(block, row): friction coefficient of cone row `row` of a force block (row_mu: one scalar; under MU4 the leg's own, or the row's).
// The MU4 bodies pass it wrapped with the robot's record (WithBody): the normal-force bounds are then the robot's as well.
template <class F, bool UNI = false> struct WithBody {
  F f;
  const double *rec;
  __device__ __forceinline__ double operator()(const int blk, const int ty) const { return f(blk, ty); }
};
template <class T> struct WithBody_of { static constexpr bool value = false; };
template <class F, bool U> struct WithBody_of<WithBody<F, U>> { static constexpr bool value = true; static constexpr bool uni = U; };
template <class T> struct WithBody_of<T &> : WithBody_of<T> {};
template <int NB, int Q, bool PACKED, bool DEFER, int NT, class ColumnOfG, class RecomputeX, class MuOf>
__device__ __forceinline__ bool exact_active_set(const DevCfg *__restrict__ c, const DevState &st, const int b, const int cmask, const int lane, const bool blk_on,
                                                 double *Tm, double *svv, double *rvv, double *lamc, const double *x0, const double *xv, const double *dv,
                                                 ColumnOfG &&column_of_G, RecomputeX &&recompute_x, MuOf &&mu_of, int &q, int &cid, int &its) {
  using TS_ = ExactT<Q, PACKED>;
  double lo = c->fz_min, hi = c->fz_max;
  if constexpr (WithBody_of<MuOf>::value) { lo = mu_of.rec[REC_BODY + BODY_FZ_MIN]; hi = mu_of.rec[REC_BODY + BODY_FZ_MAX]; if constexpr (WithBody_of<MuOf>::uni) { lo = uniform_f64(lo); hi = uniform_f64(hi); } }   // MU4: the robot's (LDS)
  const double vtol = 1e-9 * (1.0 + hi * 1e-3);
  int am = blk_on ? 0 : 0x3F;   // active-type mask of this lane's block (a block that is no variable has nothing to search)
  double clam = 0.0, cs0 = 0.0;   // slot k on lane k: multiplier; DEFER: c_k'x0 - b_k
  bool failed = false;
  q = 0; cid = -1;
  // r = T s for per-slot values s (lane k < q holds s_k); returns r_k on lane k < q, 0 elsewhere
  auto apply_T = [&](const double sk) -> double {
    if (lane < Q) svv[lane] = lane < q ? sk : 0.0;
    solver_sync<NT>();
    return TS_::row_dot(Tm, svv, lane, q);
  };
  // T <- [[T + r r'/dz, -r/dz], [-r'/dz, 1/dz]]: constraint `id` takes slot q with multiplier lam (idz = 1 / dz)
  auto border = [&](const double rk, const double idz, const int id, const double lam, const double s0) {
    if (lane < Q) rvv[lane] = lane < q ? rk : 0.0;
    solver_sync<NT>();
    const double ri = rk * idz;
    TS_::rank1(Tm, rvv, lane, q, ri, true);
    if (lane < q) { Tm[TS_::at(q, lane)] = -ri; if constexpr (!PACKED) Tm[TS_::at(lane, q)] = -ri; }
    if (lane == q) { Tm[TS_::at(q, q)] = idz; cid = id; clam = lam; cs0 = s0; }
    if (lane == id / 6) am |= 1 << (id % 6);
    q++;
    solver_sync<NT>();
  };
  // drop slot l: rank-1 downdate of T with its row l, then the last slot moves into l and row / column `last` are cleared
  auto drop = [&](const int l) {
    const int last = q - 1;
    const double cl = (lane < q) ? Tm[TS_::at(lane, l)] : 0.0;                  // column l (= row l)
    if (lane < Q) rvv[lane] = cl;
    const double itau = fast_rcp(readlane_f64(cl, l));
    solver_sync<NT>();
    TS_::rank1(Tm, rvv, lane, q, -cl * itau, lane != l);
    const int did = __builtin_amdgcn_readlane(cid, l);
    if (lane == did / 6) am &= ~(1 << (did % 6));
    if (lane == 0) lamc[did] = 0.0;
    solver_sync<NT>();
    const double vlast = (lane < q) ? Tm[TS_::at(last, lane)] : 0.0;   // row `last` after the downdate
    const double dlast = readlane_f64(vlast, last);
    solver_sync<NT>();
    if (l != last) {
      if (lane < q && lane != l && lane != last) { Tm[TS_::at(lane, l)] = vlast; if constexpr (!PACKED) Tm[TS_::at(l, lane)] = vlast; }
      if (lane == l) Tm[TS_::at(l, l)] = dlast;
      const int t_id = __builtin_amdgcn_readlane(cid, last);
      const double t_lam = readlane_f64(clam, last);
      if (lane == l) { cid = t_id; clam = t_lam; }
      if constexpr (DEFER) { const double t_s0 = readlane_f64(cs0, last); if (lane == l) cs0 = t_s0; }
    }
    if (lane < q) { Tm[TS_::at(last, lane)] = 0.0; if constexpr (!PACKED) Tm[TS_::at(lane, last)] = 0.0; }
    if (lane == last) { cid = -1; clam = 0.0; }
    q--;
    solver_sync<NT>();
  };
  // per-slot c_k' v for a vector v in LDS (lane k < q; 0 elsewhere)
  auto slot_dot = [&](const double *v) -> double {
    if (lane >= q) return 0.0;
    const ExactCon k = exact_constraint(cid, mu_of(cid / 6, cid % 6), lo, hi);
    return k.v0 * v[k.i0] + k.v1 * v[k.i1];
  };
  auto refresh_x = [&]() {
    if (lane < q) lamc[cid] = clam;
    solver_sync<NT>();
    its++;
    recompute_x();
  };
  // ---- warm start from the working set of the previous tick (same contact set) ----
  if (b >= 0 && c->warm && st.ws_cnt && __builtin_amdgcn_readfirstlane(st.warm_key[b]) == cmask) {
    int nw = __builtin_amdgcn_readfirstlane(st.ws_cnt[b]);
    nw = nw < Q ? nw : Q;
    const int my_id = lane < nw ? (int)st.ws_ids[(size_t)b * RG_WS_MAX + lane] : 0;   // one coalesced load, not one per constraint
    for (int w = 0; w < nw; w++) {
      const int id = __builtin_amdgcn_readlane(my_id, w);
      if (id >= 6 * NB) continue;
      const ExactCon p = exact_constraint(id, mu_of(id / 6, id % 6), lo, hi);
      its++;
      double dq = 0.0;
      const double sigma = column_of_G(p, DEFER ? &dq : nullptr);
      const double svk = slot_dot(dv), rk = apply_T(svk);
      const double dz = sigma - wave_sum_f64(svk * rk);
      if (!(dz > 1e-9 * sigma)) continue;   // linearly dependent on the constraints already taken
      border(rk, fast_rcp(dz), id, 0.0, -dq - p.rhs);
    }
    // multipliers of the minimiser over the working set as equalities: lambda = -T (C_A x0 - b_A); drop negative ones
    while (q > 0) {
      double s0k = 0.0;
      if constexpr (DEFER) s0k = lane < q ? cs0 : 0.0;
      else if (lane < q) s0k = slot_dot(x0) - exact_constraint(cid, 0.0, lo, hi).rhs;
      const double lk = -apply_T(s0k);
      const double cand = lane < q ? lk : INFINITY;
      const double mn = wave_min_f64(cand);
      if (mn >= 0.0) { clam = lane < q ? lk : 0.0; break; }
      const unsigned long long hit = __ballot(cand == mn);
      if (!hit) { failed = true; break; }   // NaN: not a start
      drop(__ffsll((long long)hit) - 1);
    }
    if (!DEFER && q > 0 && !failed) refresh_x();
  }
  if constexpr (DEFER) { if (!failed) refresh_x(); }   // the first x: G (C_A' lambda - q)
  // ---- dual active-set iterations ----
  const int it_cap = 12 * NB + 40;
  for (int outer = 0; !failed; outer++) {
    if (outer > it_cap) { failed = true; break; }
    // most violated constraint outside the working set: lane b < NB evaluates block b
    double best = 0.0;
    int bid = -1;
    if (lane < NB) {
      const double fx = xv[3 * lane], fy = xv[3 * lane + 1], fz = xv[3 * lane + 2];
      const double sv6[6] = {-fx + mu_of(lane, 0) * fz, fx + mu_of(lane, 1) * fz, -fy + mu_of(lane, 2) * fz, fy + mu_of(lane, 3) * fz, fz - lo, hi - fz};
#pragma unroll
      for (int ty = 0; ty < 6; ty++) if (!((am >> ty) & 1) && sv6[ty] < best) { best = sv6[ty]; bid = 6 * lane + ty; }
    }
    const double bmin = wave_min_f64(best);
    const unsigned long long hitp = __ballot(best == bmin && bid >= 0);
    if (!hitp || bmin >= -vtol) break;
    if (q >= Q) { failed = true; break; }   // working set full: the re-solve list takes the robot
    const int pid = __builtin_amdgcn_readlane(bid, __ffsll((long long)hitp) - 1);
    const ExactCon p = exact_constraint(pid, mu_of(pid / 6, pid % 6), lo, hi);
    its++;
    const double sigma = column_of_G(p, nullptr);
    double s_p = bmin, lam_p = 0.0;
    for (int inner = 0;; inner++) {
      if (inner > Q + 8) { failed = true; break; }
      const double svk = slot_dot(dv), rk = apply_T(svk);
      const double dz = sigma - wave_sum_f64(svk * rk);
      const double cand = (lane < q && rk > 0.0) ? clam * fast_rcp(rk) : INFINITY;
      const double t1 = wave_min_f64(cand);
      const bool have_z = dz > 1e-13 * (1.0 + fabs(sigma));
      const double idz = fast_rcp(dz);
      const double t2 = have_z ? -s_p * idz : INFINITY;
      const double tt = fmin(t1, t2);
      if (!(tt < INFINITY)) { failed = true; break; }
      if (lane < q) clam = fma(-tt, rk, clam);
      lam_p += tt;
      if (have_z) s_p = fma(tt, dz, s_p);
      if (have_z && t2 <= t1) { border(rk, idz, pid, lam_p, 0.0); break; }
      const unsigned long long hit = __ballot(cand == t1 && cand < INFINITY);
      if (!hit) { failed = true; break; }
      drop(__ffsll((long long)hit) - 1);
    }
    if (failed) break;
    refresh_x();
  }
  return !failed;
}

// What every exact body does once the solve has ended, by the role of the launch it runs in:
//   RG_EXACT_FIRST   (inside the QP launch) a robot that was not solved goes to the exact re-solve list of its stance-leg
//                    count and nothing is stored; otherwise the working set is stored for the next tick and the robot is no
//                    (longer) marked for direct routing;
//   RG_EXACT_DIRECT  (the direct lists' concurrent launch: a body sized to fit the LDS a finished QP workgroup frees) as
//                    FIRST, but a solved robot STAYS marked for the front kernel's direct routing (DevState::hard);
//   RG_EXACT_LAST    (the end-of-tick re-solve launch, whose bodies have room for every constraint) a breakdown is a
//                    counted failure, a solved robot is marked for direct routing.
// RG_QP_AUDIT: nothing of the robot's state is touched.  Returns whether the body goes on to its output stage.
enum { RG_EXACT_FIRST = 0, RG_EXACT_LAST = 1, RG_EXACT_DIRECT = 2 };
template <int NC>
__device__ __forceinline__ bool exact_epilogue(const DevCfg *__restrict__ c, const bool solved, const int te, const int b, const int cmask, const int q, const int cid, const int its,
                                               const int mode, const int role) {
  const bool last = role == RG_EXACT_LAST;
  if (mode == RG_QP_AUDIT) return true;
  const QpKernArgsP ka = reread_kernel_args();
  if (!solved) {
    if (te == 0) {
      if (last) { atomicAdd(&ka->st.counts[7], 1); ka->st.hard[b] = 0; }
      else { const int slot = atomicAdd(&ka->st.counts[8 + NC], 1); ka->st.bins[(size_t)(5 + NC) * ka->B + slot] = b; }
      ka->st.iters[b] = mode == RG_QP_RETRY ? ka->st.iters[b] + its : its;
      ka->st.warm_key[b] = -1;
    }
    return last;   // (the last resort writes the row it has: the failure is counted, the command is finite)
  }
  if (c->warm && ka->st.ws_cnt && q <= RG_WS_MAX) {
    if (te < q) ka->st.ws_ids[(size_t)b * RG_WS_MAX + te] = (unsigned char)cid;
    if (te == 0) { ka->st.ws_cnt[b] = q; ka->st.warm_key[b] = cmask; }
  }
  if (te == 0) {
    ka->st.iters[b] = mode == RG_QP_RETRY ? ka->st.iters[b] + its : its;
    ka->st.hard[b] = role == RG_EXACT_FIRST ? 0 : cmask + 1;
  }
  return true;
}

// =====================================================================================================================
// force space: one and two stance legs (N = 30 / 60 variables), 8 x 8 lanes with 8 x 8 register tiles of -G (rows reordered
// for the DPP reduce-scatter, as in the ADMM loop); every lane owns one matrix row after the reduce
// =====================================================================================================================
constexpr bool RG_RANK5_H20 = false;
template <int NC, int H, int Q, int LG = 3, int T = 8>
struct ExactLds {
  static constexpr int m3 = 3 * NC, N = m3 * H, LC = 1 << LG, NT = LC * LC, NP = T * LC, TS = TileShape<T>::TS, NPAD = TS * LC, NPB = NPAD + 2, NB = N / 3;
  // 8 x 8 tiles (one wave at horizon 10, 256 lanes at horizon 20): the matrix is swept with every 6 x 6 block held once
  // (rg_qp_sym6.inc) and moved into the tiles through a staging area that covers everything from `vv` on (nothing there is
  // live at that moment); 4 x 4 tiles (256 lanes at horizon 10) go through tile_sweep
  static constexpr bool SYM6 = T == 8;
  static_assert(T == 4 || (N % 6 == 0 && ((LG == 3 && N <= 60) || (LG == 4 && N <= 120))), "8 x 8 tiles: the symmetric 6 x 6-block sweep covers the matrix");
  static constexpr int NBS = N / 6;                // block rows of the symmetric sweep
  // two stance legs: one direction of every 6 x 6 block is known in closed form (force_space_rank5), the sweep runs on the
  // 5 x 5 corners of the blocks (sym6_sweep<.., 5>: three pivot buffers) and sym5_back_transform restores the 6 x 6 blocks
  // (RG_RANK5_H20: the 256-lane grid of horizon 20 keeps the 6 x 6 sweep -- with the set-up helper in it the hybrid horizon-20
  // launch holds one more scalar across the solve than it has registers for, and the spill costs it a VGPR and 4 B of scratch)
  static constexpr bool RANK5 = SYM6 && NC == 2 && (LG == 3 || RG_RANK5_H20);
  static constexpr int LAMC = (6 * NB + 63) / 64 * 64 < 128 ? 128 : (6 * NB + 63) / 64 * 64;
  // live through the solve
  static constexpr int rec = 0;                    // RG_REC_N
  static constexpr int grf = rec + RG_REC_N;       // 24
  static constexpr int lamc = grf + 24;            // LAMC  multipliers by constraint id (0 = not in the working set)
  static constexpr int sc = lamc + LAMC;           // 8 (workgroups of more than one wave): mat-vec command of the solver wave, then (solved, q, its)
  static constexpr int vv = sc + (NT > 64 ? 8 : 0); // NPAD mat-vec input (groups of T padded to TS)
  static constexpr int x0 = vv + NPAD;             // NP    the gradient q (x0 = -G q itself is never formed: exact_active_set, DEFER)
  static constexpr int x = x0 + NP;                // NP    primal iterate
  static constexpr int d = x + NP;                 // NP    G c_p
  static constexpr int sv = d + NP;                // Q     per-slot vector handed to T (zero beyond q)
  static constexpr int rv = sv + Q;                // Q     per-slot vector of the rank-1 updates of T (zero beyond q)
  static constexpr int Tm = rv + Q;                // T = (C_A G C_A')^-1, zero beyond q x q
  // set-up only, dead once the tile is swept and q is on the owner lanes: ALIASED by T (which is zeroed after the set-up)
  static constexpr int pbuf = Tm;                  // the sweep's ping-pong pivot buffers
  static constexpr int PBUF = SYM6 ? (RANK5 ? 3 : 2) * Sym6<SYM6 ? NBS : 1>::PB : 2 * NPB;
  static constexpr int GU = pbuf + PBUF, GV = GU + m3 * m3, c1 = GV + m3 * m3, c2 = c1 + N, Bw = c2 + N, TBw = Bw + 3 * m3;
  static constexpr int hv = TBw + 3 * m3;          // RG_RANK5_HV (RANK5) the reflector and what force_space_rank5 derives from it
  static constexpr int setup_end = hv + (RANK5 ? RG_RANK5_HV : 0);
  static_assert(GU % 2 == 0 && hv % 2 == 0, "16-byte loads of the Gram blocks and of the reflector");
  static constexpr int stage_end = SYM6 ? vv + Sym6<SYM6 ? NBS : 1>::STG : 0;   // staging area of sym6_to_tile8: from vv on
  template <bool PACKED> static constexpr int total = cmax(cmax((size_t)(Tm + ExactT<Q, PACKED>::doubles), (size_t)setup_end), (size_t)stage_end);
  // what stays live through sym6_to_tile8 ends where the staging area starts, and the staging area fits the layout
  static_assert(!SYM6 || (rec + RG_REC_N <= vv && grf + 24 <= vv && lamc + LAMC <= vv && sc + (NT > 64 ? 8 : 0) <= vv), "sym6_to_tile8 stages over live LDS");
  static_assert(!SYM6 || (stage_end <= total<false> && stage_end <= total<true>), "the staging area of sym6_to_tile8 fits the layout");
};
template <int NC, int H, int Q, bool PACKED = false, int LG = 3, int T = 8>
constexpr size_t qp_exact_lds_doubles() { return (size_t)ExactLds<NC, H, Q, LG, T>::template total<PACKED>; }

// PACKED: storage of T (ExactT).  mode / role: see exact_epilogue; in RG_QP_AUDIT mode `st.rec` is the audit ring entry's record
// array and `b` the slot in it.
// Lane grids (LG, T): (3, 8) one wave, 8 x 8 lanes with 8 x 8 tiles -- horizon 10, N <= 64; (4, 4) 256 lanes with 4 x 4 tiles --
// horizon 10 for batches that leave most of the chip idle (a sweep pivot costs 16 FMAs per lane instead of 64); (4, 8) 256
// lanes with 8 x 8 tiles -- horizon 20, N <= 128.  With more than one wave the solve (one wave's work: a working-set slot per
// lane) runs on wave 0 and the other waves serve its tile mat-vecs: the solver wave writes the input vector and a command
// word, both sides meet at a barrier, every lane multiplies its tile, the owner lanes write the result, a second barrier.
#define RG_EXACT_CMD_D 1      // result to d (a column of G)
#define RG_EXACT_CMD_X 2      // result to x (the primal iterate)
#define RG_EXACT_CMD_DONE 3
template <int NC, int H, int Q, bool PACKED = false, int LG = 3, int T = 8, bool MU4 = false>
__device__ __forceinline__ void qp_exact_robot(const DevCfg *__restrict__ c, const DevState &st, const DevOut &out, const int B, const int b,
                                               const double *tabN, const double *tabS, double *lds, const int mode = RG_QP_SOLVE, const int role = RG_EXACT_FIRST) {
  using LY = ExactLds<NC, H, Q, LG, T>;
  using TSH = TileShape<T>;
  constexpr int LC = LY::LC, NT = LY::NT, m3 = LY::m3, N = LY::N, NB = LY::NB, NP = LY::NP;
  static_assert(N <= NP && NP <= 128 && NB <= 64 && Q <= 64 && Q % 8 == 0 && 6 * NB <= LY::LAMC, "a working-set slot and a force block per lane of the solver wave; rows of T in groups of 8");
  double *vv = lds + LY::vv, *qv = lds + LY::x0, *xv = lds + LY::x, *dv = lds + LY::d, *lamc = lds + LY::lamc, *rec = lds + LY::rec, *grf = lds + LY::grf;
  double *Tm = lds + LY::Tm, *svv = lds + LY::sv, *rvv = lds + LY::rv, *pbuf = lds + LY::pbuf, *GU = lds + LY::GU, *GV = lds + LY::GV, *c1 = lds + LY::c1, *c2 = lds + LY::c2;
  double *Bw = lds + LY::Bw, *TBw = lds + LY::TBw, *sc = lds + LY::sc;
  int cmask;
  double tile[T][T];
  double qi = 0.0;
  {
    const int tid = wg_lane<NT>();
    __syncthreads();
    for (int e = tid; e < RG_REC_N; e += NT) rec[e] = st.rec[(size_t)b * RG_REC_N + e];
    if (tid < 24) grf[tid] = 0.0;
    for (int e = tid; e < LY::LAMC; e += NT) lamc[e] = 0.0;
    __syncthreads();
    cmask = (int)rec[REC_CONTACT];
    if constexpr (LY::RANK5) {   // the reflector with B_w, the projected Gram blocks with the linear term's tables: two stages in all
      force_space_reflector(c, rec, cmask, tid, lds + LY::hv);
      force_space_tables<NC, H, NT, false, MU4, false>(c, rec, cmask, tid, Bw, TBw, GU, GV, nullptr, nullptr, c1, c2);
      force_space_rank5<NT, MU4>(c, rec, tid, Bw, TBw, GU, GV, lds + LY::hv);
    } else force_space_tables<NC, H, NT, false, MU4>(c, rec, cmask, tid, Bw, TBw, GU, GV, nullptr, nullptr, c1, c2);
    __syncthreads();
    // ---- my T x T tile of P = 2 (N (x) G_U + S (x) G_V) + alpha I (identity in the padding), and q of the row I own ----
    int lrv = tid >> LG, lcv = tid & (LC - 1);
    asm volatile("" : "+v"(lrv), "+v"(lcv));
    {
      const int iov = lrv * T + TSH::own_a(lcv);
      if (lcv < T && iov < N) {
        const int a = iov / m3, i = iov - a * m3;
        for (int kq = a; kq < H; kq++) qi += c1[kq * m3 + i] + ((double)(kq - a) + 0.5) * c2[kq * m3 + i];
        qi *= 2.0;
      }
    }
    stamp_phase(0);
    if constexpr (LY::SYM6) {
      // ---- every 6 x 6 block of P once: build, symmetric sweep, move into the 8 x 8 tiles (rows already in the reduce-scatter's
      // order, the sweep's diagonal offset removed) ----
      constexpr int NBS = LY::NBS;
      double X[6][6];
      int sbr, sbc;
      bool son;
      sym6_lane<NBS>(tid, sbr, sbc, son);
      // (a lane below the block diagonal starts with the mirror image of its block: block (bc, br) of the symmetric P)
      if constexpr (m3 == 6) sym6_build_kron6<H>(X, tabN, tabS, GU, GV, sbc, sbr, son, c->alpha);
      else sym6_build_kron3<H>(X, tabN, tabS, GU, GV, sbc, sbr, son, c->alpha);
      stamp_phase(1);
      if constexpr (LY::RANK5) {
        sym6_sweep<NBS, NBS, NT, 5>(X, pbuf, sbr, sbc, son);
        sym5_back_transform(X, lds + LY::hv, sbr, sbc, son);   // (hv is read before sym6_to_tile8's first barrier frees the staging area)
      } else sym6_sweep<NBS, NBS, NT>(X, pbuf, sbr, sbc, son);
      stamp_phase(2);
      sym6_to_tile8<NBS, NBS, LG, NT>(X, sbr, sbc, son, tile, lds + LY::vv, tid);
    } else {
    build_tile_entries<T, H, m3>(tile, tabN, tabS, GU, GV, lrv, lcv, N, c->alpha);
    // ---- symmetric sweep: tile <- -(P^-1) (+2 on the diagonal, removed once), rows reordered for the reduce-scatter ----
    stamp_phase(1);
    tile_sweep<T, LG, N>(tile, pbuf, lrv, lcv);
    stamp_phase(2);
    finish_swept_tile4(tile, lrv, lcv);
    }
    // the set-up arrays are dead: their LDS becomes T (zero outside the working set's q x q block)
    __syncthreads();
    for (int e = tid; e < ExactT<Q, PACKED>::doubles / 2; e += NT) reinterpret_cast<double2 *>(Tm)[e] = make_double2(0.0, 0.0);
    if (tid < Q) { svv[tid] = 0.0; rvv[tid] = 0.0; }
  }
  // ---- lane roles of the solve, from a fresh lane index (nothing of them is live across the sweep) ----
  const int lane = wg_lane<NT>();
  const int lr = lane >> LG, lc = lane & (LC - 1);
  const int io = lr * T + TSH::own_a(lc);    // the matrix row this lane owns after the reduce-scatter (owner lanes: lc < T)
  const bool owner = lc < T, own_real = owner && io < N;
  if (owner) qv[io] = own_real ? qi : 0.0;
  __syncthreads();   // q of every row, the zeroed T: in LDS before the solve reads them
  int q = 0, cid = -1, its = 0;
  bool solved = false;
  const int wave = NT > 64 ? __builtin_amdgcn_readfirstlane(lane >> 6) : 0;   // (scalar: the barriers below sit in wave-uniform control flow)
  if (wave == 0) {
    auto mu_of = [&](const int blk, const int ty) -> double { if constexpr (MU4) return row_mu<MU4>(c, rec, nth_leg(cmask, blk % NC), ty);
                                                         else return row_mu<MU4>(c, nullptr, MU4 ? nth_leg(cmask, blk % NC) : 0, ty); };   // block = step * NC + stance-leg slot (rec: captured by the MU4 lambda only)
    // dst = G vv on the owner lanes (tile = -G): every lane of the workgroup takes part, between two barriers
    auto apply_G = [&](const int cmd) {
      if constexpr (NT > 64) { if (lane == 0) sc[0] = (double)cmd; }
      __syncthreads();
      const double t = tile_matvec<T, LG>(tile, vv, lr, lc);
      if (owner) (cmd == RG_EXACT_CMD_D ? dv : xv)[io] = own_real ? t : 0.0;
      __syncthreads();
    };
    // d = G c_p -> dv, returns sigma = c_p' G c_p; *dq = d'q
    auto column_of_G = [&](const ExactCon &p, double *dq) -> double {
      for (int r = lane; r < NP; r += 64) vv[TSH::pad(r)] = (r == p.i0 ? p.v0 : 0.0) + (r == p.i1 ? p.v1 : 0.0);
      apply_G(RG_EXACT_CMD_D);
      if (dq) {
        double a = 0.0;
        for (int r = lane; r < NP; r += 64) a = fma(dv[r], qv[r], a);
        *dq = wave_sum_f64(a);
      }
      return uniform_f64(p.v0 * dv[p.i0] + p.v1 * dv[p.i1]);   // the same value on every lane: keep what depends on it scalar
    };
    // x = G (C_A' lambda - q): the block lanes assemble C_A' lambda from the dense multiplier table
    auto recompute_x = [&]() {
      if (lane < NB) {
        const double l0 = lamc[6 * lane], l1 = lamc[6 * lane + 1], l2 = lamc[6 * lane + 2], l3 = lamc[6 * lane + 3], l4 = lamc[6 * lane + 4], l5 = lamc[6 * lane + 5];
        const int r0 = 3 * lane, r1 = r0 + 1, r2 = r0 + 2;
        vv[TSH::pad(r0)] = (l1 - l0) - qv[r0];
        vv[TSH::pad(r1)] = (l3 - l2) - qv[r1];
        if constexpr (MU4) vv[TSH::pad(r2)] = fma(mu_of(lane, 0), l0, fma(mu_of(lane, 1), l1, fma(mu_of(lane, 2), l2, fma(mu_of(lane, 3), l3, l4 - l5)))) - qv[r2];
        else vv[TSH::pad(r2)] = fma(mu_of(lane, 0), (l0 + l1) + (l2 + l3), l4 - l5) - qv[r2];
      }
      for (int r = N + lane; r < NP; r += 64) vv[TSH::pad(r)] = 0.0;
      apply_G(RG_EXACT_CMD_X);
    };
    if constexpr (MU4) solved = exact_active_set<NB, Q, PACKED, true, NT>(c, st, mode == RG_QP_AUDIT ? -1 : b, cmask, lane, lane < NB, Tm, svv, rvv, lamc, qv, xv, dv, column_of_G, recompute_x, WithBody<decltype(mu_of)>{mu_of, rec}, q, cid, its);
    else solved = exact_active_set<NB, Q, PACKED, true, NT>(c, st, mode == RG_QP_AUDIT ? -1 : b, cmask, lane, lane < NB, Tm, svv, rvv, lamc, qv, xv, dv, column_of_G, recompute_x, mu_of, q, cid, its);
    if constexpr (NT > 64) {   // the helper waves leave their loop; the outcome goes to every wave
      if (lane == 0) { sc[0] = (double)RG_EXACT_CMD_DONE; sc[1] = solved ? 1.0 : 0.0; sc[2] = (double)q; sc[3] = (double)its; }
      __syncthreads();
    }
  } else {
    for (;;) {   // helper waves: serve the solver wave's mat-vecs until it says DONE
      __syncthreads();
      const int cmd = (int)sc[0];
      if (cmd == RG_EXACT_CMD_DONE) break;
      const double t = tile_matvec<T, LG>(tile, vv, lr, lc);
      if (owner) (cmd == RG_EXACT_CMD_D ? dv : xv)[io] = own_real ? t : 0.0;
      __syncthreads();
    }
  }
  if constexpr (NT > 64) { solved = sc[1] != 0.0; q = (int)sc[2]; its = (int)sc[3]; }
  stamp_phase(3);
  const int te = wg_lane<NT>();
  if (!exact_epilogue<NC>(c, solved, te, b, cmask, q, cid, its, mode, role)) return;
  if (te < m3) grf[3 * nth_leg(cmask, te / 3) + te % 3] = -xv[te];
  __syncthreads();
  qp_write_outputs<NT>(c, rec, grf, b, te, mode);
  if (mode == RG_QP_AUDIT) audit_compare(c, rec, grf, b, !solved);
}

// =====================================================================================================================
// wrench space: three and four stance legs.  The reduction of qp_wrench_robot (rg_qp_wrench_kernel.inc) with rho = 0:
//     G = P^-1 = I / alpha + X [ (alpha I + K')^-1 - I / alpha ] X',     X = blockdiag(Ch)',  Ch = L^-1 C  (6 x 3 nc per step),
// applied, never formed: 6 x 3 block product and quad reduce on the block lanes (lane 4 k + j = horizon step k, leg slot j),
// the 60 x 60 tile mat-vec, the 3 x 6 block product back.  Variables, constraints and the working set live on the block
// lanes' index space (block = lane 4 k + j, unused slots j >= nc are no variables).
// =====================================================================================================================
template <int NC, int H, int Q>
struct ExactWrenchLds {
  static constexpr int m3 = 3 * NC, NW = 6 * H, NP = 64, NPAD = 80, NPB = NPAD + 2, NV = 12 * H;
  // live through the solve
  static constexpr int vv = 0;                     // NPAD  mat-vec input (wrench space, padded groups)
  static constexpr int uv = vv + NPAD;             // NP    mat-vec output
  static constexpr int qh = uv + NP;               // NW    L' q_w
  static constexpr int x0 = qh + NW, x = x0 + NV, d = x + NV;   // NV each, indexed 3 * block + axis
  static constexpr int lamc = d + NV;              // 2 NV  multipliers by constraint id
  static constexpr int rec = lamc + 2 * NV;        // RG_REC_N
  static constexpr int grf = rec + RG_REC_N;       // 24
  static constexpr int sv = grf + 24, rv = sv + Q;
  static constexpr int Tm = rv + Q;                // packed lower triangle of T
  // set-up only, aliased by T
  static constexpr int pbuf = Tm;                  // 2 * NPB
  static constexpr int Cm = pbuf + 2 * NPB, Ch = Cm + 6 * m3, Qm = Ch + 6 * m3, Lm = Qm + 36, AU = Lm + 36, AV = AU + 36, qw = AV + 36;
  static constexpr int EU = (qw + NW + 1) & ~1, EV = EU + RG_E6_DOUBLES;
  static constexpr int setup_end = EV + RG_E6_DOUBLES;
  static constexpr int total = (Tm + ExactT<Q, true>::doubles > setup_end) ? Tm + ExactT<Q, true>::doubles : setup_end;
};
template <int NC, int H, int Q>
constexpr size_t qp_exact_wrench_lds_doubles() { return (size_t)ExactWrenchLds<NC, H, Q>::total; }

template <int NC, int H, int Q, bool MU4 = false>
__device__ __forceinline__ void qp_exact_wrench_robot(const DevCfg *__restrict__ c, const DevState &st, const DevOut &out, const int B, const int b,
                                                      const double *tabN, const double *tabS, double *lds, const int mode = RG_QP_SOLVE, const int role = RG_EXACT_FIRST) {
  using LY = ExactWrenchLds<NC, H, Q>;
  constexpr int T = 8, LG = 3, NT = 64, m3 = LY::m3, NW = LY::NW, NB = 4 * H;
  static_assert(NW <= 64 && NB <= 64 && Q <= 64 && Q % 8 == 0 && NC >= 3, "one wave: a wrench row per lane, a block per lane, a working-set slot per lane");
  double *vv = lds + LY::vv, *uv = lds + LY::uv, *qh = lds + LY::qh, *x0 = lds + LY::x0, *xv = lds + LY::x, *dv = lds + LY::d, *lamc = lds + LY::lamc;
  double *rec = lds + LY::rec, *grf = lds + LY::grf, *svv = lds + LY::sv, *rvv = lds + LY::rv, *Tm = lds + LY::Tm, *pbuf = lds + LY::pbuf;
  double *Cm = lds + LY::Cm, *Ch = lds + LY::Ch, *Qm = lds + LY::Qm, *Lm = lds + LY::Lm, *AU = lds + LY::AU, *AV = lds + LY::AV, *qw = lds + LY::qw;
  double *EU = lds + LY::EU, *EV = lds + LY::EV;
  const double dt = c->dt;
  const double aa = c->alpha, inv_aa = uniform_f64(1.0 / aa);
  int cmask;
  bool degenerate = false;
  double tile[T][T];
  double Cb[6][3];
  {
    const int tid = wg_lane<NT>();
    __syncthreads();
    for (int e = tid; e < RG_REC_N; e += NT) rec[e] = st.rec[(size_t)b * RG_REC_N + e];
    if (tid < 24) grf[tid] = 0.0;
    for (int e = tid; e < 2 * LY::NV; e += NT) lamc[e] = 0.0;
    if (tid >= NW && tid < LY::NP) vv[(tid >> 3) * 10 + (tid & 7)] = 0.0;   // padding of the mat-vec input: never written again
    __syncthreads();
    cmask = (int)rec[REC_CONTACT];
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
    {
      double Qr[6][6];
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) Qr[i][j] = Qm[i * 6 + j];
#pragma unroll
      for (int j = 0; j < 6; j++) {
        double s = Qr[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s = fma(-L[j][k], L[j][k], s);
        if (!(s > 1e-12 * Qr[j][j])) { degenerate = true; s = 1.0; }   // (near-)collinear feet: rank C < 6 -- the force-space re-solve takes it
        const double d = sqrt(s);
        L[j][j] = d;
        Li[j] = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
          double t = Qr[i][j];
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
    // q_w(a) = 2 sum_{k >= a} [ dt g1(k) + (k - a + 1/2) dt^2 R6' g2(k) ]  (as in qp_wrench_robot)
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
      double su = 0.0, sv_ = 0.0;
#pragma unroll
      for (int r = 0; r < 6; r++) {
        const double li = Lm[r * 6 + i], lj = Lm[r * 6 + j];
        su = fma((r < 3 ? c->w[6 + r] : c->w[9 + r - 3] * im2) * li, lj, su);
        double ri = li, rj = lj;   // rows of R6 L: (invcp L0, L1, tanp L0 + L2, L3, L4, L5)
        if (r == 0) { ri = rec[REC_INVCP] * li; rj = rec[REC_INVCP] * lj; }
        if (r == 2) { ri = fma(rec[REC_TANP], Lm[i], li); rj = fma(rec[REC_TANP], Lm[j], lj); }
        sv_ = fma((r < 3 ? c->w[r] : c->w[3 + r - 3] * im2) * ri, rj, sv_);
      }
      AU[tid] = su * dt * dt;
      AV[tid] = sv_ * dt * dt * dt * dt;
      put_periodic6(EU, i, j, AU[tid]);
      put_periodic6(EV, i, j, AV[tid]);
    }
    for (int e = tid; e < NW; e += NT) {   // qh = L' q_w per step
      const int a = e / 6, cc = e % 6;
      double s = 0.0;
      for (int r = cc; r < 6; r++) s = fma(Lm[r * 6 + cc], qw[a * 6 + r], s);
      qh[e] = s;
    }
    __syncthreads();
    // ---- my 8 x 8 tile of alpha I + K', swept to -(alpha I + K')^-1 ----
    {
      const int lr = tid >> LG, lc = tid & 7;
      build_tile_kron6<H>(tile, tabN, tabS, EU, EV, lr, lc, NW, aa);
      tile_sweep<8, LG, NW>(tile, pbuf, lr, lc);
      if (lr == lc) {
#pragma unroll
        for (int ta = 0; ta < T; ta++) tile[ta][ta] -= 2.0;
      }
      permute_tile_rows_for_reduce(tile, lc);
    }
    // ---- this block lane's 6 x 3 block of Ch (lanes with b0 = 1 hold the rows rotated by three, see qp_wrench_robot) ----
    {
      const int t2 = wg_lane<NT>(), bj = t2 & 3, b0 = t2 & 1;
      const bool blk_real = (t2 >> 2) < H && bj < NC;
#pragma unroll
      for (int cc = 0; cc < 6; cc++) {
        const int src = b0 ? (cc + 3) % 6 : cc;
#pragma unroll
        for (int d = 0; d < 3; d++) Cb[cc][d] = blk_real ? Ch[src * m3 + 3 * bj + d] : 0.0;
      }
    }
    // the set-up arrays are dead: their LDS becomes T
    __syncthreads();
    for (int e = tid; e < ExactT<Q, true>::doubles / 2; e += NT) reinterpret_cast<double2 *>(Tm)[e] = make_double2(0.0, 0.0);
    if (tid < Q) { svv[tid] = 0.0; rvv[tid] = 0.0; }
  }
  // ---- lane roles of the solve (WrenchLane), from a fresh lane index ----
  const int lane = wg_lane<NT>();
  const WrenchLane<H, LG> WL(lane);
  const int io = WL.io, iov_pad = WL.iov_pad, bj = WL.bj, b1 = WL.b1, padA = WL.padA, padB = WL.padB;
  const int ubase0 = WL.ubase0, ubase1 = WL.ubase1;
  const bool own_real = WL.own_real, quad_real = WL.quad_real, blk_real = WL.quad_real && bj < NC;
  const int lr = lane >> LG, lc = lane & 7;
  // out = G w for the force 3-vector w of this block lane; `from_qh`: the input is q = X qh instead (G q = X (alpha I + K')^-1 qh)
  auto apply_G = [&](const double w0, const double w1, const double w2, const bool from_qh, double &o0, double &o1, double &o2) {
    if (!from_qh) {
      double cw[6];
#pragma unroll
      for (int cc = 0; cc < 6; cc++) cw[cc] = fma(Cb[cc][2], w2, fma(Cb[cc][1], w1, Cb[cc][0] * w0));
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
    const double tw = tile8_matvec<LG>(tile, vv, lr, lc);   // (alpha I + K')^-1 (X' w)
    if (own_real) uv[io] = from_qh ? tw : fma(-vv[iov_pad], inv_aa, tw);
    __syncthreads();
    o0 = 0.0; o1 = 0.0; o2 = 0.0;
    if (blk_real) {
      const double u6[6] = {uv[ubase0], uv[ubase0 + 1], uv[ubase0 + 2], uv[ubase1], uv[ubase1 + 1], uv[ubase1 + 2]};
      double x3[3] = {from_qh ? 0.0 : w0 * inv_aa, from_qh ? 0.0 : w1 * inv_aa, from_qh ? 0.0 : w2 * inv_aa};
#pragma unroll
      for (int cc = 0; cc < 6; cc++) {
#pragma unroll
        for (int d = 0; d < 3; d++) x3[d] = fma(Cb[cc][d], u6[cc], x3[d]);
      }
      o0 = x3[0]; o1 = x3[1]; o2 = x3[2];
    }
  };
  auto mu_of = [&](const int blk, const int ty) -> double { if constexpr (MU4) return row_mu<MU4>(c, rec, nth_leg(cmask, blk & 3), ty);
                                                         else return row_mu<MU4>(c, nullptr, MU4 ? nth_leg(cmask, blk & 3) : 0, ty); };   // block = lane 4 k + stance-leg slot (rec: captured by the MU4 lambda only)
  // d = G c_p -> dv, returns sigma = c_p' G c_p
  auto column_of_G = [&](const ExactCon &p, double *) -> double {
    const int pb = p.i1 / 3;   // the constraint's block = its lane
    const double w0 = (lane == pb && p.i0 == 3 * pb) ? p.v0 : 0.0, w1 = (lane == pb && p.i0 == 3 * pb + 1) ? p.v0 : 0.0;
    const double w2 = (lane == pb) ? ((p.i0 == p.i1 ? p.v0 : 0.0) + p.v1) : 0.0;
    double o0, o1, o2;
    apply_G(w0, w1, w2, false, o0, o1, o2);
    if (lane < NB) { dv[3 * lane] = o0; dv[3 * lane + 1] = o1; dv[3 * lane + 2] = o2; }
    __syncthreads();
    return uniform_f64(p.v0 * dv[p.i0] + p.v1 * dv[p.i1]);
  };
  // x = x0 + G C_A' lambda
  auto recompute_x = [&]() {
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if (blk_real) {
      const double l0 = lamc[6 * lane], l1 = lamc[6 * lane + 1], l2 = lamc[6 * lane + 2], l3 = lamc[6 * lane + 3], l4 = lamc[6 * lane + 4], l5 = lamc[6 * lane + 5];
      w0 = l1 - l0; w1 = l3 - l2;
      if constexpr (MU4) w2 = fma(mu_of(lane, 0), l0, fma(mu_of(lane, 1), l1, fma(mu_of(lane, 2), l2, fma(mu_of(lane, 3), l3, l4 - l5))));
      else w2 = fma(mu_of(lane, 0), (l0 + l1) + (l2 + l3), l4 - l5);
    }
    double o0, o1, o2;
    apply_G(w0, w1, w2, false, o0, o1, o2);
    if (lane < NB) { xv[3 * lane] = x0[3 * lane] + o0; xv[3 * lane + 1] = x0[3 * lane + 1] + o1; xv[3 * lane + 2] = x0[3 * lane + 2] + o2; }
    __syncthreads();
  };
  // ---- x0 = -G q ----
  {
    double o0, o1, o2;
    apply_G(0.0, 0.0, 0.0, true, o0, o1, o2);
    if (lane < NB) {
      x0[3 * lane] = -o0; x0[3 * lane + 1] = -o1; x0[3 * lane + 2] = -o2;
      xv[3 * lane] = -o0; xv[3 * lane + 1] = -o1; xv[3 * lane + 2] = -o2;
    }
  }
  __syncthreads();
  int q = 0, cid = -1, its = 1;
  bool solved = false;
  if constexpr (MU4) { if (!degenerate) solved = exact_active_set<NB, Q, true, false, 64>(c, st, mode == RG_QP_AUDIT ? -1 : b, cmask, lane, blk_real, Tm, svv, rvv, lamc, x0, xv, dv, column_of_G, recompute_x, WithBody<decltype(mu_of), true>{mu_of, rec}, q, cid, its); }
  else if (!degenerate) solved = exact_active_set<NB, Q, true, false, 64>(c, st, mode == RG_QP_AUDIT ? -1 : b, cmask, lane, blk_real, Tm, svv, rvv, lamc, x0, xv, dv, column_of_G, recompute_x, mu_of, q, cid, its);
  const int te = wg_lane<NT>();
  if (!exact_epilogue<NC>(c, solved, te, b, cmask, q, cid, its, mode, role)) return;
  if (te < NC) { const int leg = nth_leg(cmask, te); grf[3 * leg] = -xv[3 * te]; grf[3 * leg + 1] = -xv[3 * te + 1]; grf[3 * leg + 2] = -xv[3 * te + 2]; }
  __syncthreads();
  qp_write_outputs<NT>(c, rec, grf, b, te, mode);
  if (mode == RG_QP_AUDIT) audit_compare(c, rec, grf, b, !solved);
}
