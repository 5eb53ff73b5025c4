// rg_qp_fused_kernel.inc -- one launch for every stance-leg count (horizons 10 and 20).
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// At one horizon every QP body runs on the same lane grid -- H = 10: one 64-lane wave (8 x 8 lanes),
// H = 20: 256 lanes (16 x 16) -- with 1-2 legs on the force-space tile body and 3-4 legs on the
// wrench-space body, so the four per-count launches collapse into one: a workgroup switches body per
// work item (block-uniform branch).  This removes three launch gaps and, more important, the tail of each
// per-count launch: at H = 10, 835 four-leg robots alone fill 40 % of the chip's 2048 wave slots, 3261
// two-leg robots 1.6 rounds of them; together they are 2.0 rounds.
// (FusedShape<H>: lane grid per horizon, defined in rg_qp_tile.inc)

// EX (horizon 10) selects the bodies: 0 -- ADMM for every stance-leg count; 1 -- one- and two-leg robots run the exact
// active-set body (qp_exact_robot), three and four legs keep the wrench-space ADMM body: the RG_SOLVER_HYBRID plan; 2 -- every
// robot runs an exact body (three and four legs in wrench space, qp_exact_wrench_robot): RG_SOLVER_ACTIVE_SET.
// Working-set capacities of the exact bodies inside the fused launch; a robot that needs more goes to the re-solve list
// (largest working sets seen on the bench workloads: ~40 two-leg, 39 four-leg)
#define RG_EXACT_Q 40    // force space: full T, 40 x 42 doubles of LDS
#define RG_EXACT_QW 64   // wrench space: packed T, 64 * 65 / 2 doubles (every lane a slot: six workgroups per CU)
// The DIRECT lists inside the QP launch.  Robots the front kernel sends straight to the exact solver (DevState::hard: one- and
// two-leg robots whose working set outgrew RG_EXACT_Q on a recent tick) are the most expensive jobs of the tick, 100-200 us
// each.  The first RG_DIRECT_HEAD workgroups of the grid -- dispatched first -- take the first entries of those lists on a
// body with room for RG_DIRECT_Q constraints (a packed T: the largest that fits this launch's LDS per workgroup); with no
// such robot they exit at once.  (They used to get a launch of their own on a side stream when a pinned hint word said a
// recent tick had had exact solves: the host runs many ticks ahead of the GPU, so the hint came late or not at all and the
// robots were solved AFTER the QP launch -- a realistic-geometry tick took 220 us instead of 160; issuing that launch every
// tick cost the workloads without such robots 6-9 %.)  What the head cannot take is left to the end-of-tick launch.
#define RG_DIRECT_HEAD 64
#define RG_DIRECT_Q 56
// Lane grid of a fused launch.  WIDE (horizon 10, hybrid plan): 256 lanes per robot with 4 x 4 tiles instead of one wave with
// 8 x 8 tiles -- the small-batch grid (rg_mpc_config.lane_grid): a robot's dependent chain is what a small batch waits for, and
// a quarter of the FMAs per lane per sweep pivot / mat-vec shortens it; the chip has the wave slots to spare there.
template <int H, int WIDE> struct FusedGrid {
  static constexpr int LG = WIDE ? 4 : FusedShape<H>::LG, TT = WIDE ? 4 : 8, T1 = FusedShape<H>::T1, NT = (1 << LG) * (1 << LG);
};
// working-set capacity of the horizon-20 exact body (full T in LDS: 64 x 66 doubles; two workgroups per CU have the room)
#define RG_EXACT_Q20 64
template <int H, int MINW, int EX, int WIDE = 0, bool MU4 = false>
__global__ void __launch_bounds__((FusedGrid<H, WIDE>::NT), MINW)
rg_qp_fused_kernel(const DevCfg *__restrict__ c, DevState st, DevOut out, int B) {
  using FG = FusedGrid<H, WIDE>;
  constexpr int LG = FG::LG, TT = FG::TT, T1 = FG::T1, NT = FG::NT;
  static_assert(!WIDE || (H == 10 && EX == 1), "the 256-lane grid at horizon 10 exists for the hybrid plan");
  static_assert(EX == 0 || H == 10 || EX == 1, "horizon 20 has the hybrid plan's exact body for one / two legs only");
  const int wg = (int)blockIdx.x;
  double *tabN = smem, *tabS = smem + H * H, *lds = smem + 2 * H * H;
  constexpr int HEAD = (EX != 0 && H == 10) ? RG_DIRECT_HEAD : 0;
  // workgroups beyond the batch: the swing-leg IK lanes of this tick (rg_front_kernel.inc: swing_ik_lane), dispatched last
  if (wg >= HEAD + B) { swing_ik_lane(c, st, out, B, (wg - HEAD - B) * NT + (int)threadIdx.x); return; }
  if constexpr (HEAD > 0) {
    if (wg < HEAD) {   // the direct lists of one- and two-leg robots (see RG_DIRECT_HEAD)
      if (!st.direct_on) return;
      const int d2 = st.counts[2], d1 = st.counts[1], w = wg;
      if (w >= d2 + d1) return;
      stamp_start();
      check_kernel_args(c, B);
      load_horizon_tables<H>(c, tabN, tabS, wg_lane<NT>(), NT);
      if (w < d2) qp_exact_robot<2, H, RG_DIRECT_Q, true, LG, TT, MU4>(c, st, out, B, __builtin_amdgcn_readfirstlane(st.bins[(size_t)2 * B + w]), tabN, tabS, lds, RG_QP_SOLVE, RG_EXACT_DIRECT);
      else qp_exact_robot<1, H, RG_DIRECT_Q, true, LG, TT, MU4>(c, st, out, B, __builtin_amdgcn_readfirstlane(st.bins[(size_t)1 * B + (w - d2)]), tabN, tabS, lds, RG_QP_SOLVE, RG_EXACT_DIRECT);
      return;
    }
  }
  stamp_start();
  check_kernel_args(c, B);
  load_horizon_tables<H>(c, tabN, tabS, wg_lane<NT>(), NT);
  // work order: cost classes, most expensive first (front kernel, plan 1); entry = robot | stance legs << 24.
  // ONE work item per workgroup (the grid is the batch): no work loop.  A loop here -- even one that never runs twice --
  // made everything the four bodies share loop-invariant: constants, lane indices and the loop's own carried values were
  // hoisted to the kernel entry, kept across every solver loop of every body, and spilled (scratch stores and reloads in
  // front of every robot).
  const int work = wg - HEAD;
  int cls = 0, first = 0, run = 0;
#pragma unroll
  for (int k = 0; k < RG_COST_CLASSES; k++) { const int n = st.counts[16 + k]; if (k > 0 && work >= run) { cls = k; first = run; } run += n; }
  if (work >= run) return;
  const int entry = __builtin_amdgcn_readfirstlane(st.bins[(size_t)(10 + cls) * B + (work - first)]);
  const int b = entry & 0xFFFFFF, nc = (entry >> 24) & 0xF, big = (entry >> 28) & 1;   // big: front kernel, RG_EXACT_BIG_WS
  if constexpr (H == 20) {
    // horizon 20: three and four legs run the schedule body with a constant schedule -- the same QP, and the body that
    // has an exact wrench-space re-solve behind it (rg_qp_sched_retry_kernel)
    if (nc >= 3) { qp_sched_robot<H, LG, false, MU4>(c, st, out, B, b, tabN, tabS, lds); return; }
    if constexpr (EX != 0) {   // hybrid plan: one / two legs on the exact body (256 lanes, 8 x 8 tiles; the solve on wave 0)
      if (nc == 2) qp_exact_robot<2, H, RG_EXACT_Q20, false, LG, TT, MU4>(c, st, out, B, b, tabN, tabS, lds);
      else qp_exact_robot<1, H, RG_EXACT_Q20, false, LG, TT, MU4>(c, st, out, B, b, tabN, tabS, lds);
      return;
    }
  } else {
    if constexpr (EX == 2) {
      if (nc == 4) { qp_exact_wrench_robot<4, H, RG_EXACT_QW, MU4>(c, st, out, B, b, tabN, tabS, lds); return; }
      if (nc == 3) { qp_exact_wrench_robot<3, H, RG_EXACT_QW, MU4>(c, st, out, B, b, tabN, tabS, lds); return; }
    } else {
      if (nc == 4) { qp_wrench_robot<4, H, LG, TT, MU4>(c, st, out, B, b, tabN, tabS, lds); return; }
      if (nc == 3) { qp_wrench_robot<3, H, LG, TT, MU4>(c, st, out, B, b, tabN, tabS, lds); return; }
    }
  }
  if constexpr (EX != 0 && H == 10) {
    if (nc == 2 && big) qp_exact_robot<2, H, RG_DIRECT_Q, true, LG, TT, MU4>(c, st, out, B, b, tabN, tabS, lds);
    else if (nc == 2) qp_exact_robot<2, H, RG_EXACT_Q, false, LG, TT, MU4>(c, st, out, B, b, tabN, tabS, lds);
    else qp_exact_robot<1, H, RG_EXACT_Q, false, LG, TT, MU4>(c, st, out, B, b, tabN, tabS, lds);
  } else if constexpr (EX == 0) {
    if (nc == 2) qp_tile_robot<2, H, 8, LG, MU4>(c, st, out, B, b, tabN, tabS, lds);
    else qp_tile_robot<1, H, T1, LG, MU4>(c, st, out, B, b, tabN, tabS, lds);
  }
}


template <int H, int EX, int WIDE = 0, bool MU4 = false>
static hipError_t launch_qp_fused(const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, hipStream_t s) {
  using FG = FusedGrid<H, WIDE>;
  constexpr int LG = FG::LG, TT = FG::TT, T1 = FG::T1, NT = FG::NT;
  constexpr int QX = H == 20 ? RG_EXACT_Q20 : RG_EXACT_Q;
  constexpr size_t body12 = EX ? cmax(qp_exact_lds_doubles<2, H, QX, false, LG, TT>(), qp_exact_lds_doubles<1, H, QX, false, LG, TT>())
                               : cmax(qp_tile_lds_doubles<2, H, 8, LG>(), qp_tile_lds_doubles<1, H, T1, LG>());
  constexpr size_t body34 = [] {   // (if constexpr: the wrench-space ADMM layout exists at horizon 10 only)
    if constexpr (H == 20) return qp_sched_lds_doubles<H, LG, false>();
    else if constexpr (EX == 2) return cmax(qp_exact_wrench_lds_doubles<4, 10, RG_EXACT_QW>(), qp_exact_wrench_lds_doubles<3, 10, RG_EXACT_QW>());
    else return cmax(qp_wrench_lds_doubles<4, H, LG, TT>(), qp_wrench_lds_doubles<3, H, LG, TT>());
  }();
  constexpr size_t body = cmax(body34, body12);
  const size_t lds = sizeof(double) * (body + 2 * H * H);
  // horizon 10: eight one-wave workgroups per CU (20 KB each); horizon 20: two 256-lane workgroups per CU (80 KB each)
  static_assert(sizeof(double) * (body + 2 * H * H) <= (H == 10 && !WIDE && EX == 1 ? 20 : 80) * 1024, "workgroups per CU of the fused launch (default plan at horizon 10: eight)");
  static bool attr_done[64] = {};
  if (lds > 64 * 1024 && lds_attr_needed(attr_done)) {
    hipError_t e = hipFuncSetAttribute((const void *)rg_qp_fused_kernel<H, 2, EX, WIDE, MU4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if constexpr (EX != 0 && H == 10) static_assert(cmax(qp_exact_lds_doubles<2, 10, RG_DIRECT_Q, true, LG, TT>(), qp_exact_lds_doubles<1, 10, RG_DIRECT_Q, true, LG, TT>()) <= body,
                                                  "RG_DIRECT_Q: the direct body runs in this launch's LDS per workgroup");
  // (the direct lists' head,) one workgroup per robot -- dispatched in cost-class order as wave slots free up (3 % faster
  // than a persistent grid of 8 workgroups per CU looping over the list) --, then the swing IK lanes
  const int grid = ((EX != 0 && H == 10) ? RG_DIRECT_HEAD : 0) + B + (4 * B + NT - 1) / NT;
  // (wide grid: two 4-wave workgroups per CU are resident, 512 robots; the ADMM robots -- the launch's longest jobs -- are
  // dispatched first, and a second round of 25 us exact robots ends before they do.  At 128 VGPRs, four workgroups per CU, the
  // wrench-space ADMM loop spills 13 values per iteration.)
  constexpr int MINW = 2;
  RG_CHECK_KERNARGS(rg_qp_fused_kernel<H, MINW, EX, WIDE, MU4>);
  rg_qp_fused_kernel<H, MINW, EX, WIDE, MU4><<<dim3(grid), dim3(NT), lds, s>>>(dcfg, st, dout, B);
  return hipGetLastError();
}

template <bool MU4>
static hipError_t launch_qp_fused_mu(int H, int exact, bool wide, const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, hipStream_t s) {
  if (H == 10 && wide && exact == 1) return launch_qp_fused<10, 1, 1, MU4>(dcfg, st, dout, B, s);
  if (H == 10) return exact == 2 ? launch_qp_fused<10, 2, 0, MU4>(dcfg, st, dout, B, s) : (exact == 1 ? launch_qp_fused<10, 1, 0, MU4>(dcfg, st, dout, B, s) : launch_qp_fused<10, 0, 0, MU4>(dcfg, st, dout, B, s));
  if (H == 20) return exact == 1 ? launch_qp_fused<20, 1, 0, MU4>(dcfg, st, dout, B, s) : launch_qp_fused<20, 0, 0, MU4>(dcfg, st, dout, B, s);
  return hipErrorInvalidValue;
}
// mu4: the four friction coefficients differ (the kernels that carry a per-lane coefficient, see leg_mu)
static hipError_t launch_qp_fused_any(int H, int exact, bool wide, bool mu4, const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, hipStream_t s) {
  return mu4 ? launch_qp_fused_mu<true>(H, exact, wide, dcfg, st, dout, B, s) : launch_qp_fused_mu<false>(H, exact, wide, dcfg, st, dout, B, s);
}

// Exact re-solve launch (horizon 10): what the QP launch could not finish -- an ADMM robot at its iteration cap, an exact
// body whose working set overflowed, four collinear feet -- on ONE-WAVE exact bodies with room for every constraint:
//   one / two stance legs: the force-space exact body (qp_exact_robot) with a packed T for 64 constraints (a 60-variable QP
//     has at most 60 independent active constraints: it cannot overflow);
//   three / four legs, and every robot of a contact schedule: the wrench-space active-set body of the schedule QP
//     (qp_sched_robot<10, 3, true>: any set of (step, leg) pairs in contact, rank-deficient stances included, T for 120).
// Round 3's kernel inlined four 256-lane force-space bodies behind the work loop (256 VGPRs + 87 AGPRs of spill space, ~140
// SGPRs parked in VGPR lanes) and its result depended on how the source was arranged; round 4 first reduced it to one
// 256-lane body (still 256 + 79 AGPRs), and this form has none of it: 64 threads, no AGPR, no scratch, and a workgroup that
// fits into the LDS a finished QP workgroup leaves behind -- which is what lets the direct lists' launch actually overlap the
// QP launch (a 256-lane workgroup with 76 KB of LDS found no CU until the QP launch had nothing left to dispatch).
// `what` selects the work:
//   RETRY_ALL    (end of the tick, caller's stream) the four re-solve lists AND the four direct lists (lists 1..4: robots the
//                front kernel sent straight to the exact solver, see DevState::hard) -- the usual case being that all are empty;
//   RETRY_DIRECT (side stream, concurrently with the QP launch) the direct lists of one- and two-leg robots only (the
//                ONLY12 instantiation: 21 KB of LDS per workgroup) -- rg_mpc_step does this when a recent tick had exact
//                solves, so that a persistently hard robot costs the tick nothing but a wave slot;
//   RETRY_LISTS  (end of the tick, after a RETRY_DIRECT) the re-solve lists and the direct lists of three / four legs;
//   RETRY_AUDIT  (audit side stream) the audit ring entry of this tick -- records of robots whose ADMM solve converged,
//                copied by the ADMM epilogues (audit_capture); the bodies compare instead of writing outputs.
//   RETRY_AFTER_HEAD (end of the tick, hybrid / exact plans) as RETRY_ALL, minus the first RG_DIRECT_HEAD entries of the one- and
//                two-leg direct lists, which the QP launch's head workgroups have solved.
enum { RETRY_ALL = 0, RETRY_AUDIT = 1, RETRY_DIRECT = 3, RETRY_LISTS = 4, RETRY_AFTER_HEAD = 5 };
#define RG_RESOLVE_Q 64
template <int H, bool ONLY12, bool MU4 = false>
__global__ void __launch_bounds__(64, 1)
rg_qp_resolve_kernel(const DevCfg *__restrict__ c, DevState st, DevOut out, int B, const int what) {
  const bool audit = what == RETRY_AUDIT;
  const int r4 = st.counts[12], r3 = st.counts[11], r2 = st.counts[10], r1 = st.counts[9];
  const int d4 = st.direct_on ? st.counts[4] : 0, d3 = st.direct_on ? st.counts[3] : 0, d2 = st.direct_on ? st.counts[2] : 0, d1 = st.direct_on ? st.counts[1] : 0;
  // work items of this launch, in the order 4-, 3-, 2-, 1-leg re-solve lists, then the direct lists
  const int n4 = what == RETRY_DIRECT ? 0 : r4, n3 = what == RETRY_DIRECT ? 0 : r3, n2 = what == RETRY_DIRECT ? 0 : r2, n1 = what == RETRY_DIRECT ? 0 : r1;
  const int m4 = what == RETRY_DIRECT ? 0 : d4, m3 = what == RETRY_DIRECT ? 0 : d3;
  // entries of the two- / one-leg direct lists already solved by the QP launch's head workgroups
  const int head2 = what == RETRY_AFTER_HEAD ? (d2 < RG_DIRECT_HEAD ? d2 : RG_DIRECT_HEAD) : 0;
  const int head1 = what == RETRY_AFTER_HEAD ? (d1 < RG_DIRECT_HEAD - head2 ? d1 : RG_DIRECT_HEAD - head2) : 0;
  const int m2 = what == RETRY_LISTS ? 0 : d2 - head2, m1 = what == RETRY_LISTS ? 0 : d1 - head1;
  // the end-of-tick launch leaves the number of exact solves of this tick in pinned host memory: rg_mpc_step reads it some
  // ticks later, without waiting, to decide whether the direct lists get their own concurrent launch
  // (only when the number changes: a store to host memory costs this otherwise empty launch ~4 us)
  if ((what == RETRY_ALL || what == RETRY_LISTS || what == RETRY_AFTER_HEAD) && st.direct_on && blockIdx.x == 0 && threadIdx.x == 0) {
    const int v = r4 + r3 + r2 + r1 + d4 + d3 + d2 + d1;
    if (v != *st.hint_dev) { *st.hint_dev = v; *st.hint_host = v; }
  }
  int total = n4 + n3 + n2 + n1 + m4 + m3 + m2 + m1;
  if (audit) { total = st.audit_cnt[st.audit_ring]; total = total < RG_AUDIT_SLOTS ? total : RG_AUDIT_SLOTS; }
  if ((int)blockIdx.x >= total) return;   // the usual case: nothing to re-solve, leave before touching the tables
  double *tabN = smem, *tabS = smem + H * H, *lds = smem + 2 * H * H;
  check_kernel_args(c, B);
  load_horizon_tables<H>(c, tabN, tabS, threadIdx.x, 64);
  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    // every work item reads its own view of the arguments through the opaque kernarg pointer: nothing of a body's set-up can
    // be computed before the loop and carried -- spilled -- across the robots a workgroup solves one after the other
    const QpKernArgsP ka = reread_kernel_args();
    const DevCfg *c = ka->c;
    DevState sw = *(const DevState *)&ka->st;
    if (audit) sw.rec = sw.audit_rec + (size_t)sw.audit_ring * RG_AUDIT_SLOTS * RG_REC_N;   // the bodies read record `slot` of the ring entry
    int idx, nc, mode = RG_QP_RETRY;
    if (audit) { idx = work; nc = st.audit_idx[(size_t)st.audit_ring * RG_AUDIT_SLOTS + work] >> 24; mode = RG_QP_AUDIT; }
    else {
      int w = work;
      if (w < n4) { nc = 4; idx = st.bins[(size_t)9 * B + w]; }
      else if ((w -= n4) < n3) { nc = 3; idx = st.bins[(size_t)8 * B + w]; }
      else if ((w -= n3) < n2) { nc = 2; idx = st.bins[(size_t)7 * B + w]; }
      else if ((w -= n2) < n1) { nc = 1; idx = st.bins[(size_t)6 * B + w]; }
      else {   // direct lists: first solve of the tick for these robots
        w -= n1;
        mode = RG_QP_SOLVE;
        if (w < m4) nc = 4;
        else if ((w -= m4) < m3) nc = 3;
        else if ((w -= m3) < m2) { nc = 2; w += head2; }
        else { w -= m2; nc = 1; w += head1; }
        idx = st.bins[(size_t)nc * B + w];
      }
    }
    idx = __builtin_amdgcn_readfirstlane(idx);
    nc = __builtin_amdgcn_readfirstlane(nc);
    // ONLY12 (the direct lists' concurrent launch): room for RG_DIRECT_Q constraints -- what fits, with everything else, into
    // the LDS of one QP-launch workgroup, so that the workgroup can start wherever such a workgroup has finished (with room
    // for all 64 it needs 21 KB against the 19.8 KB a finished QP workgroup frees: the launch then found no CU before the QP
    // launch had nothing left to dispatch, ~86 us into the tick, and its 80 us robots ended the tick 70 us late); a robot
    // with more active constraints than that goes to the end-of-tick lists.
    constexpr int QX = ONLY12 ? RG_DIRECT_Q : RG_RESOLVE_Q, ROLE = ONLY12 ? RG_EXACT_DIRECT : RG_EXACT_LAST;
    if (nc == 2) qp_exact_robot<2, H, QX, true, 3, 8, MU4>(c, sw, out, B, idx, tabN, tabS, lds, mode, ROLE);
    else if (nc == 1) qp_exact_robot<1, H, QX, true, 3, 8, MU4>(c, sw, out, B, idx, tabN, tabS, lds, mode, ROLE);
    else if constexpr (!ONLY12) qp_sched_robot<H, 3, true, MU4>(c, sw, out, B, idx, tabN, tabS, lds, mode);
  }
}

template <bool ONLY12, bool MU4>
static hipError_t launch_qp_resolve_impl(const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, int cu_count, hipStream_t s, int what) {
  constexpr int H = 10;
  constexpr int QX = ONLY12 ? RG_DIRECT_Q : RG_RESOLVE_Q;
  constexpr size_t body12 = cmax(qp_exact_lds_doubles<2, H, QX, true>(), qp_exact_lds_doubles<1, H, QX, true>());
  constexpr size_t body = ONLY12 ? body12 : cmax(body12, qp_sched_lds_doubles<H, 3, true>());
  if constexpr (ONLY12) {   // the direct lists' workgroups start in the LDS a finished workgroup of the (hybrid) QP launch leaves
    constexpr size_t qp_wg = cmax(cmax(qp_exact_lds_doubles<2, 10, RG_EXACT_Q>(), qp_exact_lds_doubles<1, 10, RG_EXACT_Q>()),
                                  cmax(qp_wrench_lds_doubles<4, H, 3>(), qp_wrench_lds_doubles<3, H, 3>()));
    static_assert(body12 <= qp_wg, "RG_DIRECT_Q: the direct body must fit a QP-launch workgroup's LDS");
  }
  const size_t lds = sizeof(double) * (body + 2 * H * H);
  static_assert(sizeof(double) * (body + 2 * H * H) <= 160 * 1024, "active-set state must fit the CU's LDS");
  static bool attr_done[64] = {};
  if (lds > 64 * 1024 && lds_attr_needed(attr_done)) {
    hipError_t e = hipFuncSetAttribute((const void *)rg_qp_resolve_kernel<H, ONLY12, MU4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  int grid = cu_count;   // the lists are short; one one-wave workgroup per CU takes them in one round
                         // (the empty launch costs the same 4-5 us with 8, 32 or 256 workgroups: it is the launch floor)
  if (grid > B) grid = B;
  if (what == RETRY_AUDIT) grid = st.audit_k + st.audit_k / 4;   // one workgroup per expected entry
  if (what == RETRY_DIRECT) grid = 64;   // a handful of robots at most, next to a full QP launch
  if (grid > RG_AUDIT_SLOTS) grid = RG_AUDIT_SLOTS;
  if (grid < 1) grid = 1;
  RG_CHECK_KERNARGS(rg_qp_resolve_kernel<H, ONLY12, MU4>);
  rg_qp_resolve_kernel<H, ONLY12, MU4><<<dim3(grid), dim3(64), lds, s>>>(dcfg, st, dout, B, what);
  return hipGetLastError();
}
static hipError_t launch_qp_resolve_h10(bool mu4, const DevCfg *dcfg, const DevState &st, const DevOut &dout, int B, int cu_count, hipStream_t s, int what) {
  if (mu4) return what == RETRY_DIRECT ? launch_qp_resolve_impl<true, true>(dcfg, st, dout, B, cu_count, s, what) : launch_qp_resolve_impl<false, true>(dcfg, st, dout, B, cu_count, s, what);
  return what == RETRY_DIRECT ? launch_qp_resolve_impl<true, false>(dcfg, st, dout, B, cu_count, s, what) : launch_qp_resolve_impl<false, false>(dcfg, st, dout, B, cu_count, s, what);
}
