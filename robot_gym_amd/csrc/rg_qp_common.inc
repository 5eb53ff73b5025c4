// rg_qp_common.inc -- helpers shared by every QP kernel (register pins, stance-leg indexing, the dynamic LDS
// array, workgroup vote, kernel-argument re-read, per-device LDS attribute bookkeeping, horizon tables)
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// index of the k-th set bit of a 4-bit contact mask (k-th stance leg) without a scratch array
__device__ __forceinline__ int nth_leg(int mask, int k) {
  int l0 = __builtin_ctz(mask | 16);
  int m1 = mask & (mask - 1);
  int l1 = __builtin_ctz(m1 | 16);
  int m2 = m1 & (m1 - 1);
  int l2 = __builtin_ctz(m2 | 16);
  int m3_ = m2 & (m2 - 1);
  int l3 = __builtin_ctz(m3_ | 16);
  return k == 0 ? l0 : (k == 1 ? l1 : (k == 2 ? l2 : l3));
}

extern __shared__ __attribute__((aligned(16))) double smem[];

// Lane index inside the workgroup.  In a one-wave workgroup it is the lane id, which v_mbcnt produces from nothing, and the
// volatile asm makes every call site compute its own copy: nothing derived from threadIdx.x (v0 at kernel entry) is then kept
// alive -- in practice: spilled at kernel entry and reloaded -- across the solver loops of every body of a launch.
template <int NT>
__device__ __forceinline__ int wg_lane() {
  if constexpr (NT == 64) {
    int t;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(t));
    return t;
  } else {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
  }
}

// Workgroup-wide "does any lane still move" vote.  A single-wave workgroup needs one ballot.  Larger workgroups: one ballot
// per wave, the wave leaders' flags through LDS, a barrier on either side (the second one also orders what the caller wrote
// to LDS before the vote against the next rewrite of the slots).
// History: round 2 replaced __syncthreads_or (the device library's workgroup reduction: LDS atomic + barriers + mbcnt, ~95
// instructions) by this after the 256-lane horizon-20 launch returned forces 10-30 % off for its three-leg robots whenever
// another QP kernel had run on the device before it -- one wave had left the ADMM loop at its first vote.  The diagnosis
// written down then ("the library primitive gives different waves different results when the timing shifts") is NOT
// confirmed: a stand-alone reproducer (tests/studies/syncthreads_or_repro.hip: 256-lane workgroups voting in a loop with
// uneven work per wave, cold instruction cache, LDS left dirty by a preceding kernel) shows 0 disagreements between waves in
// 1.6 M workgroup runs for the library primitive and for this one.  What is established: with this vote the failure does not
// occur (tests/test_gpu_parity.py::test_launch_order_independence replays the sequence, and fails on the old code), every
// LDS slot the bodies share around a vote is written and read on opposite sides of one of its two barriers, and it is
// cheaper (config 5: -2 %).
__shared__ int rg_vote_slots[16];
template <int NT>
__device__ __forceinline__ bool workgroup_any(int pred) {
  if constexpr (NT <= 64) return __ballot(pred) != 0ull;
  else {
    const int any = __ballot(pred) != 0ull;
    if ((threadIdx.x & 63) == 0) rg_vote_slots[threadIdx.x >> 6] = any;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) r |= rg_vote_slots[k];
    __syncthreads();   // the slots are rewritten at the next vote; this also orders what the caller wrote to LDS before the vote
    return r != 0;
  }
}

// Workgroup-wide sums of three per-lane values (the dot products of the extrapolation test below) WITHOUT barriers of their
// own: sum3_publish before the vote's workgroup_any (whose barrier orders the LDS slots), sum3_collect after it; every lane
// gets the same three results.  `scratch`: 3 * (NT / 64) LDS doubles, only touched when NT > 64; the slots are next written
// a vote period later, with the iteration's barriers in between.  Single-wave workgroups do everything in sum3_collect.
template <int NT>
__device__ __forceinline__ void sum3_publish(const double a, const double b, const double c, double *scratch) {
  if constexpr (NT > 64) {
    const double sa = wave_sum_f64(a), sb = wave_sum_f64(b), sc = wave_sum_f64(c);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { scratch[3 * w] = sa; scratch[3 * w + 1] = sb; scratch[3 * w + 2] = sc; }
  }
}
template <int NT>
__device__ __forceinline__ void sum3_collect(double &a, double &b, double &c, const double *scratch) {
  if constexpr (NT > 64) {
    a = 0.0; b = 0.0; c = 0.0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) { a += scratch[3 * k]; b += scratch[3 * k + 1]; c += scratch[3 * k + 2]; }
  } else {
    a = wave_sum_f64(a); b = wave_sum_f64(b); c = wave_sum_f64(c);
  }
}

// Dominant-mode (Aitken / vector-extrapolation) step of the ADMM iterate, decided at a convergence vote.
// Once the set of active constraints has settled, ADMM is an affine map w -> A w + b of w = (z, y); a robot that
// crawls does so along ONE slow eigenvector, its vote-to-vote displacements d1 = w_k - w_(k-c), d0 = w_(k-c) - w_(k-2c)
// are then parallel and shrink by a fixed ratio r, and the fixed point is w_k + d1 r / (1 - r).  From sums over the
// robot's entries  d11 = <d1,d1>, d00 = <d0,d0>, d10 = <d1,d0>:  jump when cos^2 = d10^2 / (d11 d00) > 0.9 and
// r = d10 / d00 in (0.5, 0.98); returns the gain r / (1 - r) (< 49), or 0 for no jump (a slower mode is left alone:
// its rate estimate is too sensitive, and the distance estimate m g of the stopping test relies on the rate that was
// used).  ADMM converges from any (z, y), so a poor jump costs iterations, never correctness; what it can upset is the
// stopping test, which is why a robot that has jumped passes stricter ones (qp_tile_robot).  Measured on the bench
// workload's crawling robots (numpy model of this loop, tests/studies/admm_extrapolation_model.py): 230-290 -> 110-145
// iterations, the population mean unchanged.
// (k = DevCfg::accel_k = rg_mpc_config {accel_cos2 0.9, accel_rmax 0.98, accel_rmin 0.5, accel_rate_cap 0.999})
__device__ __forceinline__ double extrapolation_gain(const double *k, const double d11, const double d00, const double d10) {
  const bool ok = d10 > 0.0 && d10 * d10 > k[0] * d11 * d00 && d10 > k[2] * d00 && d10 < k[1] * d00;
  return ok ? d10 * fast_rcp(d00 - d10) : 0.0;
}
// The same three sums as a convergence guard for robots that have been extrapolated in this stage: while consecutive
// window displacements point the same way (cos^2 > 0.5) the iterate is still r / (1 - r) displacements away from where
// it is going, r = d10 / d00 (capped at 0.999).  The NEXT vote multiplies each entry's movement by this factor and holds
// it against the distance tolerance, like the per-entry estimate m r / (1 - r) with r = m / m_prev but with a rate
// measured on the whole iterate: the per-entry one sees nothing when a slow mode moves every entry by less than the
// rounding of its ratio.  (Seed 97 of the configuration sweep: after a jump had removed the dominant mode, a mode with
// r ~ 0.995 was left moving less than the tolerance per window -- 2.9e-4 off.)
__device__ __forceinline__ double remaining_distance_factor(const double *k, const double d11, const double d00, const double d10) {
  if (!(d10 > 0.0 && d10 * d10 > 0.5 * d11 * d00)) return 0.0;
  const double r = fmin(d10 * fast_rcp(d00), k[3]);
  return r * fast_rcp(1.0 - r);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember it per (kernel instantiation, device),
// so one process driving several GPUs sets it on each of them
static bool lds_attr_needed(bool (&done)[64]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;
  if (done[dev]) return false;
  done[dev] = true;
  return true;
}

// Every QP kernel starts its parameter list with (cfg, state, outputs, batch).  The per-robot bodies need most of those
// pointers only before and after the solver loops; used directly, the by-value structs stay live in ~60 SGPRs across the loops,
// and on the fused kernel that pushed uniform loop constants out to VGPR lanes and those to scratch (8 scratch reloads per ADMM
// iteration).  The epilogues therefore re-read what they need from the kernarg segment through a pointer the optimiser cannot
// see through, with QpKernArgs as the layout of the segment's head.
// (Measured and dropped: ONE by-value QpKernArgs as the kernels' first parameter -- the tie by construction -- costs the fused
// kernel 54 scratch operations instead of 26, one of them inside the wrench-space ADMM loop.)  The tie is made at compile time
// instead: RG_CHECK_KERNARGS(kernel) fails to compile unless the kernel's real parameter list starts with exactly these four
// types, and the static_asserts below pin the kernarg offsets those four parameters get (each at its natural alignment, in
// order) to the struct's.
struct QpKernArgs { const DevCfg *c; DevState st; DevOut out; int B; };
typedef const __attribute__((address_space(4))) QpKernArgs *QpKernArgsP;
__device__ __forceinline__ QpKernArgsP reread_kernel_args() {
  QpKernArgsP p = (QpKernArgsP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
template <class F> struct KernArgHead { static constexpr bool ok = false; };
template <class... Rest> struct KernArgHead<void (*)(const DevCfg *, DevState, DevOut, int, Rest...)> { static constexpr bool ok = true; };
#define RG_CHECK_KERNARGS(...) static_assert(KernArgHead<decltype(&__VA_ARGS__)>::ok, "QP kernels start with (const DevCfg *, DevState, DevOut, int): reread_kernel_args() reads them back through QpKernArgs")
constexpr size_t kernarg_align_up(size_t off, size_t a) { return (off + a - 1) / a * a; }
static_assert(offsetof(QpKernArgs, c) == 0 && offsetof(QpKernArgs, st) == kernarg_align_up(sizeof(const DevCfg *), alignof(DevState)) &&
              offsetof(QpKernArgs, out) == kernarg_align_up(offsetof(QpKernArgs, st) + sizeof(DevState), alignof(DevOut)) &&
              offsetof(QpKernArgs, B) == kernarg_align_up(offsetof(QpKernArgs, out) + sizeof(DevOut), alignof(int)),
              "QpKernArgs lays its members out like four consecutive kernel parameters");

// Run-time guard on top of that (one compare per workgroup): the re-read view agrees with the kernel's own arguments.
__device__ __forceinline__ void check_kernel_args(const DevCfg *c, const int B) {
  const QpKernArgsP ka = reread_kernel_args();
  if (ka->c != c || ka->B != B) __builtin_trap();
}

// ---- audit lane ----------------------------------------------------------------------------------------------------
// The ADMM exit test is a stack of tuned rules (movement, primal residual, geometric distance estimates, the rules for
// robots that were extrapolated); each was added after a seeded sweep found a robot that had "converged" > 1e-4 off.
// So that the next such case cannot go unnoticed, every tick about audit_k pseudo-randomly picked robots whose ADMM
// solve CONVERGED are solved again by the exact active-set bodies and the joint torques compared (rg_mpc_audit_stats).
//   capture (ADMM epilogues, this launch): the robot's front->QP record and its first-step forces are copied into a slot of
//     ring entry st.audit_ring -- nothing else is needed to pose the same QP again;
//   compare (exact bodies, mode RG_QP_AUDIT, rg_qp_*_retry_kernel launched on the library's side stream): solve from the
//     copied record, tau = J' f for both force sets, accumulate count / over-tolerance / maxima.  Outputs are never touched.
#define RG_QP_SOLVE 0   // body writes the robot's outputs
#define RG_QP_RETRY 1   // ... as the exact re-solve of a robot ADMM left unconverged (iteration counts add up)
#define RG_QP_AUDIT 2   // exact re-solve of a captured record: compare with the captured ADMM forces, write no output
__device__ __forceinline__ unsigned audit_hash(unsigned x, const unsigned seed) {   // murmur3 finaliser
  x = x * 0x9E3779B1u ^ seed;
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
// Every lane of the workgroup calls this once the first-step forces grf[0..11] (LDS) are complete; `converged`, `b` and the
// pick are workgroup-uniform.  list_nc: the exact re-solve list this body's robots go to (stance legs; 4 for the schedule body).
template <int NT>
__device__ __forceinline__ void audit_capture(const bool converged, const int b, const int list_nc, const double *rec, const double *grf) {
  const QpKernArgsP ka = reread_kernel_args();
  const int k = ka->st.audit_k;
  if (k <= 0 || !converged) return;
  const unsigned h = audit_hash((unsigned)b, ka->st.audit_seed);
  if ((unsigned)(((unsigned long long)h * (unsigned)ka->B) >> 32) >= (unsigned)k) return;   // probability k / B per robot and tick
  const int ring = ka->st.audit_ring;
  const int lane = wg_lane<NT>();
  if (lane == 0) rg_vote_slots[15] = atomicAdd(&ka->st.audit_cnt[ring], 1);
  __syncthreads();
  const int slot = rg_vote_slots[15];
  if (slot < RG_AUDIT_SLOTS) {
    const size_t base = (size_t)ring * RG_AUDIT_SLOTS + slot;
    for (int e = lane; e < RG_REC_N; e += NT) ka->st.audit_rec[base * RG_REC_N + e] = rec[e];
    if (lane < 12) ka->st.audit_f[base * 12 + lane] = grf[lane];
    if (lane == 0) ka->st.audit_idx[base] = b | (list_nc << 24);
  } else if (lane == 0) atomicAdd(&ka->st.audit_stat[5], 1ull);   // the tick's slots are full: dropped, counted
  __syncthreads();   // the broadcast slot is rewritten by the next robot of a looping workgroup
}
// Exact bodies in RG_QP_AUDIT mode, after their epilogue put the exact first-step forces in grf[0..11] and torques in
// grf[12..23] (LDS): same J' f * MOTOR_DIRECTION for the captured ADMM forces, then the parity metric of tests/helpers.py
// (per robot: max_j |dtau_j| / max(max_j |tau_j|, 1 N m); per joint: |dtau_j| / max(|tau_j|, 1 N m)).
__device__ __forceinline__ void audit_compare(const DevCfg *__restrict__ c, const double *rec, const double *grf, const int slot, const bool failed) {
  if (threadIdx.x != 0) return;
  const QpKernArgsP ka = reread_kernel_args();
  unsigned long long *stat = ka->st.audit_stat;
  if (failed) { atomicAdd(&stat[4], 1ull); return; }
  const double *fa = ka->st.audit_f + ((size_t)ka->st.audit_ring * RG_AUDIT_SLOTS + slot) * 12;
  double tmax = 1.0, emax = 0.0, eelem = 0.0;
  for (int j = 0; j < 12; j++) {
    const int leg = j / 3, jj = j - 3 * leg;
    const double *J = &rec[REC_JAC + 9 * leg];
    const double ta = (fa[3 * leg] * J[jj] + fa[3 * leg + 1] * J[3 + jj] + fa[3 * leg + 2] * J[6 + jj]) * c->mdir[j];
    const double te = grf[12 + j], d = fabs(ta - te);
    tmax = fmax(tmax, fabs(te)); emax = fmax(emax, d); eelem = fmax(eelem, d / fmax(fabs(te), 1.0));
  }
  const double rel = emax / tmax;
  atomicAdd(&stat[0], 1ull);
  if (!(rel <= c->audit_tol)) atomicAdd(&stat[1], 1ull);
  // non-negative doubles order like their bit patterns; a NaN (all-ones exponent) lands above every finite value
  atomicMax(&stat[2], (unsigned long long)__double_as_longlong(fabs(rel)));
  atomicMax(&stat[3], (unsigned long long)__double_as_longlong(fabs(eelem)));
}

// Measurement build (make stamp -> librg_mpc_stamp.so, never the shipped library): every QP workgroup notes the 100 MHz wall
// clock when it starts, and the output stage puts (start, end, low 24 bits, exact in float32) into the first two entries of
// the robot's optional grf row -- tests/studies/fused_launch_schedule.py turns them into the launch's actual schedule.
#ifdef RG_STAMP
__shared__ unsigned rg_stamp_start;
__shared__ unsigned rg_stamp_phase[6];
__device__ __forceinline__ void stamp_start() { if (threadIdx.x == 0) { rg_stamp_start = (unsigned)(wall_clock64() & 0xFFFFFF); for (int k = 0; k < 6; k++) rg_stamp_phase[k] = 0; } }
// phase k of a body ends now (exact body: 0 tables, 1 tile, 2 sweep, 3 solve; wrench ADMM body: 0 tables, 1 tile, 2 sweep, 3 loop)
__device__ __forceinline__ void stamp_phase(const int k) { if (threadIdx.x == 0) rg_stamp_phase[k] = (unsigned)(wall_clock64() & 0xFFFFFF); }
#else
__device__ __forceinline__ void stamp_start() {}
__device__ __forceinline__ void stamp_phase(const int) {}
#endif

// Output stage shared by every QP body.  In: the first-step forces grf[0..11] (LDS, complete, zero for legs without a force).
// tau = J' f * MOTOR_DIRECTION for all twelve joints (left in grf[12..23]: the audit compares them), the optional grf /
// tau_stance rows, and the 60-float command row: a joint of a leg whose desired state is SWING gets its position tuple
// (q*, kp, 0, kd, 0), every other joint (0, 0, 0, 0, tau) -- the merge of LocomotionController.get_action (SURVEY 8a-19).  A
// non-finite command (NaN state in, or a solver breakdown) is counted, never silent.  RG_QP_AUDIT: nothing is written.
template <int NT>
__device__ __forceinline__ void qp_write_outputs(const DevCfg *__restrict__ c, const double *rec, double *grf, const int b, const int tid, const int mode) {
  const QpKernArgsP ka = reread_kernel_args();
  if (tid < 12) {
    const int leg = tid / 3, j = tid % 3;
    const double *J = &rec[REC_JAC + 9 * leg];
    const double tau = (grf[3 * leg] * J[j] + grf[3 * leg + 1] * J[3 + j] + grf[3 * leg + 2] * J[6 + j]) * c->mdir[tid];
    grf[12 + tid] = tau;
    if (mode != RG_QP_AUDIT) {
      if (ka->out.grf) ka->out.grf[(size_t)b * 12 + tid] = (float)grf[tid];
      if (ka->out.tau_stance) ka->out.tau_stance[(size_t)b * 12 + tid] = (float)tau;
    }
  }
  __syncthreads();
  if (mode != RG_QP_AUDIT && tid < 60) {
    const int j = tid / 5, f = tid % 5;
    const int emit = ((int)rec[REC_EMIT] >> j) & 1;
    float v;
    if (emit) v = (f == 1) ? (float)c->kp[j] : (f == 3 ? (float)c->kd[j] : 0.f);
    else v = (f == 4) ? (float)grf[12 + j] : 0.f;
    if (!(emit && f == 0)) ka->out.action[(size_t)b * 60 + tid] = v;   // q* of a joint with a position command: written by swing_ik_lane
    if (__ballot(!(fabsf(v) <= 3.0e38f)) != 0ull && tid == 0) atomicAdd(&ka->st.counts[7], 1);
  }
#ifdef RG_STAMP
  if (mode != RG_QP_AUDIT && tid == 0 && ka->out.grf) { ka->out.grf[(size_t)b * 12] = (float)rg_stamp_start; ka->out.grf[(size_t)b * 12 + 1] = (float)(unsigned)(wall_clock64() & 0xFFFFFF); for (int k = 0; k < 6; k++) ka->out.grf[(size_t)b * 12 + 2 + k] = (float)rg_stamp_phase[k]; }
#endif
}

constexpr size_t cmax(size_t a, size_t b) { return a > b ? a : b; }

// workgroup preamble shared by all QP kernels: 2 N_ab and 2 S_ab into LDS
template <int H>
__device__ __forceinline__ void load_horizon_tables(const DevCfg *__restrict__ c, double *tabN, double *tabS, const int tid, const int nt) {
  for (int e = tid; e < H * H; e += nt) { tabN[e] = 2.0 * c->Ntab[e]; tabS[e] = 2.0 * c->Stab[e]; }
}
