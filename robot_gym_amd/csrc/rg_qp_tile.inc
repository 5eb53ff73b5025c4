// rg_qp_tile.inc -- the register-tile primitives every QP body shares: the in-register symmetric sweep, the tile builds, the
// tile mat-vec with its DPP reduce-scatter, the lane grid per horizon, and the force-space set-up tables.
// Included by rg_mpc.hip (single translation unit) after rg_qp_common.inc; not a stand-alone header.
#pragma once

// ------------------------------------------------------------------------------------
// A row-per-lane layout is bound by the LDS instruction pipe (rocprof: SQ_ACTIVE_INST_LDS ~ 88 % of kernel
// time in the round-1 experiment): every f64 FMA needs half a 16-B broadcast read.  Here the lanes of a robot form an LC x LC grid and lane (lr, lc) keeps the T x T tile
// rows lr*T.., cols lc*T.. of the (padded, NP = T*LC) symmetric matrix in VGPRs, so every value
// read from LDS feeds T FMAs:
//   sweep step kp: 2T values (pivot-row entries of my columns and, by symmetry, of my rows)
//                  for T*T FMAs; the LC lanes of lane-row kp/T publish the row in parallel.
//   ADMM mat-vec : T values of the rhs for T*T FMAs, then a reduce-scatter over the LC lanes
//                  of a lane-row (cross-lane, no LDS data) leaves one finished entry per lane.
// ------------------------------------------------------------------------------------
// Opaque "use + redefine" of one tile row: no instruction is emitted, but the optimiser can no longer
// defer this row's updates past this point.  (Left alone, hipcc turns the unrolled pivot steps into
// a look-ahead schedule that keeps every step's pivot-row values live: > 380 VGPRs, spills in the loop.)
template <int T>
__device__ __forceinline__ void pin_row(double (&t)[T]) {
  static_assert(T == 4 || T == 8, "tile sizes of the lane grids: 8 and 4");
  if constexpr (T == 8) asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]));
  else asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
}

// The reduce-scatter that finishes an 8 x 8-tile mat-vec keeps a different half of the partial sums on
// each lane (selected by lane-column bits 2 and 0): 24 v_cndmask per mat-vec.  Reordering the tile ROWS of
// each lane once (rows h <-> h+4 where bit 2 is set, then h <-> h+2 where bit 0 is set) makes "keep the low
// half, send the high half" right for every lane, so the selects disappear from the iteration loop.
__device__ __forceinline__ void permute_tile_rows_for_reduce(double (&tile)[8][8], const int lc) {
  const bool s4 = (lc >> 2) & 1, s2 = lc & 1;
#pragma unroll
  for (int h = 0; h < 4; h++)
#pragma unroll
    for (int tb = 0; tb < 8; tb++) { const double a = tile[h][tb], b = tile[h + 4][tb]; tile[h][tb] = s4 ? b : a; tile[h + 4][tb] = s4 ? a : b; }
#pragma unroll
  for (int h = 0; h < 8; h++) {
    if (h & 2) continue;
#pragma unroll
    for (int tb = 0; tb < 8; tb++) { const double a = tile[h][tb], b = tile[h + 2][tb]; tile[h][tb] = s2 ? b : a; tile[h + 2][tb] = s2 ? a : b; }
  }
}
// row sums of a row-permuted tile's mat-vec partials -> the lane's own row (4 b2 + 2 b0 + b1 of its lane-row)
template <int LG>
__device__ __forceinline__ double reduce_scatter8_permuted(double (&acc)[8], const int lc) {
#pragma unroll
  for (int h2 = 0; h2 < 4; h2++) acc[h2] += dpp_f64<0x141>(acc[4 + (h2 ^ 2)]);   // 7 - i inside 8 lanes: that lane's bit 0 differs too, hence ^ 2
#pragma unroll
  for (int h2 = 0; h2 < 2; h2++) acc[h2] += dpp_f64<0xB1>(acc[2 + h2]);    // lane ^ 1
  const bool up = (lc >> 1) & 1;
  const double keep = up ? acc[1] : acc[0], send = up ? acc[0] : acc[1];
  double tot = keep + dpp_f64<0x4E>(send);                                  // lane ^ 2
  if constexpr (LG >= 4) tot += dpp_f64<0x128>(tot);
#pragma unroll
  for (int kx = 4; kx < LG; kx++) tot += __shfl_xor(tot, 1 << kx);
  return tot;
}

// ---- the same for 4 x 4 tiles on a 16 x 16 lane grid (horizon 10 on 256 lanes: the small-batch lane grid) ----
// Two reduce-scatter steps (lane ^ 1, lane ^ 2) leave one row sum per lane, then two all-reduce steps over the four lane
// groups of a lane-row (row_ror:4, row_ror:8); the rows of each lane's tile are reordered once so that every lane keeps its
// low half.  Kept row: 2 b0 + b1 of the lane-row's four rows.
__device__ __forceinline__ void permute_tile_rows_for_reduce4(double (&tile)[4][4], const int lc) {
  const bool s2 = lc & 1, s1 = (lc >> 1) & 1;
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int tb = 0; tb < 4; tb++) { const double a = tile[h][tb], b = tile[h + 2][tb]; tile[h][tb] = s2 ? b : a; tile[h + 2][tb] = s2 ? a : b; }
#pragma unroll
  for (int h = 0; h < 4; h += 2)   // both halves: the half a lane sends in the first step must be in its partner's order
#pragma unroll
    for (int tb = 0; tb < 4; tb++) { const double a = tile[h][tb], b = tile[h + 1][tb]; tile[h][tb] = s1 ? b : a; tile[h + 1][tb] = s1 ? a : b; }
}
__device__ __forceinline__ double reduce_scatter4_permuted(double (&acc)[4]) {
#pragma unroll
  for (int h2 = 0; h2 < 2; h2++) acc[h2] += dpp_f64<0xB1>(acc[2 + h2]);   // lane ^ 1 (that lane sends its other half: its rows are swapped)
  double tot = acc[0] + dpp_f64<0x4E>(acc[1]);                             // lane ^ 2
  tot += dpp_f64<0x124>(tot);                                              // row_ror:4
  tot += dpp_f64<0x128>(tot);                                              // row_ror:8
  return tot;
}

// Tile-size traits shared by the bodies that run on more than one lane grid: padded group stride of the LDS vectors that are
// read as T-wide groups, the position of row r in such a vector, and the row of its lane-row a lane owns after the reduce.
template <int T> struct TileShape {
  static constexpr int TS = (T == 8) ? 10 : T;
  static __device__ __forceinline__ int pad(const int r) { return (int)(((unsigned)r / (unsigned)T) * (unsigned)TS + ((unsigned)r % (unsigned)T)); }
  static __device__ __forceinline__ int own_a(const int lc) {
    if constexpr (T == 8) return 4 * ((lc >> 2) & 1) + 2 * (lc & 1) + ((lc >> 1) & 1);
    else { static_assert(T == 4, "tile sizes with a DPP reduce-scatter: 8 and 4"); return 2 * (lc & 1) + ((lc >> 1) & 1); }
  }
};

// Symmetric in-register sweep of a T x T-tiled SPD matrix on an LC x LC lane grid: on return tile = -(M^-1) with +2 on every
// diagonal entry (the caller removes it once).  NREAL: rows / columns of M; the rest of the T LC grid is identity padding,
// whose pivot steps change nothing (d = 1, every coefficient 0) and are skipped.  Per pivot the pivot row goes through the
// LDS ping-pong buffer pbuf (2 x (TS LC + 2) doubles, groups of T padded to TS) with entry kp replaced by d - 1, so that one
// unconditional FMA per entry is right for every row (no branches, no dynamic register indexing).  Look-ahead: inside step kp
// the tile row that holds pivot row kp + 1 is updated FIRST and published immediately, so its LDS write -> read latency hides
// behind the other T - 1 row updates.
template <int T, int LG, int NREAL>
__device__ __forceinline__ void tile_sweep(double (&tile)[T][T], double *pbuf, const int lr, const int lc) {
  constexpr int TS = (T == 8) ? 10 : T, LC = 1 << LG, NPAD = TS * LC, NPB = NPAD + 2;
  auto publish = [&](int tr, int kb, double *pb) {   // lanes of lane-row kb publish tile row tr (tr static after unrolling)
    if (lr == kb) {
      const bool diag = (lc == kb);
#pragma unroll
      for (int tb = 0; tb < T; tb += 2) {
        double v0 = tile[tr][tb], v1 = tile[tr][tb + 1];
        if (tb == tr) v0 = diag ? v0 - 1.0 : v0;
        if (tb + 1 == tr) v1 = diag ? v1 - 1.0 : v1;
        *reinterpret_cast<double2 *>(&pb[lc * TS + tb]) = make_double2(v0, v1);
      }
      if (diag) pb[NPAD] = tile[tr][tr];
    }
  };
  publish(0, 0, pbuf);
  __syncthreads();
  for (int kb = 0; kb < LC; kb++) {
#pragma unroll
    for (int tr = 0; tr < T; tr++) {
      const int kp = kb * T + tr;
      if (kp >= NREAL) continue;
      double *pb = pbuf + (kp & 1) * NPB;
      const double invd = fast_rcp(pb[NPAD]);
      double prow[T], pcol[T];
#pragma unroll
      for (int t2 = 0; t2 < T; t2 += 2) {
        double2 a2 = *reinterpret_cast<const double2 *>(&pb[lr * TS + t2]);
        double2 b2 = *reinterpret_cast<const double2 *>(&pb[lc * TS + t2]);
        prow[t2] = a2.x; prow[t2 + 1] = a2.y; pcol[t2] = b2.x; pcol[t2 + 1] = b2.y;
      }
      const int tn = (tr + 1) % T;                // tile row of the next pivot (static)
      const int kbn = (tr + 1 < T) ? kb : kb + 1;  // its lane-row
      {
        const double ncc = -prow[tn] * invd;
#pragma unroll
        for (int tb = 0; tb < T; tb++) tile[tn][tb] = fma(ncc, pcol[tb], tile[tn][tb]);
      }
      if (kp + 1 < NREAL) publish(tn, kbn, pbuf + ((kp + 1) & 1) * NPB);
#pragma unroll
      for (int ta = 0; ta < T; ta++) {
        if (ta == tn) continue;
        // (pivot row itself, ta == tr on lane-row kb: its prow entry is the published d - 1, so -prow/d = 1/d - 1 as required)
        const double ncc = -prow[ta] * invd;
#pragma unroll
        for (int tb = 0; tb < T; tb++) tile[ta][tb] = fma(ncc, pcol[tb], tile[ta][tb]);
      }
#pragma unroll
      for (int ta = 0; ta < T; ta++) pin_row<T>(tile[ta]);
      __syncthreads();
    }
  }
}

// Per-entry build of a T x T register tile of  N (x) GU + S (x) GV + diag I  (m3 x m3 blocks GU / GV in LDS, identity in the
// padding): index divisions and four 8-byte reads per entry -- the build for the lane grids without a branch-free table
// version (build_tile_kron6 covers 8 x 8 tiles of 6 x 6 blocks); with 4 x 4 tiles it is 16 entries per lane.
template <int T, int H, int m3>
__device__ __forceinline__ void build_tile_entries(double (&tile)[T][T], const double *tabN, const double *tabS, const double *GU, const double *GV,
                                                   const int lr, const int lc, const int nreal, const double diag_real) {
#pragma unroll
  for (int ta = 0; ta < T; ta++) {
    const int row = lr * T + ta;
    const int a = row / m3, i = row - a * m3;
    const bool rreal = row < nreal;
    const double *tN = tabN + (rreal ? a : 0) * H, *tS = tabS + (rreal ? a : 0) * H, *gu = GU + (rreal ? i : 0), *gv = GV + (rreal ? i : 0);
#pragma unroll
    for (int tb = 0; tb < T; tb++) {
      const int col = lc * T + tb;
      const int bb = col / m3, j = col - bb * m3;
      double v;
      if (rreal && col < nreal) {
        v = tN[bb] * gu[j * m3] + tS[bb] * gv[j * m3];
        if (col == row) v += diag_real;
      } else v = (col == row) ? 1.0 : 0.0;
      tile[ta][tb] = v;
    }
    __builtin_amdgcn_sched_barrier(0);   // one tile row at a time: bounds the LDS loads in flight (VGPR pressure)
  }
}

// ---- branch-free build of an 8 x 8 register tile of  N (x) U + S (x) V + diag  for 6-wide blocks ----
// The matrix is 2 (N (x) G_U + S (x) G_V) with 6 x 6 blocks (two stance legs in force space, or any leg count in
// wrench space).  A tile row/column range of 8 straddles at most two blocks, always at an even offset, so a lane
// needs four N and four S table values in all, and its 8 x 8 window of the PERIODIC extensions EU, EV of the two
// 6 x 6 matrices ([14][18] doubles in LDS, written by put_periodic6) as 16-byte reads.  ~430 instructions and 72
// LDS reads per lane, no branches; the per-entry version (index divisions, four 8-byte reads and a branch per
// entry) was 1240 instructions and 256 reads -- 10 % of a trot robot's time under load.
#define RG_E6_ROWS 14
#define RG_E6_LD 18
#define RG_E6_DOUBLES (RG_E6_ROWS * RG_E6_LD)
__device__ __forceinline__ void put_periodic6(double *E, const int i, const int j, const double v) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int q = 0; q < 3; q++)
      if (i + 6 * r < RG_E6_ROWS) E[(i + 6 * r) * RG_E6_LD + j + 6 * q] = v;
}
template <int H>
__device__ __forceinline__ void build_tile_kron6(double (&tile)[8][8], const double *tabN, const double *tabS, const double *EU, const double *EV,
                                                 const int lr, const int lc, const int nreal, const double diag_real) {
  const int r0 = 8 * lr, c0 = 8 * lc;
  const int a0r = r0 / 6, i0 = r0 - 6 * a0r, b0r = c0 / 6, j0 = c0 - 6 * b0r;   // i0, j0 in {0, 2, 4}
  const int a0 = a0r < H ? a0r : H - 1, a1 = a0r + 1 < H ? a0r + 1 : H - 1;
  const int b0 = b0r < H ? b0r : H - 1, b1 = b0r + 1 < H ? b0r + 1 : H - 1;
  const double n00 = tabN[a0 * H + b0], n01 = tabN[a0 * H + b1], n10 = tabN[a1 * H + b0], n11 = tabN[a1 * H + b1];
  const double s00 = tabS[a0 * H + b0], s01 = tabS[a0 * H + b1], s10 = tabS[a1 * H + b0], s11 = tabS[a1 * H + b1];
  // Table factor per column pair, for a row in the low / high block.  Column pair p is in the high block iff
  // j0 + 2 p >= 6: never for p = 0, always for p = 3, lane-dependent only for p = 1, 2.
  double nlo[4], nhi[4], slo[4], shi[4];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    if (p == 0) { nlo[p] = n00; nhi[p] = n10; slo[p] = s00; shi[p] = s10; }
    else if (p == 3) { nlo[p] = n01; nhi[p] = n11; slo[p] = s01; shi[p] = s11; }
    else {
      const bool chi = j0 + 2 * p >= 6;
      nlo[p] = chi ? n01 : n00; nhi[p] = chi ? n11 : n10; slo[p] = chi ? s01 : s00; shi[p] = chi ? s11 : s10;
    }
  }
  const double dlane = (lr == lc) ? diag_real : 0.0;
#pragma unroll
  for (int ta = 0; ta < 8; ta++) {
    // row ta is in the high block iff i0 + ta >= 6: never for ta < 2, always for ta >= 6
    const bool rhi = i0 + ta >= 6;
    const double *eu = EU + (i0 + ta) * RG_E6_LD + j0, *ev = EV + (i0 + ta) * RG_E6_LD + j0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const double2 u = *reinterpret_cast<const double2 *>(eu + 2 * p), v = *reinterpret_cast<const double2 *>(ev + 2 * p);
      const double np = ta < 2 ? nlo[p] : (ta >= 6 ? nhi[p] : (rhi ? nhi[p] : nlo[p]));
      const double sp = ta < 2 ? slo[p] : (ta >= 6 ? shi[p] : (rhi ? shi[p] : slo[p]));
      tile[ta][2 * p] = fma(np, u.x, sp * v.x);
      tile[ta][2 * p + 1] = fma(np, u.y, sp * v.y);
    }
    tile[ta][ta] += dlane;
    __builtin_amdgcn_sched_barrier(0);   // one tile row at a time: bounds the LDS loads in flight (VGPR pressure)
  }
  // padding (only the last lane-row / lane-column has any): zero, with 1 on the diagonal
  if (c0 + 8 > nreal) {
#pragma unroll
    for (int tb = 0; tb < 8; tb++)
      if (c0 + tb >= nreal) {
#pragma unroll
        for (int ta = 0; ta < 8; ta++) tile[ta][tb] = 0.0;
      }
  }
  if (r0 + 8 > nreal) {
#pragma unroll
    for (int ta = 0; ta < 8; ta++)
      if (r0 + ta >= nreal) {
#pragma unroll
        for (int tb = 0; tb < 8; tb++) tile[ta][tb] = (ta == tb && lr == lc) ? 1.0 : 0.0;
      }
  }
}

// (M^-1 v)_io on the owner lanes (tile = -M^-1, rows reordered by permute_tile_rows_for_reduce): tile mat-vec, then the DPP reduce-scatter over the lanes of a lane-row
template <int LG>
__device__ __forceinline__ double tile8_matvec(const double (&tile)[8][8], const double *vin_pad, const int lr, const int lc) {
  constexpr int T = 8, TS = 10;
  double acc[T], vloc[T];
#pragma unroll
  for (int t2 = 0; t2 < T; t2 += 2) {
    double2 v2 = *reinterpret_cast<const double2 *>(&vin_pad[lc * TS + t2]);
    vloc[t2] = v2.x; vloc[t2 + 1] = v2.y;
  }
#pragma unroll
  for (int ta = 0; ta < T; ta++) {
    double a0 = 0.0;
#pragma unroll
    for (int tb = 0; tb < T; tb++) a0 = fma(tile[ta][tb], vloc[tb], a0);
    acc[ta] = a0;
  }
  return -reduce_scatter8_permuted<LG>(acc, lc);
}

// ... and for either tile size: T = 8 on 8 x 8 or 16 x 16 lanes, T = 4 on 16 x 16 lanes (rows reordered by the matching permute)
template <int T, int LG>
__device__ __forceinline__ double tile_matvec(const double (&tile)[T][T], const double *vin_pad, const int lr, const int lc) {
  if constexpr (T == 8) return tile8_matvec<LG>(tile, vin_pad, lr, lc);
  else {
    static_assert(T == 4 && LG == 4, "4 x 4 tiles run on the 16 x 16 lane grid");
    const double2 a = *reinterpret_cast<const double2 *>(&vin_pad[lc * 4]), b = *reinterpret_cast<const double2 *>(&vin_pad[lc * 4 + 2]);
    double acc[4];
#pragma unroll
    for (int ta = 0; ta < 4; ta++) acc[ta] = fma(tile[ta][3], b.y, fma(tile[ta][2], b.x, fma(tile[ta][1], a.y, tile[ta][0] * a.x)));
    return -reduce_scatter4_permuted(acc);
  }
}
// a swept 4 x 4 tile, ready for tile_matvec (8 x 8 tiles come out of sym6_to_tile8 finished)
__device__ __forceinline__ void finish_swept_tile4(double (&tile)[4][4], const int lr, const int lc) {
  if (lr == lc) {   // remove the sweep's +2 diagonal offset: tile = -M^-1
#pragma unroll
    for (int ta = 0; ta < 4; ta++) tile[ta][ta] -= 2.0;
  }
  permute_tile_rows_for_reduce4(tile, lc);
}

// Lane grid per horizon: at one horizon every ADMM body runs on the same (1 << LG) x (1 << LG) lanes -- H = 10: one 64-lane
// wave (8 x 8), H = 20: 256 lanes (16 x 16) -- so that one launch can switch body per work item.  T1: tile size of the one-leg body.
template <int H> struct FusedShape;
template <> struct FusedShape<10> { static constexpr int LG = 3, T1 = 4; };   // one leg: 30 -> 32 = 4 x 8
template <> struct FusedShape<20> { static constexpr int LG = 4, T1 = 4; };   // one leg: 60 -> 64 = 4 x 16

// ---- force-space set-up shared by the ADMM body (qp_tile_robot) and the exact body (qp_exact_robot) ----
// From the front->QP record (LDS): B_w = Iw^-1 [r]x per stance-leg force component, T B_w (rpy-rate map), the Gram blocks
// G_U = U' W U, G_V = V' W V (m3 x m3; their periodic extensions when the tile is built by build_tile_kron6) and the two
// per-variable coefficient tables of the linear term: q_(a,i) = 2 sum_{k >= a} [ c1(k,i) + (k - a + 1/2) c2(k,i) ].
// cmask: contact mask whose set bits are the NC stance legs, in order.  Ends with a workgroup barrier.
// GRAM = false: G_U / G_V are left to the caller (two legs on the rank-5 form: force_space_rank5 writes the projected blocks).
template <int NC, int H, int NT, bool KRON6, bool MU4 = false, bool GRAM = true>
__device__ __forceinline__ void force_space_tables(const DevCfg *__restrict__ c, const double *rec, const int cmask, const int tid, double *Bw, double *TBw,
                                                   double *GU, double *GV, double *EU, double *EV, double *c1, double *c2) {
  constexpr int m3 = 3 * NC, N = m3 * H;
  const double dt = c->dt;
  if (tid < m3) {
    int l = nth_leg(cmask, tid / 3), d = tid % 3;
    const double *rr = &rec[REC_FEETW + 3 * l];
    double s0 = (d == 0) ? 0.0 : (d == 1 ? -rr[2] : rr[1]);
    double s1 = (d == 0) ? rr[2] : (d == 1 ? 0.0 : -rr[0]);
    double s2 = (d == 0) ? -rr[1] : (d == 1 ? rr[0] : 0.0);
    const double *Iw = &rec[REC_IWINV];
    double b0 = Iw[0] * s0 + Iw[1] * s1 + Iw[2] * s2;
    double b1 = Iw[3] * s0 + Iw[4] * s1 + Iw[5] * s2;
    double b2 = Iw[6] * s0 + Iw[7] * s1 + Iw[8] * s2;
    Bw[tid] = b0; Bw[m3 + tid] = b1; Bw[2 * m3 + tid] = b2;
    TBw[tid] = rec[REC_INVCP] * b0; TBw[m3 + tid] = b1; TBw[2 * m3 + tid] = rec[REC_TANP] * b0 + b2;
  }
  __syncthreads();
  if constexpr (GRAM)
  for (int e = tid; e < m3 * m3; e += NT) {
    int i = e / m3, j = e % m3;
    double gu = c->w[6] * Bw[i] * Bw[j] + c->w[7] * Bw[m3 + i] * Bw[m3 + j] + c->w[8] * Bw[2 * m3 + i] * Bw[2 * m3 + j];
    double gv = c->w[0] * TBw[i] * TBw[j] + c->w[1] * TBw[m3 + i] * TBw[m3 + j] + c->w[2] * TBw[2 * m3 + i] * TBw[2 * m3 + j];
    if (i % 3 == j % 3) { gu += c->w[9 + i % 3] * body_val<MU4>(c, rec, BODY_INV_MASS) * body_val<MU4>(c, rec, BODY_INV_MASS); gv += c->w[3 + i % 3] * body_val<MU4>(c, rec, BODY_INV_MASS) * body_val<MU4>(c, rec, BODY_INV_MASS); }
    GU[e] = gu * dt * dt;
    GV[e] = gv * dt * dt * dt * dt;
    if constexpr (KRON6) { put_periodic6(EU, i, j, GU[e]); put_periodic6(EV, i, j, GV[e]); }
  }
  for (int e = tid; e < N; e += NT) {
    int a = e / m3, i = e % m3;
    double kd = (double)(a + 1) * dt;
    const double *om = &rec[REC_OMEGA], *vb = &rec[REC_VBODY], *cm = &rec[REC_CMD];
    double e_r = rec[REC_ROLL] + kd * rec[REC_INVCP] * om[0];
    double e_p = rec[REC_PITCH] + kd * om[1];
    double e_y = kd * (rec[REC_TANP] * om[0] + om[2]) - kd * cm[2];
    double e_x = kd * vb[0] - kd * cm[0];
    double e_yy = kd * vb[1] - kd * cm[1];
    double e_z = rec[REC_COMZ] + kd * vb[2] - 0.5 * kd * kd * c->g - body_val<MU4>(c, rec, BODY_HEIGHT);
    double e_w0 = om[0], e_w1 = om[1], e_w2 = om[2] - cm[2];
    double e_v0 = vb[0] - cm[0], e_v1 = vb[1] - cm[1], e_v2 = vb[2] - kd * c->g;
    int d = i % 3;
    double ev = (d == 0) ? c->w[9] * e_v0 : (d == 1 ? c->w[10] * e_v1 : c->w[11] * e_v2);
    double ep = (d == 0) ? c->w[3] * e_x : (d == 1 ? c->w[4] * e_yy : c->w[5] * e_z);
    c1[e] = dt * (Bw[i] * c->w[6] * e_w0 + Bw[m3 + i] * c->w[7] * e_w1 + Bw[2 * m3 + i] * c->w[8] * e_w2 + body_val<MU4>(c, rec, BODY_INV_MASS) * ev);
    c2[e] = dt * dt * (TBw[i] * c->w[0] * e_r + TBw[m3 + i] * c->w[1] * e_p + TBw[2 * m3 + i] * c->w[2] * e_y + body_val<MU4>(c, rec, BODY_INV_MASS) * ep);
  }
}

// ---- two stance legs: the direction of force space in which P is alpha, taken out before the sweep ----
// With the stance feet at r1, r2 and e = (r1 - r2) / |r1 - r2| the force pair n = (e, -e) / sqrt 2 has no net force and no net
// torque: B_w n = Iw^-1 ((r1 - r2) x e) / sqrt 2 = 0 and (e - e) / m = 0, so G_U n = G_V n = 0 and P = 2 (N (x) G_U + S (x) G_V)
// + alpha I is alpha in the ten directions (step k) (x) n.  With Q = I - beta v v', v = n + sign(n_5) e_6, beta = 2 / v'v =
// 1 / (1 + |n_5|) (v'v >= 2: no cancellation) the reflector that maps e_6 to -+n, and Q5 its first five columns,
//     P^-1 = (I (x) Q5) (alpha I + 2 N (x) Q5' G_U Q5 + 2 S (x) Q5' G_V Q5)^-1 (I (x) Q5') + I (x) n n' / alpha:
// only a 5 NB x 5 NB matrix is swept (sym6_sweep<.., 5>) and sym5_back_transform puts the sixth direction back.
// Two halves around force_space_tables<2, .., GRAM = false>, and no stage of their own (each stage is a barrier and an LDS round
// trip of a job that nobody overlaps):
//   force_space_reflector, BEFORE it: the reflector depends on the two stance feet only, so it is built in the stage that builds
//     B_w / T B_w and published by that stage's barrier.  hv (RG_RANK5_HV doubles, 8 used): v[0..5], beta, 2 - 1 / alpha (what the
//     sweep's result has in the sixth direction of a diagonal block).
//   force_space_rank5, AFTER it, next to the linear term's tables: writes GU / GV, the projected Gram blocks, built from B_w Q5,
//     T B_w Q5 and [I I] Q5 -- so that the dropped sixth row and column are zero by construction, not by cancellation -- and padded
//     to 6 x 6 with zeros (sym6_build_kron6 keeps its addresses).  Every lane that owns an entry takes the nine projections
//     beta (B_w v), beta (T B_w v), beta ([I I] v) itself (36 FMAs on broadcast reads; they used to be a stage of nine lanes).
//     The caller's barrier follows.
// Coincident feet (or a difference that is not finite) take e = x: any unit e is right there, the null space only grows.
constexpr int RG_RANK5_HV = 18;   // doubles of hv (even: what follows it in a layout stays 16-byte aligned)
static_assert(8 <= RG_RANK5_HV && RG_RANK5_HV % 2 == 0, "hv holds v, beta and 2 - 1 / alpha");
__device__ __forceinline__ void force_space_reflector(const DevCfg *__restrict__ c, const double *rec, const int cmask, const int tid, double *hv_) {
  // (the odd forms: see force_space_rank5)
  int opaque0 = 0;
  asm volatile("" : "+v"(opaque0));
  double *hv = hv_ + opaque0;
  if (tid < 8) {
    const double *r1 = &rec[REC_FEETW + 3 * nth_leg(cmask, 0)], *r2 = &rec[REC_FEETW + 3 * nth_leg(cmask, 1)];
    double e0 = r1[0] - r2[0], e1 = r1[1] - r2[1], e2 = r1[2] - r2[2];
    double d2 = 2.0 * fma(e0, e0, fma(e1, e1, e2 * e2));
    if (!(d2 > 0.0 && (d2 - d2) == 0.0)) { e0 = 1.0; e1 = 0.0; e2 = 0.0; d2 = 2.0; }   // coincident feet, or a difference that is not finite: e = x
    // y = 1 / sqrt(2 |r1 - r2|^2): n = (r1 - r2, r2 - r1) y
    double y = __builtin_amdgcn_rsq(d2);
#pragma unroll
    for (int it = 0; it < 2; it++) { const double er = fma(-d2 * y, y, 1.0); y = fma(0.5 * y, er, y); }
    const double n5 = -e2 * y;
    const int a = tid % 3;
    const double ea = a == 0 ? e0 : (a == 1 ? e1 : e2);
    double o = tid < 3 ? ea * y : -ea * y;                           // n
    if (tid == 5) o += n5 < 0.0 ? -1.0 : 1.0;                        // v = n + sign(n_5) e_6
    if (tid == 6) o = 1.0 / (1.0 + fabs(n5));                        // beta
    if (tid == 7) o = 2.0 - 1.0 / c->alpha;
    hv[tid] = o;
  }
}
template <int NT, bool MU4 = false>
__device__ __forceinline__ void force_space_rank5(const DevCfg *__restrict__ c, const double *rec, const int tid, const double *Bw_, const double *TBw_,
                                                  double *GU_, double *GV_, double *hv_) {
  constexpr int m3 = 6;
  // KEEP the odd forms below; tests/test_kernel_resources.py fails without them.  Whatever is loop-invariant in this helper is
  // hoisted out of the re-solve kernel's work loop (rg_qp_resolve_kernel) and held in VGPRs across its robots: with M_SQRT1_2,
  // INFINITY and the LDS addresses as literals that kernel needed 8 VGPRs more (231 -> 239), with a byte compare of i % 3 one
  // more (LAB_NOTES).  So: every LDS address is one opaque register (a zero the compiler cannot see through) plus a constant;
  // the only floating-point constants are inline ones (0.5, 1.0, 2.0), which occupy no register -- 1 / sqrt 2 comes out of
  // v_rsq_f64 and two Newton steps, finiteness is tested as d2 - d2 == 0; i % 3 is made an opaque 32-bit value.
  int opaque0 = 0;
  asm volatile("" : "+v"(opaque0));
  double *hv = hv_ + opaque0;
  const double *Bw = hv + (Bw_ - hv_), *TBw = hv + (TBw_ - hv_);
  double *GU = hv + (GU_ - hv_), *GV = hv + (GV_ - hv_);
  for (int e = tid; e < m3 * m3; e += NT) {
    const int i = e / m3, j = e % m3;
    double gu = 0.0, gv = 0.0;
    if (i < 5 && j < 5) {
      const double vi = hv[i], vj = hv[j];
      double pb[3], pt[3], pe[3];   // beta (B_w v), beta (T B_w v), beta ([I I] v)
#pragma unroll
      for (int r = 0; r < 3; r++) {
        double sb = Bw[r * m3] * hv[0], st = TBw[r * m3] * hv[0];
#pragma unroll
        for (int k = 1; k < m3; k++) { sb = fma(Bw[r * m3 + k], hv[k], sb); st = fma(TBw[r * m3 + k], hv[k], st); }
        pb[r] = hv[6] * sb; pt[r] = hv[6] * st; pe[r] = hv[6] * (hv[r] + hv[3 + r]);
      }
      const double im2 = body_val<MU4>(c, rec, BODY_INV_MASS) * body_val<MU4>(c, rec, BODY_INV_MASS);
      const double *cw = c->w;
      int ia = i % 3, ja = j % 3;
      asm volatile("" : "+v"(ia), "+v"(ja));   // (32-bit compares against inline constants: a byte compare takes its constant from a register)
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const double bi = fma(-pb[r], vi, Bw[r * m3 + i]), bj = fma(-pb[r], vj, Bw[r * m3 + j]);
        const double ti = fma(-pt[r], vi, TBw[r * m3 + i]), tj = fma(-pt[r], vj, TBw[r * m3 + j]);
        const double ei = fma(-pe[r], vi, ia == r ? 1.0 : 0.0), ej = fma(-pe[r], vj, ja == r ? 1.0 : 0.0);
        gu = fma(cw[6 + r] * bi, bj, fma(cw[9 + r] * im2 * ei, ej, gu));
        gv = fma(cw[r] * ti, tj, fma(cw[3 + r] * im2 * ei, ej, gv));
      }
    }
    const double dt = c->dt;
    GU[e] = gu * dt * dt;
    GV[e] = gv * dt * dt * dt * dt;
  }
}
