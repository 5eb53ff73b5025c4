// rg_qp_sym6.inc -- the symmetric sweep with every 6 x 6 block of the matrix held ONCE, and the move of its result into the
// 8 x 8-tile layout of the solver loops' mat-vec.
// Included by rg_mpc.hip (single translation unit); not a stand-alone header.
#pragma once

// ------------------------------------------------------------------------------------
// Every QP body starts by inverting a symmetric positive definite 6 NB x 6 NB matrix whose natural unit is a 6 x 6 block
// (force space, two stance legs: P, block = a pair of horizon steps; wrench space: a I + K').  tile_sweep
// (rg_qp_tile.inc) holds it as LC x LC lanes x 8 x 8 register tiles, i.e. BOTH triangles: lanes (r, c) and (c, r)
// compute the same 64 numbers -- 64 FMAs, 8 coefficient products and 16 doubles from LDS per lane and pivot, and the sweep
// was 45 % of the wave-slot time of the headline launch (profiles/r5_launch_schedule.txt).
//
// Here lane t holds ONE block (br, bc), br >= bc, of the lower block triangle: NB (NB + 1) / 2 lanes (55 of 64 for NB = 10;
// 210 of 256 for NB = 20), 36 FMAs, 6 coefficient products and 12 doubles from LDS per lane and pivot, 72 VGPRs of matrix
// instead of 128.  The elimination is the one of tile_sweep, step for step: pivot k changes entry (i, j) by -p_i p_j / d with
// p the pivot row, which by symmetry is also the pivot column, so ONE published vector serves the rows and the columns of
// every block; it is collected from the blocks of block-row kb (their row ko) and of block-column kb (their column ko), with
// entry k replaced by d - 1 so that one unconditional FMA per entry is right for every row.  A diagonal block keeps all its
// 36 entries (both triangles), so it needs no special case.  One block per lane -- not two 4 x 4 tiles in two orientations,
// the round-4 experiment (tests/studies/symmetric_sweep_experiment.inc) whose publish cost more instructions than the FMAs
// it saved -- and three more things that experiment did not have:
//   * no row-or-column select per pivot: a lane below the block diagonal starts with the mirror image of its block and turns
//     it over once (sym6_sweep, below);
//   * the pivot row of step k + 1 is READ in step k, right after it was published, into a second register set (the 56 VGPRs
//     the smaller matrix frees): its LDS round trip and the reciprocal's Newton steps hide behind the rest of step k;
//   * the move into the 8 x 8 tiles is a plain gather: every lane stores its block once, row-contiguous, and reads its 64
//     entries from where they are; the reduce-scatter's row order (permute_tile_rows_for_reduce: 256 v_cndmask) and the
//     removal of the sweep's +2 diagonal offset are folded into the addresses / the store, so the move costs about the
//     vector instructions the row permutation alone used to.
// Measured (tests/studies/sweep_bench.hip, profiles/r6_sweep_bench_study.txt; build + inversion + move, 60 x 60, us per robot):
// 16.4 -> 14.9 alone, 28.1 -> 24.3 with two waves per SIMD; its floor without any LDS traffic is 17.2 under load, the three
// ds_write_b128 of a pivot cost 4.7 and reading them back 2.4.  A CPU model of the index algebra: tests/test_sym6_model.py.
// Two stance legs in force space sweep only the 5 x 5 corners of their blocks (sym6_sweep<.., 5>, sym5_back_transform below; CPU
// model: tests/test_sym5_model.py).
// ------------------------------------------------------------------------------------

template <int NB> struct Sym6 {
  static constexpr int NBLK = NB * (NB + 1) / 2;   // lanes that hold a block
  static constexpr int DS = 6 * NB;                // slot of the pivot d behind the pivot vector
  static constexpr int PB = 6 * NB + 2;            // doubles per pivot buffer (two of them: ping-pong; three for the five-wide sweep)
  static constexpr int PB2 = 12 * NB + 4;          // ... of the two-pivot form: two rows and the 2 x 2 pivot block
  static constexpr int STG = NBLK * 36;            // doubles of the staging area of sym6_to_tile8
};

// Block (br, bc), br >= bc, of lane t: block-rows r and NB - 1 - r hold NB + 1 blocks together and share NB + 1 consecutive
// lanes.  Lanes beyond the triangle hold no block (`on` false; they run the arithmetic on zeros and never store).
template <int NB>
__device__ __forceinline__ void sym6_lane(const int t, int &br, int &bc, bool &on) {
  const int pair = (int)((unsigned)t / (unsigned)(NB + 1)), off = t - pair * (NB + 1);
  on = t < Sym6<NB>::NBLK;
  const bool lo = off <= pair;
  br = on ? (lo ? pair : NB - 1 - pair) : 0;
  bc = on ? (lo ? off : off - pair - 1) : 0;
}

// A = tN[br][bc] U + tS[br][bc] V + diag I (diagonal blocks) for 6 x 6 U, V in LDS (row-major; every lane reads the same
// addresses: broadcasts); tabN / tabS: the H x H horizon tables (already doubled).  One table value each per lane.
template <int H>
__device__ __forceinline__ void sym6_build_kron6(double (&A)[6][6], const double *tabN, const double *tabS, const double *U, const double *V,
                                                 const int br, const int bc, const bool on, const double diag) {
  const double n = on ? tabN[br * H + bc] : 0.0, s = on ? tabS[br * H + bc] : 0.0;
  const double dl = (on && br == bc) ? diag : 0.0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int b = 0; b < 6; b += 2) {
      const double2 u = *reinterpret_cast<const double2 *>(U + a * 6 + b), v = *reinterpret_cast<const double2 *>(V + a * 6 + b);
      A[a][b] = fma(n, u.x, s * v.x);
      A[a][b + 1] = fma(n, u.y, s * v.y);
    }
    A[a][a] += dl;
  }
}
// ... the same for 3 x 3 U, V (one stance leg in force space): a 6 x 6 block is 2 x 2 horizon steps
template <int H>
__device__ __forceinline__ void sym6_build_kron3(double (&A)[6][6], const double *tabN, const double *tabS, const double *U, const double *V,
                                                 const int br, const int bc, const bool on, const double diag) {
  double n[2][2], s[2][2];
#pragma unroll
  for (int x = 0; x < 2; x++)
#pragma unroll
    for (int y = 0; y < 2; y++) { n[x][y] = on ? tabN[(2 * br + x) * H + 2 * bc + y] : 0.0; s[x][y] = on ? tabS[(2 * br + x) * H + 2 * bc + y] : 0.0; }
  const double dl = (on && br == bc) ? diag : 0.0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int b = 0; b < 6; b++) A[a][b] = fma(n[a / 3][b / 3], U[(a % 3) * 3 + b % 3], s[a / 3][b / 3] * V[(a % 3) * 3 + b % 3]);
    A[a][a] += dl;
  }
}

template <int NT>
__device__ __forceinline__ void sym6_sync() {
  // one wave: its LDS operations execute in order, the pivot vector needs no barrier -- only the compiler must keep the order
  if constexpr (NT == 64) asm volatile("" ::: "memory"); else __syncthreads();
}

// lane that holds block (r, c), r >= c (the inverse of sym6_lane)
template <int NB>
__device__ __forceinline__ int sym6_lane_of(const int r, const int c) {
  return (2 * r <= NB - 1) ? r * (NB + 1) + c : (NB - 1 - r) * (NB + 2) + 1 + c;
}
// ---- the form that ships: no orientation select ----
// A lane below the block diagonal hands on a COLUMN of its block while the pivots run through its block-column (kb == bc) and
// a ROW once they reach its block-row (kb == br > bc).  Selecting row or column per pivot costs 11 v_cndmask and puts the
// column's five FMAs on the critical path.  Instead every such lane starts with the MIRROR IMAGE of its block, X = block'
// ("row group" gr = bc, "column group" gc = br: the update X[a][b] -= p[6 gr + a] p[6 gc + b] / d is the same statement with
// the two groups exchanged), so that what it hands on is a row of X in both phases, and transposes X in place (30 v_swap,
// once, when the pivots reach its block-row: the lanes with br == kb + 1 in front of pivot (kb, 5), whose successor they
// publish).  The caller builds X as block (gr, gc) of the symmetric matrix (sym6_groups) -- for the Kronecker bodies the
// blocks are symmetric themselves.  Publisher: gr == kb; destination: entries 6 gc .. 6 gc + 5; always row ko of X.
template <int NB>
__device__ __forceinline__ void sym6_groups(const int br, const int bc, int &gr, int &gc) { gr = bc; gc = br; }

// W: the active edge of every block.  W = 6 is the sweep above.  W = 5 sweeps the 5 NB x 5 NB matrix whose blocks are the leading
// 5 x 5 corners of X (two stance legs in force space: the sixth direction of every block is known in closed form, see
// force_space_rank5 / sym5_back_transform): five rows, five columns and five pivots per block row, the turn-over in front of pivot
// (kb, 4).  Lanes, groups of six doubles in the pivot buffers (the sixth slot is padding) and the 16-byte stores stay as they
// are; row 5 and column 5 of X are neither read nor written.  Five pivots per block row have no parity to pick the buffer by,
// so this form rotates through THREE buffers (pivot ko of a block row: 0, 1, 0, 1, 2 -- static, and no two pivots in a row
// share one, which is all the ping-pong is for).
template <int W> __device__ __forceinline__ constexpr int sym6_buf(const int ko) { return (W == 5 && ko == 4) ? 2 : (ko & 1); }

template <int NB, int NBR, int NT, int W = 6>
__device__ __forceinline__ void sym6_sweep(double (&X)[6][6], double *pbuf, const int br, const int bc, const bool on) {
  static_assert(W == 6 || W == 5, "blocks are swept whole or without their sixth row and column");
  constexpr int PB = Sym6<NB>::PB, DS = Sym6<NB>::DS;
  int gr = bc, gc = br;
  auto publish = [&](const int ko, const int kb, double *pb) {
    if (on && gr == kb) {
      const bool dg = gc == kb;
      double *dst = pb + 6 * gc;
      double w[6];
#pragma unroll
      for (int e = 0; e < 6; e++) w[e] = e < W ? X[ko][e] : 0.0;
      if constexpr (NT > 64) { if (dg) pb[DS] = w[ko]; }
      w[ko] -= dg ? 1.0 : 0.0;
#pragma unroll
      for (int e = 0; e < 6; e += 2) *reinterpret_cast<double2 *>(dst + e) = make_double2(w[e], w[e + 1]);
    }
  };
  auto fetch = [&](const double *pb, double (&pr)[6], double (&pc)[6], double &d) {
    if constexpr (NT > 64) d = pb[DS];
#pragma unroll
    for (int e = 0; e < 6; e += 2) {
      const double2 a2 = *reinterpret_cast<const double2 *>(pb + 6 * gr + e), b2 = *reinterpret_cast<const double2 *>(pb + 6 * gc + e);
      pr[e] = a2.x; pr[e + 1] = a2.y; pc[e] = b2.x; pc[e + 1] = b2.y;
    }
  };
  auto pivot = [&](const int ko, const int kb) -> double {   // one wave: d straight from the diagonal block's lane
    const int kk = kb < NB ? kb : NB - 1, t = sym6_lane_of<NB>(kk, kk);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(X[ko][ko]), t), __builtin_amdgcn_readlane(__double2loint(X[ko][ko]), t));
  };
  double pr[6], pc[6], d = 0.0;
  if constexpr (NT == 64) d = pivot(0, 0);
  publish(0, 0, pbuf);
  sym6_sync<NT>();
  fetch(pbuf, pr, pc, d);
  double invd = fast_rcp(d);
  for (int kb = 0; kb < NBR; kb++) {
#pragma unroll
    for (int ko = 0; ko < W; ko++) {
      const int kon = (ko + 1) % W;                   // row of the next pivot inside its blocks (static)
      const int kbn = (ko == W - 1) ? kb + 1 : kb;    // its block row
      if (ko == W - 1) {
        // the lanes of block-row kb + 1 turn their block over before they publish its first row (their column phase is over)
        if (on && br == kb + 1 && gr != br) {
#pragma unroll
          for (int a = 0; a < W; a++)
#pragma unroll
            for (int b = a + 1; b < W; b++) { const double t = X[a][b]; X[a][b] = X[b][a]; X[b][a] = t; }
#pragma unroll
          for (int e = 0; e < W; e++) { const double t = pr[e]; pr[e] = pc[e]; pc[e] = t; }
          gr = br; gc = bc;
        }
      }
      // the next pivot row first: its diagonal entry (the next pivot d: its reciprocal's chain starts from here), then the
      // rest of row kon ...   (-p / d of the pivot row itself: its entry is the published d - 1, so 1 / d - 1 as required)
      const double nk = -pr[kon] * invd;
      X[kon][kon] = fma(nk, pc[kon], X[kon][kon]);
      double npr[6], npc[6], nd = 0.0;
      if constexpr (NT == 64) nd = pivot(kon, kbn);
#pragma unroll
      for (int b = 0; b < W; b++) if (b != kon) X[kon][b] = fma(nk, pc[b], X[kon][b]);
      // ... handed on and read back at once (after the last pivot: nobody publishes, the read returns old finite values)
      double *pbn = pbuf + sym6_buf<W>(kon) * PB;   // W = 6: pivot k = 6 kb + ko, k & 1 == ko & 1
      publish(kon, kbn, pbn);
      sym6_sync<NT>();
      fetch(pbn, npr, npc, nd);
      // the other rows, with the dependent steps of 1 / d (next pivot) spread between them: a lone wave issues in
      // order, and behind the rows the chain would add its full latency to every pivot
      __builtin_amdgcn_sched_barrier(0);
      double xr = __builtin_amdgcn_rcp(nd), er = 0.0;
      asm volatile("" : "+v"(xr));   // (pins the step here: left alone the optimiser sinks the whole chain behind the rows)
      int row = 0;
#pragma unroll
      for (int a = 0; a < W; a++) {
        if (a == kon) continue;
        const double na = -pr[a] * invd;
#pragma unroll
        for (int b = 0; b < W; b++) X[a][b] = fma(na, pc[b], X[a][b]);
        __builtin_amdgcn_sched_barrier(0);
        if (row == 0 || row == 2) { er = fma(-nd, xr, 1.0); asm volatile("" : "+v"(er)); }
        if (row == 1 || row == 3) { xr = fma(xr, er, xr); asm volatile("" : "+v"(xr)); }
        row++;
      }
#pragma unroll
      for (int a = 0; a < W; a++) {
        if constexpr (W == 6) asm volatile("" : "+v"(X[a][0]), "+v"(X[a][1]), "+v"(X[a][2]), "+v"(X[a][3]), "+v"(X[a][4]), "+v"(X[a][5]));
        else asm volatile("" : "+v"(X[a][0]), "+v"(X[a][1]), "+v"(X[a][2]), "+v"(X[a][3]), "+v"(X[a][4]));
      }
#pragma unroll
      for (int e = 0; e < W; e++) { pr[e] = npr[e]; pc[e] = npc[e]; }
      invd = xr;
    }
  }
}

// ---- two stance legs in force space: the swept 5 x 5 blocks back into the 6 x 6 blocks of -G + 2 I ----
// After sym6_sweep<.., 5> on P5 = alpha I + 2 N (x) (Q5' G_U Q5) + 2 S (x) (Q5' G_V Q5) (force_space_rank5, rg_qp_tile.inc) a lane
// holds the 5 x 5 block M of -P5^-1 (+ 2 I on diagonal blocks) in the leading corner of X.  With Q = I - beta v v' the reflector
// whose first five columns are Q5 and whose sixth is -+n, the direction in which P is alpha:
//     block of -P^-1 (+ 2 I) = Q [ M 0 ; 0 c ] Q,   c = 2 - 1 / alpha on diagonal blocks, 0 elsewhere
//                            = M6 - v w~' - u~ v',  u~ = beta M6 v,  w~ = beta M6' v - beta^2 (v' M6 v) v.
// In place: two mat-vecs, then two FMAs per entry; no second block is live.  hv (LDS, per robot): v[0..5], beta, 2 - 1 / alpha.
__device__ __forceinline__ void sym5_back_transform(double (&X)[6][6], const double *hv, const int br, const int bc, const bool on) {
  double v[6];
#pragma unroll
  for (int e = 0; e < 6; e += 2) { const double2 t = *reinterpret_cast<const double2 *>(hv + e); v[e] = t.x; v[e + 1] = t.y; }
  const double2 bc2 = *reinterpret_cast<const double2 *>(hv + 6);
  const double beta = bc2.x, c55 = (on && br == bc) ? bc2.y : 0.0;
  double u[6], w[6];
#pragma unroll
  for (int a = 0; a < 5; a++) {
    double t = X[a][0] * v[0];
#pragma unroll
    for (int b = 1; b < 5; b++) t = fma(X[a][b], v[b], t);
    u[a] = t;
  }
#pragma unroll
  for (int b = 0; b < 5; b++) {
    double t = X[0][b] * v[0];
#pragma unroll
    for (int a = 1; a < 5; a++) t = fma(X[a][b], v[a], t);
    w[b] = t;
  }
  u[5] = c55 * v[5]; w[5] = u[5];
  double s = u[0] * v[0];
#pragma unroll
  for (int a = 1; a < 6; a++) s = fma(u[a], v[a], s);
  const double b2s = beta * beta * s;
#pragma unroll
  for (int e = 0; e < 6; e++) { u[e] *= beta; w[e] = fma(beta, w[e], -b2s * v[e]); }
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) {
      const double m = (a < 5 && b < 5) ? X[a][b] : ((a == 5 && b == 5) ? c55 : 0.0);
      X[a][b] = fma(-v[a], w[b], fma(-u[a], v[b], m));
    }
}

// floor(i / 6) for 0 <= i <= 130 (the callers stay below 128: rows / columns of a 16 x 16 grid of 8 x 8 tiles)
__device__ __forceinline__ int div6_u8(const int i) { return (i * 43) >> 8; }

// The swept matrix -> LC x LC lanes x 8 x 8 tiles for tile8_matvec: tile row ta of lane (lr, lc) gets matrix row
// 8 lr + (ta ^ perm(lc)) -- the order reduce_scatter8_permuted expects --, columns 8 lc .. 8 lc + 7, with the sweep's +2
// diagonal offset removed.  Rows / columns beyond 6 NBR (the padding of the 8-wide grid) read entries of the last block row
// instead: finite numbers that meet zeros of the mat-vec input or land in rows nobody reads.
// stg: Sym6<NB>::STG doubles of LDS nobody else uses during the call; blocks are stored whole, row-major, block (r, c) at
// (r (r + 1) / 2 + c) * 36.  An entry (i, j) with block(i) >= block(j) is read from block (block(i), block(j)) at
// [i % 6][j % 6], otherwise from the mirror image.  Per lane the choice depends on the row only: lanes below the lane
// diagonal read "lower", lanes above it "mirrored", and in a diagonal lane the rows of its first block read mirrored
// (their own diagonal block is symmetric, so the mirror image is as good there), the rows of its second block lower.
template <int NB, int NBR, int LG, int NT>
__device__ __forceinline__ void sym6_to_tile8(const double (&A)[6][6], const int br, const int bc, const bool on, double (&tile)[8][8], double *stg, const int lane) {
  constexpr int LC = 1 << LG;
  __syncthreads();   // the staging area is free
  if (on) {
    double *dst = stg + (br * (br + 1) / 2 + bc) * 36;
    const double off = (br == bc) ? 2.0 : 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 6; b += 2)
        *reinterpret_cast<double2 *>(dst + a * 6 + b) = make_double2(b == a ? A[a][b] - off : A[a][b], b + 1 == a ? A[a][b + 1] - off : A[a][b + 1]);
  }
  __syncthreads();
  const int lr = lane >> LG, lc = lane & (LC - 1), perm = ((lc & 1) << 1) | (lc & 4);
  // column parts of the address (in doubles): lower form jb * 36 + ja, mirrored form tri(jb) * 36 + 6 ja
  int cl[8], cm[8];
#pragma unroll
  for (int tb = 0; tb < 8; tb++) {
    const int j = 8 * lc + tb, q = div6_u8(j), ja = j - 6 * q, jb = q < NBR ? q : NBR - 1;
    cl[tb] = jb * 36 + ja;
    cm[tb] = (jb * (jb + 1) / 2) * 36 + 6 * ja;
  }
  const int rsplit = 6 * (div6_u8(8 * lr) + 1);   // first row of the second block of this lane-row's row range
#pragma unroll
  for (int ta = 0; ta < 8; ta++) {
    const int i = 8 * lr + (ta ^ perm), q = div6_u8(i), ia = i - 6 * q, ib = q < NBR ? q : NBR - 1;
    const bool mir = lr < lc || (lr == lc && i < rsplit);
    const int rpart = mir ? ib * 36 + ia : (ib * (ib + 1) / 2) * 36 + 6 * ia;
#pragma unroll
    for (int tb = 0; tb < 8; tb++) tile[ta][tb] = stg[rpart + (mir ? cm[tb] : cl[tb])];
  }
}
