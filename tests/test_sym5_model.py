"""CPU model of the two-leg exact body's rank-5 inversion (robot_gym_amd/csrc: force_space_rank5 in rg_qp_tile.inc,
sym6_sweep<.., 5> and sym5_back_transform in rg_qp_sym6.inc), lane by lane in numpy, in the style of test_sym6_model.py.

With two stance feet at r1, r2 the force pair n = (e, -e) / sqrt 2, e = (r1 - r2) / |r1 - r2|, has no net force and no net
torque: G_U n = G_V n = 0, so P = 2 (N (x) G_U + S (x) G_V) + alpha I is alpha along (step k) (x) n.  The kernel reflects e_6 onto
-+n (Q = I - beta v v'), sweeps the 5 NB x 5 NB matrix alpha I + 2 N (x) Q5' G_U Q5 + 2 S (x) Q5' G_V Q5 with every block held
once -- the turn-over sweep of test_sym6_model.py with five rows, columns and pivots per block row, the turn-over in front
of pivot (kb, 4), three pivot buffers instead of two -- and turns every swept 5 x 5 block back into its 6 x 6 block of
-P^-1 (+ 2 I).  Modelled here: the set-up (reflector, projected Gram blocks built from B_w Q5, T B_w Q5, [I I] Q5), the
five-wide sweep at NB = 5, 10 and 20, the back-transform and (8 x 8 lanes) the gather into the 8 x 8 tiles; the result is
-inv(P) entry for entry, to the bound test_sym6_model.py holds the six-wide model to.
What it accelerates: reference controllers/mpc/mpc_controller.py:102-106 (the QP solve inside get_action)."""
import numpy as np
import pytest

from tests.test_sym6_model import div6_u8, sym6_lane

W_GHOST = (5, 5, 0.2, 0, 0, 10, 0.5, 0.5, 0.2, 0.2, 0.2, 0.1)   # MPCConfig.weights[:12]
ALPHA, DT, MASS = 1e-5, 0.025, 190 / 9.8
INERTIA = np.diag([0.07335, 0.25068, 0.25447])


def skew(r):
    return np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])


def force_space_tables(r1, r2, rpy, w=W_GHOST):
    """B_w (3 x 6), T B_w, G_U, G_V as force_space_tables builds them for two stance legs (per-step Gram blocks)."""
    roll, pitch, yaw = rpy
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Iw_inv = np.linalg.inv(R @ INERTIA @ R.T)
    Bw = np.hstack([Iw_inv @ skew(r1), Iw_inv @ skew(r2)])
    invcp, tanp = 1.0 / np.cos(pitch), np.tan(pitch)
    TBw = np.vstack([invcp * Bw[0], Bw[1], tanp * Bw[0] + Bw[2]])
    E = np.hstack([np.eye(3), np.eye(3)])
    im2 = 1.0 / MASS ** 2
    GU = (Bw.T @ np.diag(w[6:9]) @ Bw + im2 * E.T @ np.diag(w[9:12]) @ E) * DT ** 2
    GV = (TBw.T @ np.diag(w[0:3]) @ TBw + im2 * E.T @ np.diag(w[3:6]) @ E) * DT ** 4
    return Bw, TBw, GU, GV


def horizon_tables(H):
    """The doubled horizon tables 2 N, 2 S of load_horizon_tables (tests/studies/sweep_bench.hip builds the same)."""
    N, S = np.zeros((H, H)), np.zeros((H, H))
    for a in range(H):
        for b in range(H):
            m = max(a, b)
            N[a, b] = 2.0 * (H - m)
            S[a, b] = 2.0 * sum((k - a - 0.5) * (k - b - 0.5) for k in range(m + 1, H + 1))
    return N, S


def force_space_rank5(r1, r2, Bw, TBw, w=W_GHOST):
    """The kernel's set-up: v, beta and the projected Gram blocks, padded to 6 x 6 with a zero sixth row and column."""
    e = r1 - r2
    d2 = 2.0 * float(e @ e)
    if not (d2 > 0.0 and np.isfinite(d2)):
        e, d2 = np.array([1.0, 0.0, 0.0]), 2.0
    y = 1.0 / np.sqrt(d2)
    n = np.concatenate([e, -e]) * y
    v = n.copy()
    v[5] += -1.0 if n[5] < 0.0 else 1.0
    beta = 1.0 / (1.0 + abs(n[5]))
    E = np.hstack([np.eye(3), np.eye(3)])
    im2 = 1.0 / MASS ** 2
    proj = lambda M: M - beta * np.outer(M @ v, v)              # M Q, row by row
    BQ, TQ, EQ = proj(Bw), proj(TBw), proj(E)
    GU5, GV5 = np.zeros((6, 6)), np.zeros((6, 6))
    for i in range(5):
        for j in range(5):
            GU5[i, j] = (sum(w[6 + r] * BQ[r, i] * BQ[r, j] + w[9 + r] * im2 * EQ[r, i] * EQ[r, j] for r in range(3))) * DT ** 2
            GV5[i, j] = (sum(w[r] * TQ[r, i] * TQ[r, j] + w[3 + r] * im2 * EQ[r, i] * EQ[r, j] for r in range(3))) * DT ** 4
    return v, beta, GU5, GV5, n


def buf_of(ko):
    return 2 if ko == 4 else ko & 1


def sweep5_model(M6, nb):
    """The lanes' 6 x 6 registers after the five-wide turn-over sweep of the matrix whose blocks are the 5 x 5 corners of the
    6 x 6 blocks of M6: {lane: 6 x 6 array} (normal orientation, +2 on the diagonal; row 5 and column 5 never touched)."""
    lanes = [t for t in range(nb * (nb + 1) // 2 + 3) if sym6_lane(t, nb)[2]]
    X, gr, gc = {}, {}, {}
    for t in lanes:
        br, bc, _ = sym6_lane(t, nb)
        gr[t], gc[t] = bc, br                                   # mirror image: block (bc, br)
        X[t] = M6[6 * bc:6 * bc + 6, 6 * br:6 * br + 6].copy()
    bufs = [np.full(6 * nb, np.nan) for _ in range(3)]           # groups of six doubles, the sixth slot is padding
    last_buf = None

    def publish(ko, kb):
        nonlocal last_buf
        assert buf_of(ko) != last_buf                           # no two pivots in a row share a buffer
        last_buf = buf_of(ko)
        p, d = bufs[buf_of(ko)], None
        for t in lanes:
            if gr[t] == kb:
                w = X[t][ko, :5].copy()
                if gc[t] == kb:
                    d = w[ko]
                    w[ko] -= 1.0
                p[6 * gc[t]:6 * gc[t] + 5] = w
                p[6 * gc[t] + 5] = 0.0
        return p, d
    p, d = publish(0, 0)
    for kb in range(nb):
        for ko in range(5):
            assert not np.isnan(p).any()
            if ko == 4:                                          # the lanes of block-row kb + 1 turn their block over
                for t in lanes:
                    br, bc, _ = sym6_lane(t, nb)
                    if br == kb + 1 and gr[t] != br:
                        X[t][:5, :5] = X[t][:5, :5].T.copy()
                        gr[t], gc[t] = br, bc
            kon, kbn = (ko + 1) % 5, kb + (ko == 4)
            for t in lanes:
                pr, pc = p[6 * gr[t]:6 * gr[t] + 5], p[6 * gc[t]:6 * gc[t] + 5]
                X[t][:5, :5] += np.outer(-pr / d, pc)
            if kbn < nb:
                p, d = publish(kon, kbn)
    for t in lanes:
        br, bc, _ = sym6_lane(t, nb)
        assert (gr[t], gc[t]) == (br, bc)                       # every lane ends in the normal orientation
    return X


def back_transform(X, v, beta, c55):
    """sym5_back_transform: Q [ M 0 ; 0 c55 ] Q in place, as M6 - v w~' - u~ v'."""
    M6 = np.zeros((6, 6))
    M6[:5, :5] = X[:5, :5]
    M6[5, 5] = c55
    u, w = M6 @ v, M6.T @ v
    s = float(u @ v)
    ut, wt = beta * u, beta * w - beta * beta * s * v
    return M6 - np.outer(v, wt) - np.outer(ut, v)


GEOMETRIES = [   # (r1, r2, rpy): the trot diagonal, the pace pair, the bound pair, the axes with both signs, near-coincident feet
    ((0.33, -0.12, -0.42), (-0.29, 0.14, -0.40), (0.10, -0.15, 3.10)),
    ((0.33, 0.13, -0.42), (-0.30, 0.12, -0.43), (-0.20, 0.12, -3.12)),
    ((0.32, -0.13, -0.41), (0.31, 0.12, -0.42), (0.05, 0.20, 1.0)),
    ((0.30, 0.10, -0.40), (-0.30, 0.10, -0.40), (0.10, 0.10, 0.3)),
    ((-0.30, 0.10, -0.40), (0.30, 0.10, -0.40), (0.10, 0.10, 0.3)),
    ((0.10, 0.15, -0.40), (0.10, -0.15, -0.40), (0.15, -0.10, -2.0)),
    ((0.10, -0.15, -0.40), (0.10, 0.15, -0.40), (0.15, -0.10, -2.0)),
    ((0.10, 0.05, -0.30), (0.10, 0.05, -0.45), (0.20, 0.20, 0.7)),
    ((0.10, 0.05, -0.45), (0.10, 0.05, -0.30), (0.20, 0.20, 0.7)),
    ((0.2000, 0.1000, -0.4000), (0.2006, 0.0992, -0.4000), (0.10, -0.20, 2.5)),      # 1 mm apart
    ((0.2, 0.1, -0.4), (0.2 + 6e-7, 0.1 - 8e-7, -0.4), (0.10, -0.20, 2.5)),           # 1 um apart
    ((0.2, 0.1, -0.4), (0.2, 0.1, -0.4), (0.10, -0.20, 2.5)),                         # coincident: the fixed e
]


@pytest.mark.parametrize("geo", range(len(GEOMETRIES)))
def test_the_dropped_direction_is_a_null_vector_and_the_reflector_is_orthogonal(geo):
    r1, r2, rpy = (np.array(x, dtype=np.float64) for x in GEOMETRIES[geo])
    Bw, TBw, GU, GV = force_space_tables(r1, r2, rpy)
    v, beta, GU5, GV5, n = force_space_rank5(r1, r2, Bw, TBw)
    assert abs(v @ v - 2.0 * (1.0 + abs(n[5]))) <= 1e-15 and v @ v >= 2.0 - 1e-15      # no cancellation
    Q = np.eye(6) - beta * np.outer(v, v)
    np.testing.assert_allclose(Q @ Q.T, np.eye(6), rtol=0, atol=4e-16)
    np.testing.assert_allclose(Q[:, 5], -np.sign(v[5]) * n, rtol=0, atol=4e-16)
    for G in (GU, GV):
        assert np.abs(G @ n).max() <= 1e-14 * np.abs(G).max()
    for G, G5 in ((GU, GU5), (GV, GV5)):                                                 # the projected blocks are Q5' G Q5, padded
        np.testing.assert_allclose(G5[:5, :5], (Q.T @ G @ Q)[:5, :5], rtol=0, atol=1e-14 * np.abs(G).max())
        assert not G5[5].any() and not G5[:, 5].any()


@pytest.mark.parametrize("nb", [5, 10, 20])
@pytest.mark.parametrize("geo", [0, 4, 8, 10])
def test_five_wide_sweep_and_back_transform_reproduce_minus_inverse_of_P(nb, geo):
    r1, r2, rpy = (np.array(x, dtype=np.float64) for x in GEOMETRIES[geo])
    Bw, TBw, GU, GV = force_space_tables(r1, r2, rpy)
    v, beta, GU5, GV5, _ = force_space_rank5(r1, r2, Bw, TBw)
    N2, S2 = horizon_tables(nb)
    n = 6 * nb
    P = np.kron(N2, GU) + np.kron(S2, GV) + ALPHA * np.eye(n)
    M6 = np.kron(N2, GU5) + np.kron(S2, GV5) + ALPHA * np.eye(n)   # what sym6_build_kron6 builds from the padded blocks
    want = -np.linalg.inv(P)
    # The bound of the six-wide model is 1e-12 absolute on -inv(M) of M = A A' + n I, n = 60, whose largest entries are 1 / n:
    # 6e-11 of the inverse's largest entry.  The same bound here, on that scale: G = P^-1 has entries up to 1 / alpha.  (numpy's
    # own inverse is good to about cond(P) eps = 2.5e5 x 1.1e-16 = 3e-11 of that scale, so nothing tighter could be asked of
    # either side.)
    tol = 6e-11 * np.abs(want).max()
    X = sweep5_model(M6, nb)
    blocks, worst = {}, 0.0
    for t, blk in X.items():
        br, bc, _ = sym6_lane(t, nb)
        blocks[t] = back_transform(blk, v, beta, (2.0 - 1.0 / ALPHA) if br == bc else 0.0)
        ref = want[6 * br:6 * br + 6, 6 * bc:6 * bc + 6] + (2.0 * np.eye(6) if br == bc else 0.0)
        worst = max(worst, np.abs(blocks[t] - ref).max())
        assert np.abs(blocks[t] - ref).max() <= tol, (t, np.abs(blocks[t] - ref).max(), tol)
    print(f"nb {nb} geometry {geo}: worst |entry error| {worst:.2e} = {worst / np.abs(want).max():.1e} of the largest entry (bound 6e-11)")
    if nb != 10:
        return
    # ---- sym6_to_tile8: staging + gather (LG = 3: 8 x 8 lanes), unchanged by the rank-5 path ----
    stg = np.full(nb * (nb + 1) // 2 * 36, np.nan)
    for t, blk in blocks.items():
        br, bc, _ = sym6_lane(t, nb)
        b = blk - (2.0 * np.eye(6) if br == bc else 0.0)
        stg[(br * (br + 1) // 2 + bc) * 36:(br * (br + 1) // 2 + bc) * 36 + 36] = b.reshape(-1)
    for lane in range(64):
        lr, lc = lane >> 3, lane & 7
        perm = ((lc & 1) << 1) | (lc & 4)
        rsplit = 6 * (div6_u8(8 * lr) + 1)
        for ta in range(8):
            i = 8 * lr + (ta ^ perm)
            q = div6_u8(i); ia = i - 6 * q; ib = min(q, nb - 1)
            mir = lr < lc or (lr == lc and i < rsplit)
            rpart = ib * 36 + ia if mir else (ib * (ib + 1) // 2) * 36 + 6 * ia
            for tb in range(8):
                j = 8 * lc + tb
                q2 = div6_u8(j); ja = j - 6 * q2; jb = min(q2, nb - 1)
                val = stg[rpart + ((jb * (jb + 1) // 2) * 36 + 6 * ja if mir else jb * 36 + ja)]
                assert np.isfinite(val), (lane, ta, tb)
                if i < n and j < n:
                    assert abs(val - want[i, j]) <= tol, (lane, ta, tb, i, j)
