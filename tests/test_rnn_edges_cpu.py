"""The cases of tests/rnn_edges.py without a GPU: every one builds from the numpy models, stays within the caps of
tests/bptt_cases.py (every acting bound within TOL_CAP too), and is what it says it is -- a gate is exactly 1 or exactly 0 in
float32, a dead layer's output is exactly 0, a tensor's float64 gradient is all zeros, the flag values are all "set", a wide
key, counter or seed cast to 32 bits draws another number.  The existing cases of tests/bptt_cases.py keep their seeds.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

from tests import bptt_cases as BC
from tests import bptt_model as BM
from tests import policy_model as PM
from tests import rnn_edges as E
from tests import rnn_model as RM


def _capped(tol, what):
    print(f"{what}: bounds {tol}")
    assert all(E.FLOOR <= v <= E.TOL_CAP for v in tol.values()), (what, tol)


# ---- the tables -------------------------------------------------------------------------------------------------------------

def test_edge_configurations_are_what_they_are_for():
    lays = {name: BC.net(name)[1] for name in BC.EDGE_CONFIGS}
    assert all(cfg["value_layers"] == (65,) for cfg in BC.EDGE_CONFIGS.values())
    assert [2 * lays[k]["gru_units"] for k in ("wave63", "wave64", "wave65")] == [126, 128, 130] and lays["unit1"]["gru_units"] == 1
    rows = {name: [i for i, _, _, _ in RM.blocks(lay)] for name, lay in lays.items()}
    assert rows["rows15"] == [15, 47, 47, 16] and rows["wave64"][0] == 15 and rows["wave64"][1] == 128
    assert any(i % BC.bptt_abi.ROWS == 15 for i in rows["rows15"]) and any(i % BC.bptt_abi.ROWS == 0 for i in rows["rows15"])   # the bias closes a tile; has its own
    assert len(lays["wave65"]["dense"]) == 2 and BC.EDGE_CONFIGS["wave65"]["obs_dim"] == 1
    assert len({s for pair in BC.EDGE_SEEDS.values() for s in pair}) == 2 * len(BC.EDGE_CONFIGS)


def test_the_existing_cases_keep_their_seeds():
    """net() and case() seed a configuration of CONFIGS from its place in sorted(CONFIGS): the table has its four keys, and the
    first draw of every net is what that seed gives."""
    assert sorted(BC.CONFIGS) == ["default", "limits", "lopsided", "two dense"]
    for k, name in enumerate(sorted(BC.CONFIGS)):
        cfg, lay, pp = BC.net(name)[:3]
        i, o, w, _ = RM.blocks(lay)[0]
        limit = np.sqrt(6.0 / (i + o))
        want = np.random.default_rng(1900 + k).uniform(-limit, limit, i * o).astype(np.float32)
        assert pp[w:w + i * o].tobytes() == want.tobytes(), name


def test_flag_values_are_all_set_and_none_is_one():
    assert set(E.FLAGS) == {256, 65536, -2 ** 31, -1, 2 ** 31 - 1}
    f = np.array(E.FLAGS, dtype=np.int64).astype(np.int32)
    assert np.all(f != 0) and np.all(f != 1)
    assert (f.astype(np.uint8) == 0).sum() == 3 and (f < 0).sum() == 2         # what a byte test and a sign test would drop
    for flag in E.FLAGS:
        r = E.resets(4, 13, flag)
        assert np.array_equal(r != 0, E.resets(4, 13) != 0) and set(np.unique(r)) == {0, np.int32(flag)}
        assert np.array_equal(E.flagged(E.resets(4, 13), flag), r)


# ---- A. shapes -----------------------------------------------------------------------------------------------------------------

def test_shapes_cover_the_tile():
    assert E.TILE == 8 and E.GUARD_BATCHES == (1, 7, 9, 257) and E.CHAIN_BATCHES == (1, 7, 8) and E.CHAIN_T == (1, 2, 33) and E.KNOWN_B == 13
    assert E.STREAM_BATCHES == (9, 257) and (E.LONG_T, E.LONG_B) == (257, 9)
    for name in E.ACT_CONFIGS:
        n = E.act_net(name)
        assert n["lay"] == RM.layout(**{k: n["cfg"][k] for k in ("obs_dim", "act_dim", "policy_layers", "gru_units", "value_layers")})
    assert E.act_net("h65")["lay"]["gru_units"] == 65 and E.act_net("h65")["lay"]["dense"][0][1] == 65


@pytest.mark.parametrize("name", E.LONG_CONFIGS)
def test_long_sequence(name):
    c = E.long_case(name)
    rule = c["rule"]
    print(f"{name} T={E.LONG_T} B={E.LONG_B}: float32-numpy vs float64 {rule['dev']}")
    _capped(rule["tol"], f"long {name}")
    assert c["reset"][0].any() and c["reset"][128].any() and c["reset"][256].any() and (c["reset"] == 0).all(axis=0).any()
    assert np.all(np.isfinite(rule["mean"])) and np.abs(rule["hidden_seq"][-1]).max() > 0.05
    u = RM.tick(RM.normalised(c["obs"][0], c["n"]["state"]), c["h0"], c["reset"][0], c["n"]["pp"], c["n"]["lay"])["u"]
    assert u.min() < 0.3 and u.max() > 0.7                                      # gates neither all shut nor all open


# ---- B. known answers --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_update_gate_open_holds_the_state_to_the_bit(name):
    c = E.known_case(name, "hold")
    m64, m32 = c["act"]["m64"], c["act"]["m32"]
    assert np.all(m32["u"] == np.float32(1.0)) and m32["u"].dtype == np.float32 and np.all(m64["u"] == 1.0)
    want = np.where(c["reset"][0][:, None] != 0, np.float32(0), c["hidden"])
    assert m32["hidden"].tobytes() == want.tobytes() and np.array_equal(m64["hidden"], want.astype(np.float64))
    assert c["unroll"]["hidden32"].tobytes() == E.carried(c["hidden"], c["reset"]).tobytes()
    assert np.abs(E.carried(c["hidden"], c["reset"])[-1]).max() > 0 and not np.array_equal(E.carried(c["hidden"], c["reset"])[-1], c["hidden"])
    _capped(c["act"]["tol"], f"hold act {name}"), _capped(c["unroll"]["tol"], f"hold unroll {name}")


@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_both_gates_shut_forget_the_state(name):
    c = E.known_case(name, "shut")
    n, lay = c["n"], c["n"]["lay"]
    m32 = c["act"]["m32"]
    assert np.all(m32["r"] == 0.0) and np.all(m32["u"] == 0.0) and np.all(c["act"]["m64"]["u"] < 1e-40)
    x = RM.normalised(c["obs"][0], n["state"])
    a = RM.tick(x, c["hidden"], None, c["pp"], lay, np.float32)
    b = RM.tick(x, c["other_hidden"], None, c["pp"], lay, np.float32)
    z = RM.tick(x, c["hidden"], np.ones(E.KNOWN_B, dtype=np.int32), c["pp"], lay, np.float32)
    assert not np.array_equal(c["hidden"], c["other_hidden"])
    assert a["hidden"].tobytes() == b["hidden"].tobytes() == z["hidden"].tobytes() == a["c"].tobytes() and a["mean"].tobytes() == b["mean"].tobytes()
    assert np.all((a["r"] == 0) & (b["r"] == 0) & (a["u"] == 0) & (b["u"] == 0))
    perm = np.array([2, 0, 3, 1])
    m, h = c["unroll"]["mean32"], c["unroll"]["hidden32"]
    mp, hp = RM.unroll(c["obs"][perm], c["reset"], c["hidden"], n["state"], c["pp"], lay, dtype=np.float32)
    assert mp.tobytes() == m[perm].tobytes() and hp.tobytes() == h[perm].tobytes() and len({t.tobytes() for t in h}) == E.KNOWN_T
    _capped(c["act"]["tol"], f"shut act {name}")


@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_a_dead_first_layer_hides_the_observation(name):
    c = E.known_case(name, "dead")
    n, lay = c["n"], c["n"]["lay"]
    for dtype in (np.float32, np.float64):
        for obs in (c["obs"][0], c["other_obs"][0]):
            assert np.all(RM.tick(RM.normalised(obs, n["state"]), c["hidden"], c["reset"][0], c["pp"], lay, dtype)["x"] == 0.0)
    i, o, w, b = lay["dense"][0]
    assert np.all(c["pp"][w:w + i * o] == 0) and np.all(c["pp"][b:b + o] < 0) and np.all(np.isfinite(c["obs"])) and np.all(np.isfinite(c["other_obs"]))
    live = E.known_case(name, "plain")
    a = RM.tick(RM.normalised(c["obs"][0], n["state"]), c["hidden"], c["reset"][0], live["pp"], lay, np.float32)
    b_ = RM.tick(RM.normalised(c["other_obs"][0], n["state"]), c["hidden"], c["reset"][0], live["pp"], lay, np.float32)
    assert np.all(np.abs(a["mean"] - b_["mean"]).max(axis=1) > 0)              # with live weights every robot's mean differs
    _capped(c["act"]["tol"], f"dead act {name}")


@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_non_finite_inputs_in_the_model(name):
    c = E.nonfinite_case(name)
    m, clean = c["rule"]["m64"], c["clean"]["m64"]
    others = np.setdiff1d(np.arange(E.KNOWN_B), E.SPOILT)
    assert E.NAN_OBS_ROBOT < E.TILE and E.INF_OBS_ROBOT < E.TILE <= E.NAN_HIDDEN_ROBOT
    assert np.isnan(c["obs"][:, E.NAN_OBS_ROBOT]).sum() == 1 and np.isinf(c["obs"][:, E.INF_OBS_ROBOT]).sum() == 1 and np.isnan(c["hidden"][E.NAN_HIDDEN_ROBOT]).all()
    for k in ("mean", "value", "hidden"):
        assert np.array_equal(m[k][others], clean[k][others]), k
        assert np.all(np.isfinite(m[k][E.INF_OBS_ROBOT])), k                    # the normaliser clips +inf to obs_clip
        assert np.all(np.isfinite(m[k][E.NAN_OBS_ROBOT])), k                    # relu sends the NaN pre-activations to 0 (module docstring of rnn_edges)
    assert m["x"][E.INF_OBS_ROBOT, 0] == 5.0 and np.isnan(m["x"][E.NAN_OBS_ROBOT]).sum() == 1
    assert np.all(np.isnan(m["mean"][E.NAN_HIDDEN_ROBOT])) and np.all(np.isnan(m["hidden"][E.NAN_HIDDEN_ROBOT])) and np.isfinite(m["value"][E.NAN_HIDDEN_ROBOT])
    assert not np.array_equal(m["mean"][E.NAN_OBS_ROBOT], clean["mean"][E.NAN_OBS_ROBOT])
    print(f"{name}: float32-numpy vs float64 {c['rule']['dev']}")
    _capped(c["rule"]["tol"], f"non-finite {name}")


@pytest.mark.parametrize("clip", E.CLIPS)
@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_obs_clip_cases(name, clip):
    c = E.clip_case(name, clip)
    x = c["rule"]["m64"]["x"]
    print(f"{name} clip {clip}: largest |x| {np.abs(x).max():.2f}; float32-numpy vs float64 {c['rule']['dev']}")
    if clip == 0.0:
        assert np.abs(x).max() > 20.0 and (np.abs(x) > 5.0).mean() > 0.2        # far beyond the default clip, and not clipped
    else:
        assert np.abs(x).max() == 0.5 and (np.abs(x) == 0.5).mean() > 0.3
    _capped(c["rule"]["tol"], f"clip {clip} {name}")


@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_wide_keys_counters_and_seed_draw_what_their_low_words_do_not(name):
    c = E.wide_case(name)
    A = c["n"]["cfg"]["act_dim"]
    keys, counters = c["keys"], c["counters"]
    assert (keys < 0).any() and (keys >= 2 ** 40).any() and {2 ** 32 - 1, 2 ** 32, 2 ** 63 - 2} <= set(counters.tolist()) and E.WIDE_SEED >= 2 ** 63
    e = c["rule"]["m64"]["eps"]
    low = lambda v: np.asarray(v, dtype=np.int64) & 0xFFFFFFFF
    wide_k, wide_c = keys != low(keys), counters != low(counters)
    assert np.all((e != PM.eps_batch(E.WIDE_SEED, low(keys), counters, A)).any(axis=1)[wide_k])
    assert np.all((e != PM.eps_batch(E.WIDE_SEED, keys, low(counters), A)).any(axis=1)[wide_c])
    assert np.all((e != PM.eps_batch(E.WIDE_SEED & 0xFFFFFFFF, keys, counters, A)).any(axis=1))
    assert np.all((e != PM.eps_batch(E.WIDE_SEED, keys, counters + 1, A)).any(axis=1))
    _capped(c["rule"]["tol"], f"wide {name}")


# ---- C. the update ------------------------------------------------------------------------------------------------------------

def _caps(c, skip=()):
    tol = {k: v for k, v in c["p_tol"].items() if k not in skip}
    print(f"{c['name']} T={c['T']} B={c['B']}: redrawn {c['redrawn']:.3f}; one ulp of the means costs {c['ulp_cost']:.3e}; float32-numpy vs float64 {c['p_dev32']} "
          f"loss {c['p_loss_dev32']:.3e}; bounds {tol} loss {c['p_loss_tol']:.3e}")
    assert c["redrawn"] <= E.REDRAW_CAP and c["ulp_cost"] <= E.ULP_CAP
    assert max(tol.values()) <= E.TOL_CAP and c["p_loss_tol"] <= E.TOL_CAP
    T, B = c["T"], c["B"]
    assert (c["reset"][0] != 0).any() and ((c["reset"][T - 1] != 0).any() or B < 3) and np.abs(c["h0"]).max() > 0
    if B >= 5:
        assert c["p64"]["over"].any() and not c["p64"]["over"].all() and c["p64"]["kl"][B - 1] == 0.0


@pytest.mark.parametrize("name,T,B", E.EDGE_CASES + E.FULL_CASES)
def test_every_gradient_case_builds_within_its_caps(name, T, B):
    c = BC.case(name, T, B)
    _caps(c)
    assert all(np.abs(c["p64"]["grad"][s]).max() > 0 for s in BM.tensors(c["lay"]).values())


@pytest.mark.parametrize("name,T,B", E.LAST_LIVE_CASES)
def test_cases_with_the_last_robot_valid_build_within_their_caps(name, T, B):
    """Mask "last": the last robot carries gradient (its removal moves tensors far beyond their bounds); the masked robot is the first."""
    c = BC.case(name, T, B, mask_kind="last")
    base = BC.case(name, T, B)
    assert np.all(base["mask"][:, B - 1] == 0) and np.all(c["mask"][:, B - 1] != 0) and np.all(c["mask"][:, 0] == 0) and c["p64"]["kl"][0] == 0.0
    assert c["obs"].tobytes() == base["obs"].tobytes()
    tol = c["p_tol"]
    print(f"last robot valid, {name} T={T} B={B}: redrawn {c['redrawn']:.3f}; one ulp of the means costs {c['ulp_cost']:.3e}; bounds {tol} loss {c['p_loss_tol']:.3e}")
    assert c["redrawn"] <= E.REDRAW_CAP and c["ulp_cost"] <= E.ULP_CAP and max(tol.values()) <= E.TOL_CAP and c["p_loss_tol"] <= E.TOL_CAP
    without = c["mask"].copy()
    without[:, B - 1] = 0
    g = BM.policy_grad(c["x"], c["reset"], c["h0"], c["pp"], c["lay"], c["action"], c["mean"], c["logstd"], c["adv"], without, stats=c["stats"], **c["model_kw"])["grad"]
    moved = BC.deviation(g, c["p64"]["grad"], BM.tensors(c["lay"]))
    print(f"without the last robot: {moved}")
    assert all(moved[k] > 10 * tol[k] for k in moved if k.startswith("W_") or k.startswith("b_"))
    assert any(B % E.TILE == 0 for _, _, B in E.LAST_LIVE_CASES) and any(B % E.TILE == 1 for _, _, B in E.LAST_LIVE_CASES)


def test_full_shapes_are_full():
    assert [(B % E.TILE, T * B % E.CHUNK) for T, B in E.FULL_SHAPES] == [(0, 0), (0, 0), (1, 0), (0, 0), (0, 8)]
    assert (2, 8) in E.FULL_SHAPES and (1, 16) in E.FULL_SHAPES and BC.bptt_abi.groups(4, 16) == 4 and BC.bptt_abi.groups(1, 16) == 1


@pytest.mark.parametrize("name,T,B", E.SATURATED_CASES)
def test_an_open_update_gate_passes_no_gradient_below_the_head(name, T, B):
    c = BC.case(name, T, B, gates="hold")
    _caps(c)
    names = BM.tensors(c["lay"])
    f = BM.forward(c["x"], c["reset"], c["h0"], c["pp"], c["lay"])
    assert np.all(f["u"] == 1.0) and np.all(BM.forward(c["x"], c["reset"], c["h0"], c["pp"], c["lay"], np.float32)["u"] == np.float32(1.0))
    for k in E.gate_tensors(c["lay"]):
        assert np.all(c["p64"]["grad"][names[k]] == 0.0) and np.all(c["p32"]["grad"][names[k]] == 0.0), k
        assert c["p_tol"][k] == BC.PROJECT_FLOOR                                 # and deviation() then measures max|g|
    assert set(names) - set(E.gate_tensors(c["lay"])) == {"W_head", "b_head", "logstd"}
    for k in ("W_head", "b_head", "logstd"):
        assert np.abs(c["p64"]["grad"][names[k]]).max() > 0, k


@pytest.mark.parametrize("name,T,B", E.SATURATED_CASES)
def test_shut_gates_leave_the_gates_weights_and_the_h_rows_without_gradient(name, T, B):
    c = BC.case(name, T, B, gates="shut")
    _caps(c, skip=E.SHUT_ZERO)
    lay, names, g64, g32 = c["lay"], BM.tensors(c["lay"]), c["p64"]["grad"], c["p32"]["grad"]
    f32 = BM.forward(c["x"], c["reset"], c["h0"], c["pp"], lay, np.float32)
    assert np.all(f32["r"] == 0.0) and np.all(f32["u"] == 0.0)
    top = float(np.abs(g64[names["W_head"]]).max())
    i, o, w, _ = lay["w_c"]
    h_rows_c = slice(w + lay["n_x"] * o, w + i * o)
    small = {k: float(np.abs(g64[s]).max()) for k, s in (("W_ru", names["W_ru"]), ("b_ru", names["b_ru"]), ("h rows of W_c", h_rows_c))}
    print(f"{name} shut: largest float64 entries {small}, the head's {top:.3e}")
    assert top > 0 and all(v < 1e-30 * top for v in small.values())
    for s in (names["W_ru"], names["b_ru"], h_rows_c):
        assert np.all(g32[s] == 0.0)
    x_rows_c = slice(w, w + lay["n_x"] * o)
    assert np.abs(g64[x_rows_c]).max() > 0 and all(np.abs(g64[names[k]]).max() > 0 for k in names if k.endswith("dense0") or k.endswith("dense1"))
    assert set(E.SHUT_ZERO) <= set(names)


def test_flag_case_holds_ones_to_replace():
    c = BC.case(*E.FLAG_CASE)
    assert (c["mask"] == 1).sum() > 10 and (c["reset"] == 1).sum() > 10
    for flag in (256, 65536, E.INT_MIN):
        m, r = E.flagged(c["mask"], flag), E.flagged(c["reset"], flag)
        assert np.array_equal(m != 0, c["mask"] != 0) and np.array_equal(r != 0, c["reset"] != 0) and (m == np.int32(flag)).sum() == (c["mask"] == 1).sum()
        assert not (m == 1).any() and not (r == 1).any()


def test_workspace_cases_are_cases():
    for name, T, B in E.WORKSPACE_CASES:
        assert (name, T, B) in E.EDGE_CASES + E.FULL_CASES
