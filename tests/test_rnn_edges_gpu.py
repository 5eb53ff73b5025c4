"""The recurrent policy's kernels (include/rg_rnn.h) and its update (include/rg_bptt.h) at their edges, on the cases of
tests/rnn_edges.py (the models alone run over them in tests/test_rnn_edges_cpu.py): guard bands around every output of act and
unroll and around the update's workspace, inputs left as they were, optional outputs, the unroll against a chain of acts at
batches around a tile and through 33 and 257 ticks, two calls and a side stream; saturated gates, a dead layer, flag values,
non-finite inputs, obs_clip 0 and 0.5 and a wide noise stream with their known answers; the gradient at wave-edge and
row-tile-edge configurations, whole tiles and whole chunks, saturated gates and the same flag values.

Every bound is tests/rnn_edges.py's or tests/bptt_cases.py's, formed from the models alone and printed before it is asserted;
the gradient checks are those of tests/test_bptt_gpu.py, imported."""
import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import DeviceRecurrentPPO, RecurrentGaussianPolicy
from robot_gym_amd.core import rnn_abi
from tests import bptt_cases as BC
from tests import bptt_model as BM
from tests import policy_model as PM
from tests import rnn_edges as E
from tests import test_bptt_gpu as TB

pytestmark = pytest.mark.gpu

TILE = rnn_abi.TILE
GUARD = 64
F_SENTINEL, I_SENTINEL = -12345.5, -77777
OUTS = ("action", "mean", "value", "logprob")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _t(a, dev):
    """A tensor holding a copy of a (the shared inputs are read-only arrays)."""
    return torch.as_tensor(np.array(a), device=dev)


def _policy(dev, n, B, pp=None, clip=5.0, seed=E.SEED):
    pol = RecurrentGaussianPolicy(B, seed=seed, device=dev, obs_clip=clip, **n["cfg"])
    assert pol.layout == n["lay"]
    with torch.no_grad():
        pol.policy_params.copy_(_t(n["pp"] if pp is None else pp, dev))
        pol.value_params.copy_(_t(n["vp"], dev))
    pol.norm_state.copy_(_t(n["state"], dev))
    return pol


def _outs(pol, names=OUTS, fill=7.0):
    B, A = pol.batch, pol.act_dim
    shapes = dict(action=(B, A), mean=(B, A), value=(B,), logprob=(B,))
    return {k: torch.full(shapes[k], fill, dtype=torch.float32, device=pol.device) for k in names}


def _state(c_or_r, dev):
    return _t(np.stack((c_or_r["keys"], c_or_r["counters"])), dev)


def _act(pol, obs, h_in, h_out, reset, state, sample, out):
    """rg_rnn_act through the handle; reset, state and every output but action may be None (a NULL pointer)."""
    ptr = lambda t: None if t is None else t.data_ptr()
    pol._rnn.act(obs.data_ptr(), pol.norm_state.data_ptr(), pol.policy_params.data_ptr(), pol.value_params.data_ptr(), ptr(state), ptr(reset), h_in.data_ptr(),
                 h_out.data_ptr(), rnn_abi.MODE_SAMPLE if sample else rnn_abi.MODE_MEAN, out["action"].data_ptr(), ptr(out.get("mean")), ptr(out.get("value")),
                 ptr(out.get("logprob")))
    return out


def _unroll(pol, obs, reset, h0, mean, hseq=None, hlast=None):
    ptr = lambda t: None if t is None else t.data_ptr()
    pol._rnn.unroll(obs.data_ptr(), reset.data_ptr(), h0.data_ptr(), pol.norm_state.data_ptr(), pol.policy_params.data_ptr(), obs.shape[0], mean.data_ptr(),
                    ptr(hseq), ptr(hlast))


def _run_act(pol, obs, h_in, reset, state, sample=False):
    """One out-of-place act with every output: dict of numpy arrays, hidden among them."""
    h_out = torch.full_like(h_in, 7.0)
    out = _act(pol, obs, h_in, h_out, reset, state, sample, _outs(pol))
    return dict({k: v.cpu().numpy() for k, v in out.items()}, hidden=h_out.cpu().numpy())


def _run_unroll(pol, obs, reset, h0):
    T, B, A, H = obs.shape[0], pol.batch, pol.act_dim, pol.gru_units
    f = dict(dtype=torch.float32, device=pol.device)
    mean, hseq, hlast = torch.full((T, B, A), 7.0, **f), torch.full((T, B, H), 7.0, **f), torch.full((B, H), 7.0, **f)
    _unroll(pol, obs, reset, h0, mean, hseq, hlast)
    return dict(mean=mean.cpu().numpy(), hidden_seq=hseq.cpu().numpy(), hidden_last=hlast.cpu().numpy())


def _chain(pol, obs, reset, h0):
    """T acts in MEAN mode with a NULL act_state, the state advanced in place: (means [T, B, A], states [T, B, H])."""
    h, out = h0.clone(), _outs(pol)
    means, states = [], []
    for t in range(obs.shape[0]):
        _act(pol, obs[t], h, h, reset[t], None, False, out)
        means.append(out["mean"].clone()), states.append(h.clone())
    return torch.stack(means), torch.stack(states)


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), F_SENTINEL if dtype.is_floating_point else I_SENTINEL, dtype=dtype, device=dev)
    return big, big[GUARD:GUARD + n].view(*shape)


def _bands_intact(big, written=True):
    sentinel = F_SENTINEL if big.dtype.is_floating_point else I_SENTINEL
    a = big.cpu().numpy()
    assert np.all(a[:GUARD] == sentinel) and np.all(a[-GUARD:] == sentinel)
    if written:
        assert not np.any(a[GUARD:-GUARD] == sentinel)           # and the slice itself was filled


def _bytes(tensors):
    return {k: v.detach().cpu().numpy().tobytes() for k, v in tensors.items()}


def _within(got, want, tol, what):
    """|got - want| <= tol where the model is finite, NaN exactly where it is not."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"{what}: kernel vs float64 model {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


# ---- A1. nothing past the ends, no input touched --------------------------------------------------------------------------------

@pytest.mark.parametrize("B", E.GUARD_BATCHES)
@pytest.mark.parametrize("name", E.GUARD_CONFIGS)
def test_act_stays_inside_its_outputs_and_leaves_its_inputs(dev, name, B):
    n = E.act_net(name)
    r = E.draw(name, 1, B, 9100 + B)
    pol = _policy(dev, n, B)
    A, H, f32 = pol.act_dim, pol.gru_units, torch.float32
    obs, h_in, reset = _t(r["obs"][0], dev), _t(r["hidden"], dev), _t(E.resets(1, B)[0], dev)
    bigs, out = {}, {}
    for k, shape in (("action", (B, A)), ("mean", (B, A)), ("value", (B,)), ("logprob", (B,))):
        bigs[k], out[k] = _guarded(shape, f32, dev)
    bigs["hidden_out"], h_out = _guarded((B, H), f32, dev)
    big_s, state = _guarded((2, B), torch.int64, dev)
    state.copy_(_state(r, dev))
    inputs = dict(obs=obs, norm_state=pol.norm_state, policy_params=pol.policy_params, value_params=pol.value_params, reset=reset, hidden_in=h_in)
    before = _bytes(inputs)
    draws = 0
    for sample in (True, False, True):
        for big in bigs.values():
            big.fill_(F_SENTINEL)
        _act(pol, obs, h_in, h_out, reset, state, sample, out)
        torch.cuda.synchronize(dev)
        draws += int(sample)
        for big in bigs.values():
            _bands_intact(big)
        _bands_intact(big_s, written=False)
        got = state.cpu().numpy()
        assert np.array_equal(got[0], r["keys"]) and np.array_equal(got[1], r["counters"] + draws)
        assert _bytes(inputs) == before
    pol.close()


@pytest.mark.parametrize("T", E.GUARD_T)
@pytest.mark.parametrize("B", E.GUARD_BATCHES)
@pytest.mark.parametrize("name", E.GUARD_CONFIGS)
def test_unroll_stays_inside_its_outputs_and_leaves_its_inputs(dev, name, B, T):
    n = E.act_net(name)
    r = E.draw(name, T, B, 9200 + B)
    pol = _policy(dev, n, B)
    A, H, f32 = pol.act_dim, pol.gru_units, torch.float32
    obs, h0, reset = _t(r["obs"], dev), _t(r["hidden"], dev), _t(E.resets(T, B), dev)
    big_m, mean = _guarded((T, B, A), f32, dev)
    big_q, hseq = _guarded((T, B, H), f32, dev)
    big_l, hlast = _guarded((B, H), f32, dev)
    inputs = dict(obs=obs, norm_state=pol.norm_state, policy_params=pol.policy_params, reset=reset, h0=h0)
    before = _bytes(inputs)
    _unroll(pol, obs, reset, h0, mean, hseq, hlast)
    torch.cuda.synchronize(dev)
    for big in (big_m, big_q, big_l):
        _bands_intact(big)
    assert _bytes(inputs) == before
    assert torch.equal(hlast, hseq[T - 1])
    pol.close()


# ---- A2. optional outputs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.GUARD_CONFIGS)
def test_optional_outputs_change_no_other_output(dev, name):
    B, T = TILE + 1, 3
    n = E.act_net(name)
    r = E.draw(name, T, B, 9300)
    pol = _policy(dev, n, B)
    obs, h_in, reset_seq = _t(r["obs"], dev), _t(r["hidden"], dev), _t(E.resets(T, B), dev)
    reset = reset_seq[0]

    def run(names, sample, with_state=True):
        state = _state(r, dev) if with_state else None
        h_out = torch.full_like(h_in, 7.0)
        out = _act(pol, obs[0], h_in, h_out, reset, state, sample, _outs(pol, names))
        res = dict(_bytes(out), hidden=h_out.cpu().numpy().tobytes())
        if with_state:
            res["state"] = state.cpu().numpy().tobytes()
        return res

    full = run(OUTS, True)
    for names in (("action", "value", "logprob"), ("action", "mean", "logprob"), ("action", "mean", "value"), ("action",)):
        got = run(names, True)
        assert set(got) == set(names) | {"hidden", "state"}
        for k, v in got.items():
            assert v == full[k], (names, k)
    det = run(OUTS, False)
    assert det["state"] == _state(r, dev).cpu().numpy().tobytes() and det["action"] == det["mean"] == full["mean"] and det["hidden"] == full["hidden"]
    for names in (OUTS, ("action",)):
        got = run(names, False, with_state=False)                # MEAN mode reads no act_state: a NULL pointer
        for k, v in got.items():
            assert v == det[k], (names, k)
    # unroll: hidden_seq NULL, hidden_last NULL, both
    want = _run_unroll(pol, obs, reset_seq, h_in)
    A, H, f = pol.act_dim, pol.gru_units, dict(dtype=torch.float32, device=dev)
    for with_seq, with_last in ((False, True), (True, False), (False, False)):
        mean = torch.full((T, B, A), 7.0, **f)
        hseq = torch.full((T, B, H), 7.0, **f) if with_seq else None
        hlast = torch.full((B, H), 7.0, **f) if with_last else None
        _unroll(pol, obs, reset_seq, h_in, mean, hseq, hlast)
        assert mean.cpu().numpy().tobytes() == want["mean"].tobytes()
        assert hseq is None or hseq.cpu().numpy().tobytes() == want["hidden_seq"].tobytes()
        assert hlast is None or hlast.cpu().numpy().tobytes() == want["hidden_last"].tobytes()
    assert want["hidden_last"].tobytes() == want["hidden_seq"][T - 1].tobytes() != want["hidden_seq"][0].tobytes()
    pol.close()


# ---- A3, A4. the unroll is a chain of acts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", E.CHAIN_BATCHES)
@pytest.mark.parametrize("name", E.GUARD_CONFIGS)
def test_unroll_equals_a_chain_of_acts_at_batches_around_a_tile(dev, name, B):
    n = E.act_net(name)
    pol = _policy(dev, n, B)
    A, H, f = pol.act_dim, pol.gru_units, dict(dtype=torch.float32, device=dev)
    for T in E.CHAIN_T:
        r = E.draw(name, T, B, 9400 + T)
        obs, h0, reset = _t(r["obs"], dev), _t(r["hidden"], dev), _t(E.resets(T, B), dev)
        assert int((reset != 0).sum()) > 0
        means, states = _chain(pol, obs, reset, h0)
        got = _run_unroll(pol, obs, reset, h0)
        assert got["mean"].tobytes() == means.cpu().numpy().tobytes(), T
        assert got["hidden_seq"].tobytes() == states.cpu().numpy().tobytes(), T
        assert got["hidden_last"].tobytes() == states[-1].cpu().numpy().tobytes(), T
        if T > 1:
            assert not torch.equal(states[-1], states[0])                      # the last state is not the first
        if T == max(E.CHAIN_T):                                                 # hidden_last alone
            mean, hlast = torch.full((T, B, A), 7.0, **f), torch.full((B, H), 7.0, **f)
            _unroll(pol, obs, reset, h0, mean, None, hlast)
            assert torch.equal(mean, means) and torch.equal(hlast, states[-1])
    pol.close()


@pytest.mark.parametrize("name", E.LONG_CONFIGS)
def test_a_long_sequence_is_the_chain_to_the_bit_and_the_model_within_the_rule(dev, name):
    c = E.long_case(name)
    n, rule = c["n"], c["rule"]
    pol = _policy(dev, n, E.LONG_B)
    obs, h0, reset = _t(c["obs"], dev), _t(c["h0"], dev), _t(c["reset"], dev)
    means, states = _chain(pol, obs, reset, h0)
    got = _run_unroll(pol, obs, reset, h0)
    assert got["mean"].tobytes() == means.cpu().numpy().tobytes() and got["hidden_seq"].tobytes() == states.cpu().numpy().tobytes()
    assert got["hidden_last"].tobytes() == states[-1].cpu().numpy().tobytes()
    print(f"{name} T={E.LONG_T} B={E.LONG_B}: float32-numpy vs float64 model {rule['dev']}")
    _within(got["mean"], rule["mean"], rule["tol"]["mean"], f"long {name} mean")
    _within(got["hidden_seq"], rule["hidden_seq"], rule["tol"]["hidden"], f"long {name} hidden")
    pol.close()


# ---- A5. two calls and a side stream ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", E.STREAM_BATCHES)
@pytest.mark.parametrize("name", E.GUARD_CONFIGS)
def test_two_calls_and_a_side_stream_give_the_same_bytes(dev, name, B):
    T = 3
    n = E.act_net(name)
    r = E.draw(name, T, B, 9500 + B)
    pol = _policy(dev, n, B)
    obs, h_in, reset = _t(r["obs"], dev), _t(r["hidden"], dev), _t(E.resets(T, B), dev)
    torch.cuda.synchronize(dev)

    def run():
        state = _state(r, dev)                                               # the counters put back
        a = _run_act(pol, obs[0], h_in, reset[0], state, sample=True)
        u = _run_unroll(pol, obs, reset, h_in)
        return {k: v.tobytes() for k, v in dict(a, state=state.cpu().numpy(), **{"unroll " + k: v for k, v in u.items()}).items()}

    first = run()
    assert run() == first
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert third == first
    pol.close()


# ---- B1 .. B3. saturated gates and a dead layer -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_an_open_update_gate_holds_the_state_to_the_bit(dev, name):
    c = E.known_case(name, "hold")
    pol = _policy(dev, c["n"], E.KNOWN_B, pp=c["pp"])
    obs, hidden, reset = _t(c["obs"], dev), _t(c["hidden"], dev), _t(c["reset"], dev)
    got = _run_act(pol, obs[0], hidden, reset[0], None)
    want = np.where(c["reset"][0][:, None] != 0, np.float32(0), c["hidden"])
    assert got["hidden"].tobytes() == want.tobytes()
    print(f"hold {name}: float32-numpy vs float64 model {c['act']['dev']}")
    _within(got["mean"], c["act"]["m64"]["mean"], c["act"]["tol"]["mean"], f"hold {name} mean")
    seq = _run_unroll(pol, obs, reset, hidden)
    carried = E.carried(c["hidden"], c["reset"])
    assert seq["hidden_seq"].tobytes() == carried.tobytes() and seq["hidden_last"].tobytes() == carried[-1].tobytes()
    _within(seq["mean"], c["unroll"]["mean"], c["unroll"]["tol"]["mean"], f"hold {name} unroll mean")
    pol.close()


@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_shut_gates_forget_the_state(dev, name):
    c = E.known_case(name, "shut")
    pol = _policy(dev, c["n"], E.KNOWN_B, pp=c["pp"])
    obs, hidden, other, reset = _t(c["obs"], dev), _t(c["hidden"], dev), _t(c["other_hidden"], dev), _t(c["reset"], dev)
    a = _run_act(pol, obs[0], hidden, reset[0], None)
    b = _run_act(pol, obs[0], other, reset[0], None)
    z = _run_act(pol, obs[0], hidden, torch.ones_like(reset[0]), None)
    for k in ("hidden", "mean", "action"):
        assert a[k].tobytes() == b[k].tobytes() == z[k].tobytes(), k
    _within(a["mean"], c["act"]["m64"]["mean"], c["act"]["tol"]["mean"], f"shut {name} mean")
    _within(a["hidden"], c["act"]["m64"]["hidden"], c["act"]["tol"]["hidden"], f"shut {name} hidden")
    perm = [2, 0, 3, 1]
    seq = _run_unroll(pol, obs, reset, hidden)
    moved = _run_unroll(pol, obs[perm].contiguous(), reset, hidden)
    assert moved["mean"].tobytes() == seq["mean"][perm].tobytes() and moved["hidden_seq"].tobytes() == seq["hidden_seq"][perm].tobytes()
    assert moved["hidden_last"].tobytes() == seq["hidden_seq"][perm[-1]].tobytes() != seq["hidden_last"].tobytes()
    pol.close()


@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_a_dead_first_layer_hides_the_observation(dev, name):
    """The value network reads the observation itself and is left out of the comparison."""
    c = E.known_case(name, "dead")
    obs, other, hidden, reset = _t(c["obs"], dev), _t(c["other_obs"], dev), _t(c["hidden"], dev), _t(c["reset"], dev)
    results = {}
    for kind in ("dead", "plain"):
        pol = _policy(dev, c["n"], E.KNOWN_B, pp=E.known_case(name, kind)["pp"])
        results[kind] = (_run_act(pol, obs[0], hidden, reset[0], None), _run_act(pol, other[0], hidden, reset[0], None),
                         _run_unroll(pol, obs, reset, hidden), _run_unroll(pol, other, reset, hidden))
        pol.close()
    a, b, ua, ub = results["dead"]
    for k in ("action", "mean", "logprob", "hidden"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ua:
        assert ua[k].tobytes() == ub[k].tobytes(), k
    assert not np.array_equal(a["value"], b["value"])
    _within(a["mean"], c["act"]["m64"]["mean"], c["act"]["tol"]["mean"], f"dead {name} mean")
    a, b, ua, ub = results["plain"]
    assert np.all(np.abs(a["mean"] - b["mean"]).max(axis=1) > 0) and np.all(np.abs(a["hidden"] - b["hidden"]).max(axis=1) > 0)
    assert not np.array_equal(ua["mean"], ub["mean"])


# ---- B4. flag values ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_every_non_zero_reset_flag_is_a_reset(dev, name):
    c = E.known_case(name, "plain")
    pol = _policy(dev, c["n"], E.KNOWN_B)
    obs, hidden = _t(c["obs"], dev), _t(c["hidden"], dev)
    one = _t(c["reset"], dev)
    base = _run_act(pol, obs[0], hidden, one[0], None)
    base_seq = _run_unroll(pol, obs, one, hidden)
    none = _run_unroll(pol, obs, torch.zeros_like(one), hidden)
    for t in range(E.KNOWN_T):                                                   # the flags matter at every tick
        assert base_seq["hidden_seq"][t].tobytes() != none["hidden_seq"][t].tobytes(), t
    for flag in E.FLAGS:
        reset = _t(E.flagged(c["reset"], flag), dev)
        assert int((reset == 1).sum()) == 0 and torch.equal(reset != 0, one != 0)
        got = _run_act(pol, obs[0], hidden, reset[0], None)
        for k in base:
            assert got[k].tobytes() == base[k].tobytes(), (flag, k)
        seq = _run_unroll(pol, obs, reset, hidden)
        for t in range(E.KNOWN_T):
            assert seq["mean"][t].tobytes() == base_seq["mean"][t].tobytes() and seq["hidden_seq"][t].tobytes() == base_seq["hidden_seq"][t].tobytes(), (flag, t)
        assert seq["hidden_last"].tobytes() == base_seq["hidden_last"].tobytes(), flag
    pol.close()


# ---- B5. non-finite inputs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_non_finite_inputs_stay_in_their_robot(dev, name):
    c = E.nonfinite_case(name)
    pol = _policy(dev, c["n"], E.KNOWN_B)
    reset = _t(c["reset"], dev)
    state = _state(c, dev)
    clean = _run_act(pol, _t(c["clean_obs"], dev), _t(c["clean_hidden"], dev), reset, state, sample=True)
    state = _state(c, dev)
    got = _run_act(pol, _t(c["obs"], dev), _t(c["hidden"], dev), reset, state, sample=True)
    others = np.setdiff1d(np.arange(E.KNOWN_B), E.SPOILT)
    for k in got:
        assert got[k][others].tobytes() == clean[k][others].tobytes(), k
    after = state.cpu().numpy()
    assert np.array_equal(after[0], c["keys"]) and np.array_equal(after[1], c["counters"] + 1)       # the spoilt robots' counters too
    rule = c["rule"]
    print(f"non-finite {name}: float32-numpy vs float64 model {rule['dev']}")
    spoilt = list(E.SPOILT)
    for k in ("mean", "value", "hidden"):
        _within(got[k][spoilt], rule["m64"][k][spoilt], rule["tol"][k], f"non-finite {name} {k}")
    assert np.array_equal(np.isnan(got["action"]), np.isnan(rule["m64"]["mean"])) and np.all(np.isfinite(got["logprob"]))
    assert np.all(np.isnan(got["hidden"][E.NAN_HIDDEN_ROBOT])) and np.all(np.isfinite(got["hidden"][[E.NAN_OBS_ROBOT, E.INF_OBS_ROBOT]]))
    pol.close()


# ---- B6. obs_clip ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip", E.CLIPS)
@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_obs_clip_zero_and_a_half_match_the_model(dev, name, clip):
    c = E.clip_case(name, clip)
    pol = _policy(dev, c["n"], E.KNOWN_B, clip=clip)
    assert pol._rnn.fields["obs_clip"] == clip
    got = _run_act(pol, _t(c["obs"], dev), _t(c["hidden"], dev), _t(c["reset"], dev), None)
    rule = c["rule"]
    print(f"clip {clip} {name}: float32-numpy vs float64 model {rule['dev']}")
    for k in ("mean", "value", "hidden"):
        _within(got[k], rule["m64"][k], rule["tol"][k], f"clip {clip} {name} {k}")
    pol.close()


# ---- B7. the noise stream beyond 32 bits ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.KNOWN_CONFIGS)
def test_noise_with_wide_keys_counters_and_seed(dev, name):
    c = E.wide_case(name)
    pol = _policy(dev, c["n"], E.KNOWN_B, seed=E.WIDE_SEED)
    state = _state(c, dev)
    got = _run_act(pol, _t(c["obs"], dev), _t(c["hidden"], dev), _t(c["reset"], dev), state, sample=True)
    m = c["rule"]["m64"]
    std = np.exp(m["logstd"].astype(np.float64))
    e = PM.eps_batch(E.WIDE_SEED, c["keys"], c["counters"], len(std)).astype(np.float64)
    rec = (got["action"].astype(np.float64) - got["mean"].astype(np.float64)) / std
    # the bound of tests/test_rnn_gpu.py::test_act_matches_the_model: the sum, the product, expf and the last float32 bit of eps
    bound = 1.01 * (np.abs(e) * (2.0 ** -24 + 2.0 ** -23 + 2.0 ** -22) + 2.0 ** -24 * np.abs(got["action"]) / std) + 1e-12
    print(f"wide {name}: worst |eps - model| / bound {float(np.max(np.abs(rec - e) / bound)):.3f}")
    assert np.all(np.abs(rec - e) <= bound), float(np.max(np.abs(rec - e) / bound))
    assert np.abs(got["logprob"] - m["logprob"]).max() <= 1e-5
    after = state.cpu().numpy()
    assert after.dtype == np.int64 and np.array_equal(after[0], c["keys"]) and np.array_equal(after[1], c["counters"] + 1)
    _within(got["mean"], m["mean"], c["rule"]["tol"]["mean"], f"wide {name} mean")
    pol.close()


# ---- C1, C2. the gradient at the edges of a wave, a row tile, a tile of robots and a chunk -----------------------------------------------

@pytest.mark.parametrize("name,T,B", E.EDGE_CASES)
def test_gradients_of_the_edge_configurations_match_the_model(dev, name, T, B):
    TB._check_gradient(dev, BC.case(name, T, B))


@pytest.mark.parametrize("name", list(BC.EDGE_CONFIGS))
def test_nothing_changed_since_the_rollout_gives_kl_zero_on_the_edge_configurations(dev, name):
    TB.test_nothing_changed_since_the_rollout_gives_kl_zero_and_ratio_one(dev, name)


@pytest.mark.parametrize("name,T,B", E.FULL_CASES)
def test_gradients_at_full_tiles_and_whole_chunks_match_the_model(dev, name, T, B):
    TB._check_gradient(dev, BC.case(name, T, B))


@pytest.mark.parametrize("name,T,B", E.LAST_LIVE_CASES)
def test_gradients_with_the_last_robot_valid_match_the_model(dev, name, T, B):
    """The cases of tests/bptt_cases.py mask the last robot of the batch throughout; here it is valid at every tick, and the
    workspace holds NaN before the call, so a last robot the delta pass never visited cannot pass for one without a gradient."""
    c = BC.case(name, T, B, mask_kind="last")
    assert np.all(c["mask"][:, B - 1] != 0) and np.all(c["mask"][:, 0] == 0)
    pol, ro = TB._policy(dev, c), TB._rollout(dev, c)
    upd = DeviceRecurrentPPO(pol, T, **c["ppo_kw"])
    upd.workspace.fill_(float("nan"))
    grad, loss = TB._grad(upd, ro)
    upd.close(), pol.close()
    err = BC.deviation(grad, c["p64"]["grad"], BM.tensors(c["lay"]))
    loss_err = abs(loss - c["p64"]["loss"]) / abs(c["p64"]["loss"])
    print(f"last robot valid, {name} T={T} B={B}: float32-numpy vs float64 {c['p_dev32']} loss {c['p_loss_dev32']:.3e}; kernel vs float64 {err} loss {loss_err:.3e}; "
          f"bounds {c['p_tol']} loss {c['p_loss_tol']:.3e}")
    for k, e in err.items():
        assert e <= c["p_tol"][k], (k, e, c["p_tol"][k])
    assert loss_err <= c["p_loss_tol"]
    TB._check_gradient(dev, c)                                                   # and the whole check of tests/test_bptt_gpu.py


# ---- C3. saturated gates in the backward pass ---------------------------------------------------------------------------------------------

def _gradient(dev, c, **replace):
    pol, ro = TB._policy(dev, c), TB._rollout(dev, c, **replace)
    upd = DeviceRecurrentPPO(pol, c["T"], **c["ppo_kw"])
    grad, loss = TB._grad(upd, ro)
    kl = upd.kl(ro).cpu().numpy()
    upd.close(), pol.close()
    return grad, loss, kl


@pytest.mark.parametrize("name,T,B", E.SATURATED_CASES)
def test_an_open_update_gate_passes_no_gradient_below_the_head(dev, name, T, B):
    c = BC.case(name, T, B, gates="hold")
    TB._check_gradient(dev, c)                                                   # every tensor and the loss within their bounds
    grad, _, _ = _gradient(dev, c)
    names = BM.tensors(c["lay"])
    for k in E.gate_tensors(c["lay"]):
        assert np.all(grad[names[k]] == 0.0), k
    for k in ("W_head", "b_head", "logstd"):
        assert np.abs(grad[names[k]]).max() > 0, k


@pytest.mark.parametrize("name,T,B", E.SATURATED_CASES)
def test_shut_gates_leave_the_gates_weights_and_the_h_rows_exactly_zero(dev, name, T, B):
    c = BC.case(name, T, B, gates="shut")
    lay, names, p64 = c["lay"], BM.tensors(c["lay"]), c["p64"]
    grad, loss, _ = _gradient(dev, c)
    i, o, w, _ = lay["w_c"]
    for what, s in (("W_ru", names["W_ru"]), ("b_ru", names["b_ru"]), ("h rows of W_c", slice(w + lay["n_x"] * o, w + i * o))):
        assert np.all(grad[s] == 0.0), what
    held = {k: s for k, s in names.items() if k not in E.SHUT_ZERO}
    err = BC.deviation(grad, p64["grad"], held)
    loss_err = abs(loss - p64["loss"]) / abs(p64["loss"])
    print(f"shut {name}: float32-numpy vs float64 { {k: c['p_dev32'][k] for k in held} } loss {c['p_loss_dev32']:.3e}; kernel vs float64 {err} loss {loss_err:.3e}; "
          f"bounds { {k: c['p_tol'][k] for k in held} } loss {c['p_loss_tol']:.3e}")
    for k, e in err.items():
        assert e <= c["p_tol"][k], (k, e, c["p_tol"][k])
    assert loss_err <= c["p_loss_tol"]
    assert np.abs(grad[w:w + lay["n_x"] * o]).max() > 0
    for k in names:
        if "dense" in k:
            assert np.abs(grad[names[k]]).max() > 0, k


# ---- C4. flag values --------------------------------------------------------------------------------------------------------------------

def test_mask_and_reset_flags_of_256_65536_and_int_min_count_as_one(dev):
    c = BC.case(*E.FLAG_CASE)
    base = _gradient(dev, c)
    assert np.abs(base[0]).max() > 0 and np.abs(base[2]).max() > 0
    for flag in (256, 65536, E.INT_MIN):
        mask, reset = E.flagged(c["mask"], flag), E.flagged(c["reset"], flag)
        assert (mask == np.int32(flag)).sum() > 10 and (reset == np.int32(flag)).sum() > 10
        got = _gradient(dev, c, mask=mask, reset=reset)
        assert got[0].tobytes() == base[0].tobytes() and got[1] == base[1] and got[2].tobytes() == base[2].tobytes(), flag


# ---- C5. the workspace guard ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,T,B", E.WORKSPACE_CASES)
def test_the_update_stays_inside_its_workspace(dev, name, T, B):
    c = BC.case(name, T, B)
    want, want_loss, want_kl = _gradient(dev, c)
    pol, ro = TB._policy(dev, c), TB._rollout(dev, c)
    upd = DeviceRecurrentPPO(pol, T, epochs_policy=2, epochs_value=1, **c["ppo_kw"])
    n = upd.workspace.numel()
    assert n * 8 == upd._handle.workspace_bytes
    big, upd.workspace = _guarded((n,), torch.float64, dev)
    assert upd.workspace.data_ptr() % 8 == 0
    upd.prepare(ro)
    grad, loss = upd.policy_grad(ro)
    assert grad.cpu().numpy().tobytes() == want.tobytes() and float(loss) == want_loss
    assert upd.kl(ro).cpu().numpy().tobytes() == want_kl.tobytes()
    torch.cuda.synchronize(dev)
    _bands_intact(big, written=False)
    upd.update(ro)
    torch.cuda.synchronize(dev)
    _bands_intact(big, written=False)
    assert upd.steps().tolist() == [2, 1] and bool(torch.isfinite(pol.policy_params).all())
    upd.close(), pol.close()
