"""The PPO agent's kernels (include/rg_policy.h) at their edges, on the inputs of tests/policy_edges.py (the model alone runs
over them in tests/test_policy_edges_cpu.py): the networks' arithmetic bit for bit against the exact float32 model, the
normaliser's transform made observable through a one-hot value head, the noise stream with keys, counters and a seed beyond
32 bits, guard bands around every output, record and returns at their shape and state edges, and a non-default stream.

The bound on the mean.  The value head is linear, so `value` is predicted bit for bit by PM.forward_exact (checked against
the C library's fmaf on the CPU).  The mean head ends in the device's tanhf; its accuracy is documented by ROCm, but no such
figure is installed with the toolchain these tests run on (its headers and documentation were searched for tanhf and for ULP
figures), so the mean keeps the rule of tests/test_policy_gpu.py: 8 x the deviation of numpy's float32 model from the float64
model over the test's inputs, floor 1e-6, formed from the model alone.  What changes is the reference: tanh in float64 of the
EXACT float32 pre-activation, so the bound is left with tanhf's own error and one rounding.  The largest error is printed,
in float32 ulps of the result too.

Measured on an MI355X: value bit-exact in all nine (configuration, batch) cases; tanhf at most 7.1e-8 (1.19 float32 ulps of
the result, wave_edges at B = 1037) against a bound of 8.7e-6, and 3.7e-8 or less elsewhere against bounds of 1e-6 .. 4.1e-6;
the transform exact in all 3465 entries that must be (4 x 832 under count <= 1, 137 clipped ones), and none of the 3191
scaled entries used the one-ulp allowance; the
cancellation case: mean exact, var_sum off by at most 1.6e-13 against bounds of 5.4e-10 .. 6.0e-10 (rtol 1e-12 would have
been 2.2e-14 .. 2.7e-14)."""
import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import BatchedGaussianPolicy, RolloutBuffer
from robot_gym_amd.core import policy_abi
from tests import policy_edges as E
from tests import policy_model as PM

pytestmark = pytest.mark.gpu

HEAD = dict(act_dim=1, policy_layers=(), value_layers=())    # the smallest networks, for the tests of record and returns
GUARD = 96
F_SENTINEL, I_SENTINEL = -12345.5, -77777


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _t(a, dev=None):
    """A tensor holding a copy of a (the shared inputs are read-only arrays)."""
    return torch.as_tensor(np.array(a), device=dev)


def _policy(dev, B, name, state, clip=5.0):
    """A policy of configuration `name` and batch B holding the edge parameters, the given normaliser state and the first B act
    states of the pool."""
    lay, pp, vp = E.params(name)
    pol = BatchedGaussianPolicy(B, seed=E.SEED, device=dev, obs_clip=clip, **E.config_of(name))
    assert pol.layout == lay
    with torch.no_grad():
        pol.policy_params.copy_(_t(pp))
        pol.value_params.copy_(_t(vp))
    pol.norm_state.copy_(_t(state))
    pol.act_state.copy_(_t(np.stack(E.act_states(B))))
    return pol


def _outs(pol, fill=7.0):
    B, A = pol.batch, pol.act_dim
    f = dict(dtype=torch.float32, device=pol.device)
    return dict(action=torch.full((B, A), fill, **f), mean=torch.full((B, A), fill, **f), value=torch.full((B,), fill, **f), logprob=torch.full((B,), fill, **f))


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


_acts = {}


def act_run(dev, name, B):
    """Once per (configuration, batch): two sampling acts in a row (the second draws at counter + 1) and a MEAN act, under an
    identity normaliser state (empty for a batch of one, one sample otherwise)."""
    if (name, B) not in _acts:
        c = E.act_case(name, B, "empty" if B == 1 else "count1")
        pol = _policy(dev, B, name, c["state"])
        obs = _t(c["obs"], dev)
        first = _np(pol.act(obs, sample=True, out=_outs(pol)))
        state1 = pol.act_state.cpu().numpy()
        second = _np(pol.act(obs, sample=True, out=_outs(pol)))
        state2 = pol.act_state.cpu().numpy()
        det = _np(pol.act(obs, sample=False, out=_outs(pol)))
        state3 = pol.act_state.cpu().numpy()
        pol.close()
        _acts[(name, B)] = dict(c=c, first=first, second=second, det=det, states=(state1, state2, state3))
    return _acts[(name, B)]


CASES = [(name, B) for name, batches in E.BATCHES.items() for B in batches]


# ---- a. the networks' arithmetic ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", CASES)
def test_value_is_the_headers_arithmetic_bit_for_bit_and_the_mean_its_tanh(dev, name, B):
    """value == forward_exact: acc = 0, fma in order, then the bias, relu as where(v > 0), a function of the configuration
    alone.  mean against tanh (float64) of the exact float32 pre-activation, within the 8 x rule of the module docstring: no
    documented tanhf accuracy is installed here, so none is used."""
    r = act_run(dev, name, B)
    c, got = r["c"], r["first"]
    want = c["value_exact"]
    diff = got["value"] != want                                  # values, not bytes: +0 == -0
    if diff.any():
        k = int(np.flatnonzero(diff)[0])
        print(f"{name} B={B}: value differs for {int(diff.sum())} robots; robot {k}: kernel {got['value'][k]!r} ({got['value'][k:k + 1].view(np.uint32)[0]:#x}) "
              f"model {want[k]!r} ({want[k:k + 1].view(np.uint32)[0]:#x})")
    assert not diff.any()
    m64, m32 = c["m64"], c["m32"]
    dev_mean = float(np.abs(m32["mean"].astype(np.float64) - m64["mean"]).max())
    tol = max(8.0 * dev_mean, 1e-6)
    ref = np.tanh(c["pre_exact"].astype(np.float64))
    err = np.abs(got["mean"].astype(np.float64) - ref)
    ulps = err / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print(f"{name} B={B}: value bit-exact for {B} robots; tanhf: largest error {err.max():.3e} ({ulps.max():.2f} float32 ulps of the result), bound {tol:.3e}")
    assert err.max() <= tol
    for other in (r["second"], r["det"]):                        # the networks do not depend on the mode or the counter
        assert np.array_equal(other["value"], got["value"]) and np.array_equal(other["mean"], got["mean"])
    assert np.array_equal(r["det"]["action"], r["det"]["mean"])


def test_value_does_not_depend_on_the_batch_or_the_place_in_the_tile(dev):
    """The smaller batches are the pool's first robots: the same robot gives the same bits at B = 1, 13 and 1037 (first tile,
    ragged tile, another workgroup's neighbours)."""
    big, mid, one = (act_run(dev, "wave_edges", B)["det"] for B in (1037, 13, 1))
    # B = 1 runs under the empty state, the others under one sample: compare 13 with 1037 directly, and 1 with the model only
    for k in ("value", "mean"):
        assert np.array_equal(big[k][:13], mid[k])
    assert one["value"].shape == (1,)


# ---- b. the transform, observable ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip", E.CLIPS)
@pytest.mark.parametrize("kind", E.NORM_STATES)
def test_transform_through_a_one_hot_value_head(dev, kind, clip):
    """A head-only value network with weight row e_i and bias 0 gives value = x_i exactly (fma(1, x_i, 0), then fma(0, x_k, x_i)
    and + 0).  With count <= 1 (no division) and at every clipped entry the kernel's x must equal the model's float32 x; a
    scaled entry may be one float32 ulp off, where the device's sqrt or division rounds the float64 quotient the other way at
    a float32 boundary.  How many entries used that ulp is printed."""
    d, B = E.TRANSFORM["obs_dim"], E.TRANSFORM_BATCH
    x, v64, scaled = E.transform_x(kind, clip, d, B)
    pol = _policy(dev, B, "transform", E.norm_state(kind, d), clip)
    obs = _t(E.observations(d)[:, :B], dev)
    rows = torch.full((d, B), F_SENTINEL, dtype=torch.float32, device=dev)
    action = torch.zeros(B, 1, dtype=torch.float32, device=dev)
    assert pol.value_params.numel() == d + 1
    with torch.no_grad():
        for i in range(d):
            pol.value_params.zero_()
            pol.value_params[i] = 1.0
            pol.act(obs, sample=False, out=dict(action=action, value=rows[i]))
    got = rows.cpu().numpy().T
    pol.close()
    exact = ~scaled[None, :] | ((np.abs(v64) >= clip) if clip > 0 else np.zeros_like(v64, dtype=bool))
    assert np.array_equal(got[exact], x[exact]), (kind, clip, int((got[exact] != x[exact]).sum()))
    loose = ~exact
    off = got[loose] != x[loose]
    near = (got[loose] == np.nextafter(x[loose], np.float32(np.inf))) | (got[loose] == np.nextafter(x[loose], np.float32(-np.inf)))
    print(f"transform {kind} clip {clip}: {int(exact.sum())} entries exact, {int(loose.sum())} scaled entries of which {int(off.sum())} used the one-ulp allowance")
    assert np.all(~off | near)
    if kind in ("empty", "count1"):
        assert exact.all()


# ---- c. the noise stream beyond 32 bits -------------------------------------------------------------------------------------

def _check_noise(c, got, counters, B):
    m = c["m64"]
    std = np.exp(m["logstd"].astype(np.float64))
    e = PM.eps_batch(E.SEED, c["keys"], counters, len(std)).astype(np.float64)
    rec = (got["action"].astype(np.float64) - got["mean"].astype(np.float64)) / std
    # the bound of tests/test_policy_gpu.py: the sum, the product, expf and the last float32 bit of eps
    bound = 1.01 * (np.abs(e) * (2.0 ** -24 + 2.0 ** -23 + 2.0 ** -22) + 2.0 ** -24 * np.abs(got["action"]) / std) + 1e-12
    assert np.all(np.abs(rec - e) <= bound), float(np.max(np.abs(rec - e) / bound))
    assert np.abs(got["logprob"] - PM.logprob(e.astype(np.float32), m["logstd"])).max() <= 1e-5


@pytest.mark.parametrize("name,B", [("head_only", 1), ("head_only", 13), ("wave_edges", 13), ("wave_edges", 1037)])
def test_noise_with_wide_keys_counters_and_seed(dev, name, B):
    """act_dim 1 and 4.  Keys such as -1, -2^63, 2^32 + 5, counters such as 2^32 - 1 (the increment crosses 32 bits: the second
    act draws at 2^32) and 2^62, a seed above 2^63: a draw from any of them cast to 32 bits differs (the CPU test)."""
    r = act_run(dev, name, B)
    c = r["c"]
    keys, counters = c["keys"], c["counters"]
    _check_noise(c, r["first"], counters, B)
    _check_noise(c, r["second"], counters + 1, B)
    for k, state in enumerate(r["states"]):
        assert state.dtype == np.int64 and np.array_equal(state[0], keys)                 # keys untouched
        assert np.array_equal(state[1], counters + min(k + 1, 2))                          # + 1 per sampling act as int64, MEAN leaves it
    assert not np.array_equal(r["first"]["action"], r["second"]["action"])


# ---- d. guard bands -----------------------------------------------------------------------------------------------------------

def _guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    sentinel = F_SENTINEL if dtype == torch.float32 else I_SENTINEL
    big = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=dev)
    return big, big[GUARD:GUARD + n].view(*shape)


def _bands_intact(big, written=True):
    sentinel = F_SENTINEL if big.dtype == torch.float32 else I_SENTINEL
    a = big.cpu().numpy()
    assert np.all(a[:GUARD] == sentinel) and np.all(a[-GUARD:] == sentinel)
    if written:
        assert not np.any(a[GUARD:-GUARD] == sentinel)           # and the slice itself was filled


@pytest.mark.parametrize("B", [13, 257])
def test_no_output_is_written_past_its_ends(dev, B):
    """Every output of act, record and returns is a contiguous slice out of the middle of a larger tensor filled with a
    sentinel; after the call the bands before and after it still hold the sentinel."""
    name, f32, i32 = "policy_deeper", torch.float32, torch.int32
    c = E.act_case(name, 13, "count1")
    A, d = c["cfg"]["act_dim"], c["cfg"]["obs_dim"]
    pol = _policy(dev, B, name, c["state"])
    obs_np = np.array(E.observations(d)[:, :B])
    obs = _t(obs_np, dev)
    bigs, out = {}, {}
    for k, shape in (("action", (B, A)), ("mean", (B, A)), ("value", (B,)), ("logprob", (B,))):
        bigs[k], out[k] = _guarded(shape, f32, dev)
    for sample in (True, False):
        pol.act(obs, sample=sample, out=out)
        for big in bigs.values():
            _bands_intact(big)
    if B == 13:
        assert np.array_equal(out["value"].cpu().numpy(), c["value_exact"])
    # record: the three slots
    rng = np.random.default_rng(B)
    reward = torch.as_tensor(rng.normal(size=B).astype(np.float32), device=dev)
    done = torch.as_tensor(rng.integers(0, 2, B).astype(np.int32), device=dev)
    big_o, ro_obs = _guarded((d, B), f32, dev)
    big_r, ro_reward = _guarded((B,), f32, dev)
    big_d, ro_done = _guarded((B,), i32, dev)
    pol.record(obs, reward, done, None, ro_obs, ro_reward, ro_done)
    for big in (big_o, big_r, big_d):
        _bands_intact(big)
    assert np.array_equal(ro_obs.cpu().numpy(), obs_np) and torch.equal(ro_reward, reward) and torch.equal(ro_done, done)
    # returns: ret and adv
    T = 3
    ro = RolloutBuffer(T, B, d, A, device=dev)
    ro.reward.copy_(torch.as_tensor(rng.normal(size=(T, B)).astype(np.float32)))
    ro.value.copy_(torch.as_tensor(rng.normal(size=(T, B)).astype(np.float32)))
    big_ret, ro.ret = _guarded((T, B), f32, dev)
    big_adv, ro.adv = _guarded((T, B), f32, dev)
    pol.returns(ro)
    _bands_intact(big_ret), _bands_intact(big_adv)
    pol.close()


# ---- e. record -----------------------------------------------------------------------------------------------------------------

def _check_state(got, want):
    got, want = got.reshape(3, -1), want.reshape(3, -1)
    assert np.array_equal(got[0], want[0])                                   # the count is exact
    assert np.allclose(got[1], want[1], rtol=1e-12, atol=0) and np.allclose(got[2], want[2], rtol=1e-12, atol=0)


def _record_run(dev, case, slots=("obs", "reward", "done"), check=True):
    """The ticks of a record case on a policy that starts from the case's state.  -> the state after every tick."""
    d, B = case["obs_dim"], case["B"]
    pol = BatchedGaussianPolicy(B, obs_dim=d, device=dev, **HEAD)
    pol.norm_state.copy_(_t(case["state0"]))
    f32 = dict(dtype=torch.float32, device=dev)
    states = []
    for obs, reward, done, mask in case["ticks"]:
        ro = dict(obs=torch.full((d, B), F_SENTINEL, **f32) if "obs" in slots else None, reward=torch.full((B,), F_SENTINEL, **f32) if "reward" in slots else None,
                  done=torch.full((B,), I_SENTINEL, dtype=torch.int32, device=dev) if "done" in slots else None)
        m = None if mask is None else _t(mask, dev)
        pol.record(_t(obs, dev), _t(reward, dev), _t(done, dev), m, ro["obs"], ro["reward"], ro["done"])
        if check:
            for k, src in (("obs", obs), ("reward", reward), ("done", done)):
                if ro[k] is not None:
                    assert np.array_equal(ro[k].cpu().numpy(), src), k
        states.append(pol.norm_state.cpu().numpy())
    pol.close()
    return states


@pytest.mark.parametrize("name", ["obs64", "obs1_256", "obs1_257", "obs1_65536", "obs1_65537", "count_2_40"])
def test_record_edges_match_the_model(dev, name):
    """obs_dim 64 (all 65 columns; the reward's workspace column is its norm_state column) and 1; B at the workgroup boundary
    (256 / 257) and at the stride boundary (65536 / 65537: robot 65536 is workgroup 0's second trip); masks holding -1, 2^31 - 1
    and -2^31, which select; a count of 2^40 before the update, which stays an exact integer."""
    case = E.record_case(name)
    got = _record_run(dev, case)
    for g, w in zip(got, case["states"]):
        _check_state(g, w)
    count = got[-1].reshape(3, -1)[0]
    assert count[0] == case["state0"][0] + sum(case["n"]) and count[PM.NORM_REWARD] == count[0] and float(count[0]).is_integer()
    d = case["obs_dim"]
    assert not got[-1].reshape(3, -1)[:, d:PM.NORM_REWARD].any()             # the columns not in use stay empty


@pytest.mark.parametrize("name", ["obs64", "obs1_257"])
def test_record_with_null_slots_updates_the_same_state(dev, name):
    """Each of the three slots NULL in turn, and all three: norm_state is byte-identical to the run with every slot given."""
    case = E.record_case(name)
    full = _record_run(dev, case)[-1]
    _check_state(full, case["want"])
    for slots in (("reward", "done"), ("obs", "done"), ("obs", "reward"), ()):
        assert _record_run(dev, case, slots)[-1].tobytes() == full.tobytes(), slots


def test_record_first_tick_under_cancellation(dev):
    """The first update from the empty state (mean = 0) over values of mean 1e4 and spread 1e-2: var_sum = sum v (v - new_mean)
    cancels five digits, so the suite's rtol = 1e-12 cannot be derived: the order of summation matters.  The bound is the
    order-independent n 2^-53 sum|(v - mean)(v - new_mean)| against the exact sum (rational arithmetic over the float64 new
    mean), and n 2^-53 sum|v - mean| / n for the mean, both from the inputs alone.  The observed errors are printed."""
    case = E.record_case("cancel")
    got = _record_run(dev, case)[-1].reshape(3, -1)
    assert got[0, 0] == 257 and got[0, PM.NORM_REWARD] == 257
    for r in E.cancel_bounds():
        err_mean, err_var = abs(got[1, r["col"]] - r["exact_mean"]), abs(got[2, r["col"]] - r["exact_var"])
        print(f"cancellation, column {r['col']}: mean off by {err_mean:.3e} (bound {r['bound_mean']:.3e}), var_sum {r['exact_var']:.6e} off by {err_var:.3e} "
              f"(bound {r['bound_var']:.3e}; rtol 1e-12 would be {1e-12 * r['exact_var']:.3e})")
        assert err_mean <= r["bound_mean"] and err_var <= r["bound_var"]


# ---- f. returns ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.RETURNS))
def test_returns_edges_match_the_model(dev, name):
    """B = 257 and 1037 (more than one workgroup), T = 1 and 300, discount 0, 0.5 and 1, lambda 0 and 0.95, reward_clip = 0, a
    reward normaliser of count 0 and 1, done holding 2 and -1, a column done at every tick; without bootstrap the last value is
    a NULL pointer, through policy_abi.PolicyHandle.  Tolerance: 1e-6 max(|want|, 1), the float32 rounding of the output."""
    c = E.returns_case(name)
    B, T = c["B"], c["T"]
    f32 = dict(dtype=torch.float32, device=dev)
    reward, value, last, done, state = (_t(c[k], dev) for k in ("reward", "value", "last", "done", "state"))
    ret, adv = torch.full((T, B), F_SENTINEL, **f32), torch.full((T, B), F_SENTINEL, **f32)
    settings = dict(obs_dim=1, discount=c["discount"], gae_lambda=c["lam"], reward_clip=c["reward_clip"], **HEAD)
    if c["bootstrap"]:
        pol = BatchedGaussianPolicy(B, device=dev, **settings)
        pol.norm_state.copy_(state)
        ro = RolloutBuffer(T, B, 1, 1, device=dev)
        ro.reward, ro.value, ro.done, ro.last_value, ro.ret, ro.adv = reward, value, done, last, ret, adv
        pol.returns(ro, bootstrap=True)
        pol.close()
    else:
        h = policy_abi.PolicyHandle(B, dev, **settings)
        h.returns(reward.data_ptr(), value.data_ptr(), done.data_ptr(), None, state.data_ptr(), T, False, ret.data_ptr(), adv.data_ptr())
        torch.cuda.synchronize(dev)
        h.close()
    for got, want in ((ret.cpu().numpy(), c["ret"]), (adv.cpu().numpy(), c["adv"])):
        err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
        assert err.max() <= 1e-6, (name, float(err.max()), np.unravel_index(err.argmax(), err.shape))


# ---- g. a non-default stream ------------------------------------------------------------------------------------------------

def _pipeline(dev, stream):
    """act (sampling), record and returns at B = 257 on `stream` (None: the default stream), their results copied to pinned
    host memory on the same stream; only that stream is waited for.  -> the bytes of every result."""
    name, B, T = "policy_deeper", 257, 4
    c = E.act_case(name, 13, "count1")
    A, d = c["cfg"]["act_dim"], c["cfg"]["obs_dim"]
    pol = _policy(dev, B, name, c["state"])
    rng = np.random.default_rng(77)
    obs = _t(E.observations(d)[:, :B], dev)
    reward = torch.as_tensor(rng.normal(size=B).astype(np.float32), device=dev)
    done = torch.as_tensor(rng.integers(0, 2, B).astype(np.int32), device=dev)
    ro = RolloutBuffer(T, B, d, A, device=dev)
    ro.reward.copy_(torch.as_tensor(rng.normal(size=(T, B)).astype(np.float32)))
    ro.value.copy_(torch.as_tensor(rng.normal(size=(T, B)).astype(np.float32)))
    ro.done.copy_(torch.as_tensor(rng.integers(0, 2, (T, B)).astype(np.int32)))
    ro.ret.fill_(F_SENTINEL), ro.adv.fill_(F_SENTINEL)
    out = _outs(pol, F_SENTINEL)
    slots = dict(ro_obs=torch.full((d, B), F_SENTINEL, dtype=torch.float32, device=dev), ro_reward=torch.full((B,), F_SENTINEL, dtype=torch.float32, device=dev),
                 ro_done=torch.full((B,), I_SENTINEL, dtype=torch.int32, device=dev))
    results = dict(out, **slots, ret=ro.ret, adv=ro.adv, norm_state=pol.norm_state, act_state=pol.act_state)
    host = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in results.items()}
    torch.cuda.synchronize(dev)                     # the inputs are in place before another stream reads them
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        pol.act(obs, sample=True, out=out)
        pol.record(obs, reward, done, None, **slots)
        pol.returns(ro)
        for k, v in results.items():
            host[k].copy_(v, non_blocking=True)
    s.synchronize()                                 # this stream alone
    got = {k: v.numpy().tobytes() for k, v in host.items()}
    torch.cuda.synchronize(dev)
    pol.close()
    return got


def test_a_non_default_stream_gives_the_same_bytes(dev):
    base = _pipeline(dev, None)
    other = _pipeline(dev, torch.cuda.Stream(dev))
    sentinel = np.float32(F_SENTINEL).tobytes()
    for k in base:
        assert other[k] == base[k], k
    for k in ("action", "mean", "value", "logprob", "ro_obs", "ro_reward", "ret", "adv"):
        assert sentinel not in [other[k][i:i + 4] for i in range(0, len(other[k]), 4)], k     # complete after the stream's own synchronize
