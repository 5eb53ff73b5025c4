"""State rows without a GPU: the layout the library reports matches the Python description, a row as a reset leaves it
passes rg_mpc_state_check, every single corruption is refused naming the robot and the field, and the gather / scatter
kernels (rg_mpc_state.hip) cross-compile for gfx950 without scratch."""
import io
import pickle

import numpy as np
import pytest

from robot_gym_amd.core import controller_state as CS
from robot_gym_amd.core import mpc_abi
from robot_gym_amd.core.config import MPCConfig
from tests import kernel_checks


def reset_rows(cfg, n, t0=0.25):
    """n rows as rg_reset_kernel leaves a robot (robot k in row k)."""
    row_bytes, desc = mpc_abi.state_layout(cfg)
    st = CS.ControllerState(np.zeros((n, row_bytes), np.uint8), desc, np.arange(n))
    h = st.header()
    hs = CS.layout_hash(desc)
    h[:, 0], h[:, 1], h[:, 2], h[:, 3], h[:, 4] = CS.MAGIC, CS.VERSION, hs & 0xFFFFFFFF, hs >> 32, np.arange(n)
    st.field("reset_time")[:] = t0
    st.field("flags")[:] = 3
    st.field("last_desired")[:] = sum((s & 1) << l for l, s in enumerate(cfg.init_state))
    st.field("warm_key")[:] = -1
    return st


@pytest.mark.parametrize("window", [1, 20, 64])
@pytest.mark.parametrize("horizon", [10, 20])
def test_layout_matches_the_python_description(window, horizon):
    row_bytes, desc = mpc_abi.state_layout(MPCConfig.for_robot("ghost", window=window, horizon=horizon))
    kv, fl = CS.parse_layout(desc)
    want, want_bytes = CS.offsets(window)
    assert row_bytes == want_bytes == int(kv["row_bytes"])
    assert list(fl) == [f[0] for f in CS.fields(window)]
    assert fl == want
    assert int(kv["window"]) == window and int(kv["horizon"]) == horizon and int(kv["warm_n"]) == CS.WARM_N and int(kv["ws_max"]) == CS.WS_MAX
    # the warm start dominates: ~2.5 KB per robot at the default window
    assert window != 20 or 2400 < row_bytes < 2800


def test_layout_hash_covers_window_and_horizon():
    descs = {mpc_abi.state_layout(MPCConfig.for_robot("ghost", window=w, horizon=hz))[1] for w in (1, 20) for hz in (10, 20)}
    assert len({CS.layout_hash(d) for d in descs}) == 4


def test_reset_row_passes_and_round_trips():
    cfg = MPCConfig.for_robot("ghost")
    st = reset_rows(cfg, 5)
    st.check(cfg)
    st.check(cfg, dst=[4, 3, 2, 1, 0], batch=5)
    st2 = pickle.loads(pickle.dumps(st))
    assert np.array_equal(st2.rows, st.rows) and st2.layout == st.layout and list(st2.indices) == list(range(5))
    buf = io.BytesIO()
    np.save(buf, st.rows)
    buf.seek(0)
    st3 = CS.ControllerState(np.load(buf))
    assert list(st3.indices) == list(range(5))
    st3.check(cfg)


def _corrupt(cfg, mutate, k=3):
    st = reset_rows(cfg, 6)
    st.field("ring_len")[:] = 2          # a few samples held: the ring check has slots to look at
    st.field("ring_head")[:] = 2
    mutate(st, k)
    return st


W = 20
CORRUPTIONS = {
    "magic": (lambda st, k: st.header().__setitem__((k, 0), 0x12345678), "header"),
    "version": (lambda st, k: st.header().__setitem__((k, 1), 7), "header"),
    "layout_hash": (lambda st, k: st.header().__setitem__((k, 2), st.header()[k, 2] ^ 1), "header"),
    "ring_len": (lambda st, k: st.field("ring_len").__setitem__(k, W + 1), "ring_len"),
    "ring_head": (lambda st, k: st.field("ring_head").__setitem__(k, W), "ring_head"),
    "ws_cnt": (lambda st, k: st.field("ws_cnt").__setitem__(k, CS.WS_MAX + 1), "ws_cnt"),
    "ws_ids": (lambda st, k: st.field("ws_ids").__setitem__((k, 7), 250), "ws_ids"),
    "warm_key": (lambda st, k: st.field("warm_key").__setitem__(k, 16), "warm_key"),
    "flags": (lambda st, k: st.field("flags").__setitem__(k, 3 | 8), "flags"),
    "last_desired": (lambda st, k: st.field("last_desired").__setitem__(k, 0x10), "last_desired"),
    "swing_valid": (lambda st, k: st.field("swing_valid").__setitem__(k, 0x1000), "swing_valid"),
    "hard": (lambda st, k: st.field("hard").__setitem__(k, 17), "hard"),
    "iters": (lambda st, k: st.field("iters").__setitem__(k, -5), "iters"),
    "fsum_nan": (lambda st, k: st.field("fsum").__setitem__((k, 1), np.nan), "fsum"),
    "reset_time_inf": (lambda st, k: st.field("reset_time").__setitem__(k, np.inf), "reset_time"),
    "ring_nan": (lambda st, k: st.field("ring").__setitem__((k, W + 1), np.nan), "ring"),
    "swing_q_nan": (lambda st, k: (st.field("swing_valid").__setitem__(k, 0x7), st.field("swing_q").__setitem__((k, 2), np.nan)), "swing_q"),
    "warm_z_nan": (lambda st, k: (st.field("warm_key").__setitem__(k, 9), st.field("warm_z").__setitem__((k, 100), np.nan)), "warm_z"),
}


@pytest.mark.parametrize("name", sorted(CORRUPTIONS))
def test_each_single_corruption_is_refused_naming_robot_and_field(name):
    cfg = MPCConfig.for_robot("ghost")
    mutate, field = CORRUPTIONS[name]
    st = _corrupt(cfg, mutate)
    with pytest.raises(mpc_abi.RgMpcError) as e:
        st.check(cfg)
    assert "robot 3" in str(e.value) and field in str(e.value), str(e.value)
    # the robot named is the destination the row goes to
    with pytest.raises(mpc_abi.RgMpcError) as e:
        st.check(cfg, dst=[10, 11, 12, 13, 14, 15], batch=16)
    assert "robot 13" in str(e.value) and field in str(e.value), str(e.value)


def test_values_the_step_never_reads_are_not_checked():
    cfg = MPCConfig.for_robot("ghost")
    st = reset_rows(cfg, 2)
    st.field("swing_q")[1, 5] = np.nan     # swing_valid clear: no stored angle yet
    st.field("warm_z")[1, 3] = np.nan      # warm_key -1: no stored iterate
    st.field("ring")[1, 0] = np.nan        # ring_len 0: no sample held
    st.field("cmd")[1, 0] = np.nan         # a non-finite command is the step's own counted failure
    st.check(cfg)


def test_truncated_buffer_and_duplicate_destinations_are_refused():
    cfg = MPCConfig.for_robot("ghost")
    st = reset_rows(cfg, 4)
    lib = mpc_abi.load_library()
    import ctypes as C
    cc = mpc_abi.make_cconfig(cfg)
    assert lib.rg_mpc_state_check(C.byref(cc), st.rows.ctypes.data, 4, st.rows.nbytes - 1, None, 0) == -1
    assert b"truncated" in mpc_abi.load_library().rg_mpc_last_error(None)
    with pytest.raises(mpc_abi.RgMpcError, match="truncated"):
        mpc_abi.state_check(cfg, st.rows.reshape(-1)[:-8].reshape(1, -1))
    with pytest.raises(mpc_abi.RgMpcError, match=r"robot 2\): destination robot repeated"):
        st.check(cfg, dst=[0, 2, 1, 2], batch=4)
    with pytest.raises(mpc_abi.RgMpcError, match="out of range"):
        st.check(cfg, dst=[0, 1, 2, 4], batch=4)
    # another window: the layout hash (and the row size) differ
    with pytest.raises(mpc_abi.RgMpcError):
        st.check(MPCConfig.for_robot("ghost", window=21))


def test_state_kernels_cross_compile_without_scratch():
    rows = kernel_checks.remarks("rg_mpc_state.hip")
    assert set(rows) == {"rg_state_gather_kernel", "rg_state_scatter_kernel"}, sorted(rows)
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)


def test_index_lists_outside_int32_are_refused_not_wrapped():
    assert list(mpc_abi._i32_array(np.array([0, 5, (1 << 31) - 1], dtype=np.int64))) == [0, 5, (1 << 31) - 1]
    for bad in ([(1 << 32) + 3], np.array([(1 << 32) + 3], dtype=np.uint64), [-(1 << 31) - 1], [1.5]):
        with pytest.raises(ValueError):
            mpc_abi._i32_array(bad)
