"""The inputs of tests/test_gpu_call_inputs.py are fair (CPU): for exactly the starts, sticks, step counts, airframes and wind the GPU
module flies (tests/call_inputs.py), the host lane model - which the kernels must equal bit for bit - holds the existing bars
against the float64 oracle, and the wind moves every drone by at least 100 x that bar, so a kernel that dropped, swapped or
misread the wind could not pass.  The GPU is asked for nothing the host build of the arithmetic cannot give."""
import numpy as np
import pytest

import call_inputs as ci
from oracle import lane_model
from parity import REL_TOL, assert_parity
from test_lane_model import FP16_TOL

ROWS = ([("plain", noise, obj, kahan) for noise in (0, 1) for obj in (0, 1) for kahan in (0, 1)] + [("override", 0), ("override", 1)]
        + [("table", noise, world) for noise in (0, 1) for world in ("plain", "ground", "objects")]
        + [("gate", v) for v in ("plain", "noise", "objects", "reset")] + [("reset", 0), ("reset", 1)])


def _id(row):
    return "-".join(str(x) for x in row)


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_lane_model_holds_the_bar_under_the_wind_and_the_wind_shows(row):
    """Measured here (1000 drones, 300 steps at 400 per second, wind (1, -2, 0.5)), worst over all rows: position 2.5e-6 relative
    and 5.2e-6 per component, quaternion 6.1e-7 - against REL_TOL = 1e-5; the smallest drift |p_wind - p_calm| / |p_wind| of any
    drone is 1.5e-3 (table, plain world: the airframe with the least drag) and 3.1e-3 or more off the table rows - against 100 x REL_TOL =
    1e-3.  Where lanes reset, the lanes that never end an episode are compared (every odd lane of the reset-source flights)."""
    windy, calm = ci.host(row, ci.WIND), ci.host(row, ci.CALM)
    err = ci.oracle_error(row, windy["snaps"][-1], ci.N)
    lanes = ci.compared_lanes(row)
    d = ci.drift(windy, calm, lanes)
    print(_id(row), f"{len(lanes)} lanes, pos_rel {err['pos_rel']:.2e} pos_comp {err['pos_comp']:.2e} quat_abs {err['quat_abs']:.2e} drift {d:.2e}")
    assert len(lanes) >= 100
    assert_parity(err, REL_TOL, _id(row))
    assert_parity(ci.oracle_error(row, calm["snaps"][-1], ci.N, wind=ci.CALM), REL_TOL, _id(row) + " (calm)")
    assert d >= 100 * REL_TOL, f"{_id(row)}: the wind moves some drone by only {d:.2e} of |p|"


def test_fp16_storage_holds_its_bar_under_the_wind_and_the_wind_shows():
    """fp16 storage, 300 steps at 120 per second (2.5 s).  Measured: pos_rel 1.3e-3, vel_rel 2.4e-3, quat_abs 1.1e-3 against FP16_TOL
    = 4e-3 / 1.5e-2 / 5e-3.  The wind moves every drone by 1.7 m or more: 100 x the position bar taken in metres (0.4 m).  As a
    fraction of |p| the drift is 3e-2, and no flight of 300 steps reaches 0.4: the wind cannot carry a drone further than its own
    speed times the flight (11 m in 300 steps at 60 per second, where the drift is 6e-2 of |p| and the lane model's own error is
    within a factor 3 of the bar), so the distance is asserted."""
    ends = {}
    for wind in (ci.WIND, ci.CALM):
        h = ci.host_h(wind)
        ends[wind] = lane_model.join_half(h["pos"], h["sh"])
        err = ci.oracle_error(("fp16",), ends[wind], ci.N, wind=wind)
        print("fp16", wind, {k: f"{err[k]:.2e}" for k in FP16_TOL})
        for k, tol in FP16_TOL.items():
            assert err[k] <= tol, (wind, k, err[k])
    d = np.linalg.norm(ends[ci.WIND][0:3, :ci.N].astype(np.float64) - ends[ci.CALM][0:3, :ci.N], axis=0)
    print(f"fp16 drift {d.min():.2f} m")
    assert d.min() >= 100 * FP16_TOL["pos_rel"]


def test_the_flights_visit_what_their_rows_are_for():
    """The object list is hit, the ceiling ends episodes on some lanes and never on others, gates are passed and missed, lanes of
    the gate flights crash and climb out, the noise generator moves the sticks, NaN thrusts leave drone-steps un-overridden."""
    assert ci.host(("plain", 0, 1, 0))["done"].any(0).sum() >= 100 and ci.host(("table", 0, "objects"))["done"].any(0).sum() >= 100
    for row in (("reset", 0), ("reset", 1), ("gate", "reset")):
        d = ci.host(row)["done"]
        assert d.any(0).sum() >= 100 and (~d.any(0)).sum() >= 100, row
        assert row[0] != "reset" or d[:24].any(0).sum() >= 20, "the short k-step launches must see resets too"
    for v in ("plain", "noise", "objects", "reset"):
        ev = (ci.host(("gate", v))["words"] >> 8) & 3
        assert ((ev == 1).any(0)).sum() >= 50 and ((ev == 2).any(0)).sum() >= 50, v
    assert ci.host(("gate", "objects"))["phys_done"].any(0).sum() >= 50
    assert not np.array_equal(ci.host(("plain", 1, 0, 0))["acts"], ci.flight("plain")["acts"])
    f = ci.override_inputs(ci.N)[1]
    assert 0.2 < np.isnan(f).mean() < 0.5
    jit, tab = ci.host(("reset", 1)), ci.host(("reset", 0))
    assert not np.array_equal(jit["snaps"][-1], tab["snaps"][-1]), "the jitter must move the reset poses"


def test_a_smaller_population_flies_the_first_columns():
    """What this module asserts for 1000 drones holds for the n = 1, 63, 129 of the GPU module: the flight of n drones is the first n
    columns, bit for bit - sticks, starts, the noise streams, the deal of the airframes and the reset samples are prefixes."""
    for row in (("plain", 1, 0, 1), ("table", 1, "ground"), ("reset", 1)):
        fl, whole = ci.row_flight(row), ci.host(row)
        for n in (1, 63, 129):
            acts = fl["acts"][:, :n]
            if row[1] and row[0] != "reset":
                acts, ns = ci.noise_sticks(fl["p"], acts, n)
                assert np.array_equal(ns, whole["ns"][:, :n])
            if row[0] == "plain":
                e = ci.fly(fl["p"], fl["init"][:, :n], acts, kahan=True)
                assert np.array_equal(e["comp"], whole["comp"][:, :n])
            elif row[0] == "table":
                e = ci.fly_table(ci.table_sets(fl["p"]), fl["init"][:, :n], acts)
            else:
                e = ci.fly(fl["p"], fl["init"][:, :n], acts, reset=ci.reset_source(fl["p"], fl["init"], n))
            for name in ("snaps", "accel", "done", "reward"):
                assert np.array_equal(e[name].view(np.uint8), np.ascontiguousarray(whole[name][..., :n]).view(np.uint8)), (row, n, name)


def test_the_per_step_model_is_the_lane_model_in_one_call():
    """`fly` steps the lane model one step at a time; the same flight in one call (what the other suites compare kernels with) ends
    on the same bits - state, accel, reward, done and the Kahan rows"""
    fl = ci.flight("objects")
    e = ci.host(("plain", 0, 1, 1))
    s = np.ascontiguousarray(fl["init"]).copy()
    comp = np.zeros((6, ci.N), np.float32)
    try:
        lane_model.set_objects(fl["objects"])
        lane_model.set_pos_comp(comp)
        _, acc, done, rew = lane_model.run(fl["p"], s, fl["acts"], wind=ci.WIND)
    finally:
        lane_model.set_objects(())
        lane_model.set_pos_comp(None)
    assert np.array_equal(s.view(np.uint32), e["snaps"][-1].view(np.uint32)) and np.array_equal(comp, e["comp"])
    assert np.array_equal(acc.view(np.uint32), e["accel"][-1].view(np.uint32)) and np.array_equal(done.astype(bool), e["done"][-1])
    assert np.array_equal(rew.view(np.uint32), e["reward"][-1].view(np.uint32))


def test_the_stick_tensor_of_the_layout_tests_tells_every_cell_apart():
    for n in ci.SIZES:
        a = ci.soa_sticks(n)
        assert a.shape == (n, 4) and a.dtype == np.float32 and np.unique(a).size == a.size and np.abs(a).max() < 1.0
        assert np.abs(a[:, 3] - a[:, 0]).min() > 1e-3 or n > 129


def test_episode_rows_and_done_bits_restatements():
    r = np.array([[1.0, 2.0], [0.5, 0.25], [4.0, 8.0]], np.float32)
    d = np.array([[0, 1], [0, 0], [1, 0]], bool)
    ep_r, ep_l, last_r, last_l = ci.episode_rows(r, d)
    assert ep_r.tolist() == [0.0, 8.25] and ep_l.tolist() == [0, 2] and last_r.tolist() == [5.5, 2.0] and last_l.tolist() == [3, 1]
    assert ep_r.dtype == np.float32 and last_l.dtype == np.int32
    bits = np.array([[1 | (1 << 63), 5]], np.uint64).view(np.int64)
    got = ci.unpack_bits(bits, 67)
    assert got.shape == (1, 67) and np.flatnonzero(got[0]).tolist() == [0, 63, 64, 66]
