"""The per-call inputs of a step on every step-kernel family (GPU): the wind, SoA sticks (`action_ld` > 0), held sticks in a k-step
launch, and the rows a step only writes - accel, done bits, the episode rows, `action_out` - through the plain [noise][obj][kahan]
kernels, the guidance-override kernels, the AoS head, the fp16 pair, the Racer, the table kernels, the gate kernels and the
"k = 1 of the k-step kernel" route.  Each family reads these through plumbing of its own (the FPV_STEP_PARAMS prefix, the views
that re-read the kernel-argument segment by offset, the wrapped argument structs, the gate kernel's ninth parameter); a mistake
there is invisible to a zero wind, a row-layout action and a null pointer.  Expected values are the host lane model's
(tests/call_inputs.py) bit for bit; tests/test_call_inputs_host.py shows on the CPU that these flights hold the oracle's bars and
that the wind moves every drone by 100 x the bar."""
import numpy as np
import pytest
import torch

import call_inputs as ci
from fpyv_amd import _lib
from fpyv_amd.env import DroneBatch, RacerBatch
from oracle import lane_model
from parity import REL_TOL, assert_parity
from test_lane_model import FP16_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIND, CALM, SIZES, STEPS = ci.WIND, ci.CALM, ci.SIZES, ci.STEPS
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _id(row):
    return "-".join(str(x) for x in row)


def _dev(x):
    return torch.from_numpy(np.array(x, order="C", copy=True)).to(DEV)


def _same(got, want, what):
    g = np.ascontiguousarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got)
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at element {bad[:4] // g.dtype.itemsize} of shape {g.shape}"


def _batch(row, n, **kw):
    """A handle of the row's family with the row's first n drones at their starts (the state is uploaded: every family starts
    from the bits the host flight starts from)"""
    fl = ci.row_flight(row)
    if row[0] == "book":                                        # the row's family on the flight's parameters under a ceiling
        row = row[1]
        kw.update(auto_reset=True)
    kind = row[0]
    p, init = fl["p"], fl["init"]
    noise = dict(stick_noise=True, noise_seed=ci.NOISE_SEED, with_action_out=True)
    source = kind in ("reset", "table_reset") or row == ("gate", "reset")
    if kind == "plain":
        kw.update(noise if row[1] else {}, kahan_position=bool(row[3]))
    elif kind in ("table", "table_reset"):
        kw.update(noise if kind == "table" and row[1] else {}, per_drone_physics=True)
    elif kind == "gate":
        kw.update(noise if row[1] == "noise" else {}, gates=ci.gate_rows(row)[0], laps=1 if row[1] == "finish" else 0)
    elif kind == "fp16":
        kw.update(fp16_state=True, rounding_seed=5)
    if source:
        kw.update(auto_reset=True, per_drone_reset_pose=True)
    b = DroneBatch(p, n, device=DEV, **kw)
    if kind in ("table", "table_reset"):
        from physics_sets import dealt
        inp = dealt(ci.table_sets(p), n)[1]
        b.set_physics(mass=inp[:, 0], thrust_poly=inp[:, 1:5], drag_coefficients=inp[:, 5:8], rates_transition_rate=inp[:, 8],
                      thrust_transition_rate=inp[:, 9])
    if source:
        b.reset(position=fl["pos"][:n], velocity=fl["vel"][:n], ypr=fl["ypr"][:n])
        _same(b.reset_pose[:, :n], init[0:10, :n], "the reset-pose table is the start the host flight resets to")
    elif kind == "gate":
        b.reset()                                               # (the words: at gate 0, nothing passed)
    if kind == "fp16":
        h = ci.host_h()
        pairs, thrust = b._state_h_views()
        b.state[:, :n] = _dev(h["pos0"][:, :n])
        pairs[:, :n] = _dev(h["sh0"][:10 * ci.N].reshape(5, ci.N, 2)[:, :n].view(np.int16))
        thrust[:n] = _dev(h["sh0"][10 * ci.N:10 * ci.N + n].view(np.int16))
    else:
        b.state[:, :n] = _dev(init[:, :n])
    return b


def _extra(row, n, t):
    """the keyword arguments of single step t of the row: its object list, its guidance call"""
    fl = ci.row_flight(row)
    row = row[1] if row[0] == "book" else row
    kw = dict(object_list=list(fl["objects"])) if fl["objects"] else {}
    if row[0] == "override":
        R, f = _override(n)
        kw.update(rotation_matrix=R, thrust_force=f[t])
    return kw


_OVERRIDE = {}


def _override(n):
    if n not in _OVERRIDE:
        R, f = ci.override_inputs(n)
        _OVERRIDE[n] = (_dev(R), _dev(f))
    return _OVERRIDE[n]


def _run(b, row, how, a, wind, rewards=None, dones=None):
    """k = a.shape[0] steps of the row's sticks on handle b: `step` k calls, `rollout` the issued launches of fpv_rollout, `step_n`
    one launch of the k-step kernel, `graph` fpv_rollout_graph.  Per-step rewards / dones go to the given [k, n] rows."""
    k, n = a.shape[0], b.n
    objects = list(ci.row_flight(row)["objects"]) or None
    if how == "step":
        for t in range(k):
            b.step(a[t], wind_velocity_vector=wind, return_imu=False, **_extra(row, n, t))
            if rewards is not None:
                rewards[t].copy_(b.reward)
                dones[t].copy_(b.done)
        return
    kw = dict(rollout=dict(fused=False), step_n=dict(fused=True), graph=dict(graph=True))[how]
    if rewards is not None:
        kw.update(rewards=rewards, dones=dones)
    b.rollout(a, wind=wind, object_list=objects, **kw)


def _check_end(b, row, e, n, what, t=-1, outputs=True):
    """handle b after step t of host flight e (whose first n columns are b's drones): every row the family writes"""
    _same(b.state[:, :n], e["snaps"][t][:, :n], f"{what}: state")
    if outputs:
        _same(b.reward, e["reward"][t][:n], f"{what}: reward")
        _same(b.done, e["done"][t][:n], f"{what}: done")
    if b.accel is not None:
        _same(b.accel[:, :n], e["accel"][t][:, :n], f"{what}: accel")
    if b.pos_comp is not None and t == -1:
        _same(b.pos_comp[:, :n], e["comp"][:, :n], f"{what}: pos_comp")
    if b.noise_state is not None and t == -1:
        _same(b.noise_state[:, :n], e["ns"][:, :n], f"{what}: noise_state")
        _same(b.action_out, e["acts"][t][:n], f"{what}: action_out is lane_model.stick_noise")
    if b.gate_word is not None:
        _same(b.gate_word.view(torch.int32), e["words"][t][:n].view(np.int32), f"{what}: gate word")
        _same(b.gate_obs.contiguous(), e["obs"][t][:n], f"{what}: gate_obs")
    assert not bool(b.state[:, n:].any()), f"{what}: columns past n were written"


def _check_oracle_and_drift(row, got, calm, n, what):
    """the two properties of the arithmetic, on the kernel's own end states: the oracle's bar under the wind, and a calm flight
    that ends 100 bars away (tests/test_call_inputs_host.py: the host build gives both)"""
    err = ci.oracle_error(row, got, n)
    lanes = ci.compared_lanes(row)
    lanes = lanes[lanes < n]
    if err is None:
        return
    assert_parity(err, REL_TOL, what)
    a, c = got[0:3, lanes].astype(np.float64), calm[0:3, lanes].astype(np.float64)
    d = (np.linalg.norm(a - c, axis=0) / np.linalg.norm(a, axis=0)).min()
    assert d >= 100 * REL_TOL, f"{what}: zero wind ends only {d:.2e} of |p| away"


def _state(b):
    torch.cuda.synchronize()
    return b.state.cpu().numpy()


# ---- 1. wind through every family that reads it -------------------------------------------------------------------------------
PLAIN = [("plain", noise, obj, kahan) for noise in (0, 1) for obj in (0, 1) for kahan in (0, 1)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", PLAIN, ids=_id)
def test_wind_plain_kernels(row, n):
    """The eight plain instantiations, single steps and one launch of the k-step kernel (without an object list the X-frame SQ
    body: no ground flag): state, reward, done, accel, pos_comp, noise_state bit for bit the lane model's under the wind, and
    `action_out` the host generator's sticks"""
    e = ci.host(row)
    a = _dev(ci.row_flight(row)["acts"][:, :n])
    for how in ("step", "step_n"):
        b = _batch(row, n)
        _run(b, row, how, a, WIND)
        _check_end(b, row, e, n, f"{_id(row)} {how} n={n}")
    calm = _batch(row, n)
    _run(calm, row, "step_n", a, CALM)
    _check_oracle_and_drift(row, _state(b), _state(calm), n, _id(row))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", [("override", 0), ("override", 1)], ids=_id)
def test_wind_override_kernels(row, n):
    """step(..., rotation_matrix=, thrust_force=) with a third of the thrusts NaN: the lane model with set_override, bit for bit;
    oracle.drone_run_guided at REL_TOL on every eighth drone"""
    e = ci.host(row)
    a = _dev(ci.row_flight(row)["acts"][:, :n])
    b, calm = _batch(row, n), _batch(row, n)
    _run(b, row, "step", a, WIND)
    _check_end(b, row, e, n, f"{_id(row)} n={n}")
    _run(calm, row, "step", a, CALM)
    _check_oracle_and_drift(row, _state(b), _state(calm), n, _id(row))


@pytest.mark.parametrize("n", SIZES)
def test_wind_aos_head(n):
    """the 16-column rows of the AoS-head kernel: the lane model's state and accel under the wind"""
    row = ("plain", 0, 0, 0)
    e = ci.host(row)
    a = _dev(ci.row_flight(row)["acts"][:, :n])
    b, calm = _batch(row, n, with_obs_aos=True), _batch(row, n, with_obs_aos=True)
    b.obs_aos.fill_(float("nan"))
    _run(b, row, "step", a, WIND)
    _check_end(b, row, e, n, f"AoS head n={n}")
    _same(b.obs_aos[:, 0:13], e["snaps"][-1][0:13, :n].T, "obs_aos: the state columns")
    _same(b.obs_aos[:, 13:16], e["accel"][-1][:, :n].T, "obs_aos: the accel columns")
    _run(calm, row, "step", a, CALM)
    _check_oracle_and_drift(row, _state(b), _state(calm), n, "AoS head")


def _storage(b, n):
    torch.cuda.synchronize()
    h, ld = b.state_h.cpu().numpy().view(np.uint16), b.ld
    return b.state.cpu().numpy()[:, :n], h[:10 * ld].reshape(5, ld, 2)[:, :n], h[10 * ld:10 * ld + n]


@pytest.mark.parametrize("n", SIZES)
def test_wind_fp16_kernels(n):
    """fp16 storage, single steps and the k-step kernel: lane_model.run_h under the wind, bit for bit on the position rows, the
    pair rows and the thrust halves; the oracle within FP16_TOL; a calm flight ends 100 x the position bar (in metres) away"""
    row, N = ("fp16",), ci.N
    want = ci.host_h(WIND)
    a = _dev(ci.row_flight(row)["acts"][:, :n])
    for how in ("step", "step_n"):
        b = _batch(row, n)
        _run(b, row, how, a, WIND)
        pos, pairs, thrust = _storage(b, n)
        _same(pos, want["pos"][:, :n], f"fp16 {how}: position rows")
        _same(pairs, want["sh"][:10 * N].reshape(5, N, 2)[:, :n], f"fp16 {how}: pair rows")
        _same(thrust, want["sh"][10 * N:10 * N + n], f"fp16 {how}: thrust halves")
        _same(b.reward, want["reward"][:n], f"fp16 {how}: reward")
        _same(b.done_u8, want["done"][:n], f"fp16 {how}: done")
    calm = _batch(row, n)
    _run(calm, row, "step_n", a, CALM)
    ends = []
    for x in (b, calm):
        torch.cuda.synchronize()
        words = torch.cat([x._state_h_views()[0][:, :n].reshape(-1), x._state_h_views()[1][:n]]).cpu().numpy().view(np.uint16)
        ends.append(lane_model.join_half(x.state.cpu().numpy()[:, :n], words))
    err = ci.oracle_error(row, ends[0], n)
    for k, tol in FP16_TOL.items():
        assert err[k] <= tol, (k, err[k], n)
    d = np.linalg.norm(ends[0][0:3].astype(np.float64) - ends[1][0:3], axis=0).min()
    assert d >= 100 * FP16_TOL["pos_rel"], f"zero wind ends only {d:.3f} m away"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", [("table", noise, world) for noise in (0, 1) for world in ("plain", "ground", "objects")], ids=_id)
def test_wind_table_kernels(row, n):
    """A table handle, [noise][obj], ground rows loaded (ground flag, object list) and not: fpv_step, fpv_rollout, fpv_step_n and
    fpv_rollout_graph leave the lane model of each drone's airframe under the wind"""
    e = ci.host(row)
    a = _dev(ci.row_flight(row)["acts"][:, :n])
    for how in ("step", "rollout", "step_n", "graph"):
        b = _batch(row, n)
        _run(b, row, how, a, WIND)
        _check_end(b, row, e, n, f"{_id(row)} {how} n={n}")
    calm = _batch(row, n)
    _run(calm, row, "step_n", a, CALM)
    _check_oracle_and_drift(row, _state(b), _state(calm), n, _id(row))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", [("gate", v) for v in ("plain", "noise", "objects", "reset")], ids=_id)
def test_wind_gate_kernels(row, n):
    """A gate handle: the single-step kernel (plain) or the k = 1 route (noise, object list, reset source) through `step`, and
    the k-step kernels through fpv_step_n with per-step outputs.  The state is the lane model's under the wind; word, reward,
    done and gate_obs are the host's fpv_gate_eval over that trajectory, on every step"""
    e = ci.host(row)
    a = _dev(ci.row_flight(row)["acts"][:, :n])
    for how in ("step", "step_n"):
        b = _batch(row, n)
        rew, don = torch.zeros((STEPS, n), device=DEV), torch.zeros((STEPS, n), dtype=torch.bool, device=DEV)
        _run(b, row, how, a, WIND, rew, don)
        what = f"{_id(row)} {how} n={n}"
        _check_end(b, row, e, n, what, outputs=how == "step")
        _same(rew, e["reward"][:, :n], f"{what}: per-step rewards")
        _same(don, e["done"][:, :n], f"{what}: per-step dones")
    quiet = _batch(row, n)
    _run(quiet, row, "step_n", a, WIND)                         # no per-step outputs: the quiet loop
    _check_end(quiet, row, e, n, f"{_id(row)} quiet step_n n={n}")
    calm = _batch(row, n)
    _run(calm, row, "step_n", a, CALM)
    _check_oracle_and_drift(row, _state(b), _state(calm), n, _id(row))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", [("reset", 0), ("reset", 1)], ids=_id)
def test_wind_reset_source_route(row, n):
    """per_drone_reset_pose=True without and with jitter under a ceiling the even lanes climb through: `step` (the k-step kernel,
    k = 1) and fpv_step_n leave the lane model's state, with fpv_reset_pose_sample's pose in every lane that reset"""
    e = ci.host(row)
    a = _dev(ci.row_flight(row)["acts"][:, :n])
    for how in ("step", "step_n"):
        b = _batch(row, n)
        _run(b, row, how, a, WIND)
        _check_end(b, row, e, n, f"{_id(row)} {how} n={n}")
    calm = _batch(row, n)
    _run(calm, row, "step_n", a, CALM)
    _check_oracle_and_drift(row, _state(b), _state(calm), n, _id(row))


def test_the_racer_has_no_wind_term():
    n, k = 129, 24
    rng = np.random.default_rng(5)
    a = _dev(np.concatenate([rng.uniform(-6, 6, (k, n, 3)), rng.uniform(0, 8, (k, n, 1))], axis=2).astype(np.float32))
    x, y = RacerBatch(None, n, device=DEV), RacerBatch(None, n, device=DEV)
    x.reset(); y.reset()
    for t in range(k):
        x._step_raw(a[t], WIND)
        y._step_raw(a[t])
    x.rollout(a, wind=WIND); y.rollout(a)
    assert torch.equal(x.state.view(torch.int32), y.state.view(torch.int32)) and torch.equal(x.reward, y.reward)


# ---- 2. SoA sticks through every kernel that accepts them --------------------------------------------------------------------
SOA_ROWS = (PLAIN + [("override", 0), ("override", 1)] + [("table", noise, world) for noise in (0, 1) for world in ("plain", "objects")]
            + [("gate", "plain"), ("gate", "noise"), ("gate", "objects"), ("reset", 0), ("table_reset",)])


def _soa(rows, pad=5):
    """[n, 4] sticks as a [4, n] view of a [4, n + pad] tensor whose padding columns are NaN"""
    n = rows.shape[0]
    t = torch.full((4, n + pad), float("nan"), device=DEV)
    t[:, :n] = rows.t()
    return t[:, :n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", SOA_ROWS, ids=_id)
def test_soa_sticks(row, n):
    """Two single steps fed as [4, n] views (row stride n + 5, NaN in the padding; every cell of the stick tensor differs): bit
    for bit the same steps fed as [n, 4] rows, and bit for bit the lane model.  With stick noise the SoA tensor is the base
    action; the gate handle's ragged last block (n = 1, 63, 129, 1000) sends its lanes past the end through the `il = 0` loads;
    a gate handle with noise or an object list, a reset-source handle and a table handle with one land on a k-step kernel's
    loads (k = 1)."""
    s0 = ci.soa_sticks(n)
    acts = np.stack([s0, np.ascontiguousarray(s0[:, ::-1]) * np.float32(0.5)])
    e = ci.fly_row(row, acts, n)
    rows, soa = _batch(row, n), _batch(row, n)
    a = _dev(acts)
    for t in range(2):
        rows.step(a[t], wind_velocity_vector=WIND, return_imu=False, **_extra(row, n, t))
        view = _soa(a[t])
        assert view.shape == (4, n) and view.stride() == (n + 5, 1)
        soa.step(view, wind_velocity_vector=WIND, return_imu=False, **_extra(row, n, t))
        assert soa._buf.action_ld == n + 5 and rows._buf.action_ld == 0
    for name in ("state", "reward", "done", "accel", "pos_comp", "noise_state", "action_out", "gate_word", "gate_obs_rows"):
        x, y = getattr(rows, name), getattr(soa, name)
        assert (x is None and y is None) or torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{_id(row)} n={n}: {name} differs between the layouts"
    _check_end(soa, row, e, n, f"{_id(row)} SoA n={n}")
    assert soa.step_counter() == 2


def test_soa_sticks_are_refused_by_name_where_no_kernel_reads_them():
    """fp16, Racer and AoS-head handles and fpv_step_n refuse action_ld through the C ABI's buffers; the refusal leaves the step
    counter where it was and the handle usable"""
    n = 129
    L = _lib.lib()
    a = torch.zeros((n, 4), device=DEV)
    view = _soa(a)
    p = ci.flight("plain")["p"]
    handles = [(DroneBatch(p, n, device=DEV, fp16_state=True), L.fpv_step), (RacerBatch(None, n, device=DEV), L.fpv_step),
               (DroneBatch(p, n, device=DEV, with_obs_aos=True), L.fpv_step), (DroneBatch(p, n, device=DEV), None)]
    for b, fn in handles:
        b.reset()
        torch.cuda.synchronize()
        before = b.state.clone()
        b._buf.action, b._buf.action_ld = view.data_ptr(), view.stride(0)
        if fn is not None:
            rc, msg = fn(b._handle, b._buf_ref, b._stream()), "SoA actions (action_ld) are supported by the fp32 drone kernel without obs_aos"
        else:
            rc, msg = L.fpv_step_n(b._handle, b._buf_ref, 3, 0, 0, b._stream()), "fpv_step_n reads action rows [n][4] only"
        assert rc == -1 and msg in L.fpv_last_error().decode(), (rc, L.fpv_last_error())
        with pytest.raises(_lib.FpvError, match="action_ld must be >= n"):
            b._buf.action_ld = n - 1
            _lib.check((fn or L.fpv_step)(b._handle, b._buf_ref, b._stream()))
        torch.cuda.synchronize()
        assert b.step_counter() == 0 and torch.equal(b.state, before)
        b._step_raw(a)                                          # the next ordinary step
        assert b.step_counter() == 1 and b._buf.action_ld == 0
        torch.cuda.synchronize()


# ---- 3. held sticks and steps= on the non-plain k-step kernels -----------------------------------------------------------------
def _racer(kind, n):
    pid = np.array([[0.004, 0.02, 1e-6], [0.003, 0.01, 2e-6], [0.002, 0.005, 0]])
    p = ci.flight("plain")["p"].replace(mode=1, racer_pid=pid, racer_omega_dt=(kind == "racer"), ceiling=5e-4)
    if kind == "racer_cpid":
        p = p.replace(racer_pid=-pid, racer_pid_variant=1, pid_integral_clip=0.05, pid_min_output=-0.004, pid_max_output=0.006,
                      pid_derivative_transition_rate=0.3)
    b = RacerBatch(p, n, device=DEV, auto_reset=True, track_episodes=True)
    b.reset()
    return b


HELD_ROWS = ([("fp16",), ("racer",), ("racer_written",), ("racer_cpid",)] + [("table", noise, world) for noise in (0, 1) for world in ("plain", "objects")]
             + [("gate", v) for v in ("plain", "noise", "objects")])


@pytest.mark.parametrize("k", [1, 2, 3, 24])
@pytest.mark.parametrize("row", HELD_ROWS, ids=_id)
def test_held_sticks_in_a_k_step_launch(row, k):
    """rollout(a[n, 4], steps=k) - action_stride 0 - on the fp16, Racer, table and gate k-step kernels: the bits of k single steps
    of the same sticks, with per-step rewards / dones and without (the quiet loop takes two steps per trip: k = 1, 2, 3, 24), and
    the lane model's where there is one; on noise handles rollout(None, steps=k) as well"""
    n = 129
    racer = row[0].startswith("racer")
    make = (lambda: _racer(row[0], n)) if racer else (lambda: _batch(row, n))
    if racer:
        rng = np.random.default_rng(5)
        held = np.concatenate([rng.uniform(-6, 6, (n, 3)), rng.uniform(0, 8, (n, 1))], axis=1).astype(np.float32)
    else:
        held = ci.soa_sticks(n)
    a = _dev(held)
    objects = None if racer else (list(ci.row_flight(row)["objects"]) or None)
    noise = (row[0] == "table" and bool(row[1])) or row == ("gate", "noise")
    for sticks in ([a, None] if noise else [a]):
        what = f"{_id(row)} k={k} sticks={'held' if sticks is not None else 'none'}"
        one = make()
        rew1, don1 = torch.zeros((k, n), device=DEV), torch.zeros((k, n), dtype=torch.bool, device=DEV)
        for t in range(k):
            if racer:
                one.step(sticks)
            else:
                one.step(sticks, wind_velocity_vector=WIND, return_imu=False, **_extra(row, n, t))
            rew1[t].copy_(one.reward)
            don1[t].copy_(one.done)
        for per_step in (False, True):
            many = make()
            rew, don = torch.zeros((k, n), device=DEV), torch.zeros((k, n), dtype=torch.bool, device=DEV)
            out = dict(rewards=rew, dones=don) if per_step else {}
            many.rollout(sticks, steps=k, fused=True, wind=None if racer else WIND, object_list=objects, **out)
            for name in ("state", "state_h", "noise_state", "action_out", "gate_word", "gate_obs_rows", "accel", "ep_return", "ep_length",
                         "last_return", "last_length"):
                x, y = getattr(one, name), getattr(many, name)
                assert (x is None and y is None) or torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what} per_step={per_step}: {name}"
            if per_step:
                assert torch.equal(rew, rew1) and torch.equal(don, don1), what
            else:
                assert torch.equal(many.reward, one.reward) and torch.equal(many.done, one.done), what
            assert many.step_counter() == one.step_counter() == k
        if racer:
            continue
        if row[0] == "fp16":
            h = ci.host_h()
            pos, sh = h["pos0"].copy(), h["sh0"].copy()
            d, r = ci.fly_h(ci.flight("fp16")["p"], pos, sh, np.broadcast_to(held, (k, n, 4)).copy(), WIND)
            got = _storage(many, n)
            _same(got[0], pos[:, :n], "fp16 held: position rows")
            _same(got[1], sh[:10 * ci.N].reshape(5, ci.N, 2)[:, :n], "fp16 held: pair rows")
            _same(got[2], sh[10 * ci.N:10 * ci.N + n], "fp16 held: thrust halves")
            _same(rew, r, "fp16 held: per-step rewards")
            continue
        e = ci.fly_row(row, np.broadcast_to(held, (k, n, 4)).copy(), n) if sticks is not None else _pure_noise_flight(row, k, n)
        _check_end(many, row, e, n, f"{what} against the lane model", outputs=False)
        _same(rew, e["reward"][:, :n], f"{what}: per-step rewards against the lane model")
        _same(don, e["done"][:, :n], f"{what}: per-step dones against the lane model")


def _pure_noise_flight(row, k, n):
    """`fly_row` of a noise row flown on the generator's sticks alone (rollout(None, steps=k))"""
    p = ci.row_flight(row)["p"]
    applied, ns = lane_model.stick_noise(p, n, k, noise_seed=ci.NOISE_SEED)
    quiet = ("table", 0, row[2]) if row[0] == "table" else ("gate", "plain")
    e = ci.fly_row(quiet, applied, n)
    e["acts"], e["ns"] = applied, ns[:, :n]
    return e


# ---- 4. written-only rows and episode bookkeeping per family -----------------------------------------------------------------
BOOK_ROWS = [("book", r) for r in (("gate", "finish"), ("gate", "noise"), ("gate", "objects"), ("table", 0, "plain"), ("table", 1, "plain"),
                                   ("table", 0, "objects"), ("table", 1, "objects"), ("override", 0), ("override", 1), ("fp16",))]


@pytest.mark.parametrize("n", [129, 897])
@pytest.mark.parametrize("row", BOOK_ROWS, ids=lambda r: _id(r[1]))
def test_written_only_rows_and_episode_bookkeeping(row, n):
    """Everything the batch can allocate for the family - accel, the episode rows, done bits, `action_out` with noise - on a handle
    that resets its lanes (a ceiling, crashes, a one-lap course): accel is the lane model's; done_bits unpacked are the dones and
    the sentinel words past ceil(n / 64) of every bucket row stay (n % 128 in 1..64); the episode rows are the NumPy restatement
    over the per-step rewards and dones, exactly; and single steps and the k-step launch agree on all of it"""
    k, base = STEPS, row[1]
    words = (n + 63) // 64
    fl = ci.row_flight(row)
    acts = fl["acts"][:k, :n]
    a = _dev(acts)
    runs = {}
    hows = ("step",) if base[0] == "override" else ("step", "step_n")
    for how in hows:
        b = _batch(row, n, with_accel=True, track_episodes=True, with_done_bits=True)
        rew, don = torch.zeros((k, n), device=DEV), torch.zeros((k, n), dtype=torch.bool, device=DEV)
        bits = torch.full((k, words + 2), SENTINEL, dtype=torch.int64, device=DEV)
        if how == "step":
            for t in range(k):
                b.set_done_bits_target(bits[t])
                b.step(a[t], wind_velocity_vector=WIND, return_imu=False, **_extra(row, n, t))
                rew[t].copy_(b.reward)
                don[t].copy_(b.done)
        else:
            b.set_done_bits_target(bits, stride_words=words + 2)
            b.rollout(a, wind=WIND, rewards=rew, dones=don, object_list=list(fl["objects"]) or None)
        torch.cuda.synchronize()
        rew, don, bits = rew.cpu().numpy(), don.cpu().numpy(), bits.cpu().numpy()
        runs[how] = (b, rew, don, bits)
        what = f"{_id(base)} {how} n={n}"
        assert don.any(), f"{what}: no episode ended"
        _same(ci.unpack_bits(bits[:, :words], n), don, f"{what}: done_bits unpacked")
        assert (bits[:, words:].view(np.uint64) == SENTINEL).all(), f"{what}: words past ceil(n / 64) were written"
        assert not (np.ascontiguousarray(bits[:, words - 1]).view(np.uint64) >> np.uint64(n - 64 * (words - 1))).any(), f"{what}: bits past n are set"
        for name, want in zip(("ep_return", "ep_length", "last_return", "last_length"), ci.episode_rows(rew, don)):
            _same(getattr(b, name), want, f"{what}: {name}")
    if base[0] == "fp16":
        h = ci.host_h()
        pos, sh = h["pos0"].copy(), h["sh0"].copy()
        d, r = ci.fly_h(fl["p"], pos, sh, np.ascontiguousarray(acts), WIND, auto_reset=True)
        e = dict(done=d, reward=r)
    else:
        e = ci.fly_row(row, acts, n)
    for how in hows:
        b, rew, don, _ = runs[how]
        _same(rew, e["reward"][:, :n], f"{_id(base)} {how}: per-step rewards against the host")
        _same(don, e["done"][:, :n], f"{_id(base)} {how}: per-step dones against the host")
        if base[0] != "fp16":
            _check_end(b, base, e, n, f"{_id(base)} {how} n={n}", outputs=False)
    if len(hows) == 2:
        x, y = runs["step"][0], runs["step_n"][0]
        for name in ("state", "state_h", "accel", "ep_return", "ep_length", "last_return", "last_length", "noise_state", "action_out", "gate_word"):
            u, v = getattr(x, name), getattr(y, name)
            assert (u is None and v is None) or torch.equal(u.view(torch.uint8), v.view(torch.uint8)), f"{_id(base)} n={n}: {name} step != step_n"
        for i in (1, 2, 3):
            assert np.array_equal(runs["step"][i], runs["step_n"][i]), f"{_id(base)} n={n}: per-step outputs step != step_n"


# ---- 5. the wind is part of a graph's shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [("plain", 0, 0, 0), ("table", 0, "plain")], ids=_id)
def test_a_replayed_graph_flies_the_wind_of_its_call(row):
    """Two rollout(..., graph=True) calls with another wind bound between them equal the issued launches with the same winds (a
    stale replay would fly the first wind twice), and the lane model"""
    n, k = 1000, 24
    fl = ci.row_flight(row)
    acts = fl["acts"][:2 * k, :n]
    a = _dev(acts)
    other = (-0.5, 0.25, 1.5)
    g, r = _batch(row, n), _batch(row, n)
    for c, wind in enumerate((WIND, other)):
        g.rollout(a[c * k:(c + 1) * k], wind=wind, graph=True)
        r.rollout(a[c * k:(c + 1) * k], wind=wind, fused=False)
    for name in ("state", "reward", "done", "accel"):
        assert torch.equal(getattr(g, name).view(torch.uint8), getattr(r, name).view(torch.uint8)), name
    start = ci.fly_row(row, acts[:k], n, wind=WIND)["snaps"][-1]
    fly = (lambda w: ci.fly_table(ci.table_sets(fl["p"]), start, acts[k:], wind=w)) if row[0] == "table" else (lambda w: ci.fly(fl["p"], start, acts[k:], wind=w))
    second, stale = fly(other), fly(WIND)
    _same(g.state[:, :n], second["snaps"][-1], "graph: state after the second wind")
    _same(g.accel[:, :n], second["accel"][-1], "graph: accel after the second wind")
    assert not np.array_equal(stale["snaps"][-1], second["snaps"][-1])
