"""fp32 error budget of the kernel's per-lane arithmetic (fpyv_amd/csrc/fpv_math.h compiled for
the host by oracle/lane_model.cpp) against the float64 oracle, on the golden stick profiles.
Runs without a GPU; the GPU tests then require the gfx950 kernel to reproduce this arithmetic."""
import numpy as np
import pytest

from conftest import load_golden, params_for_golden, racer_params_for_golden
from oracle import lane_model, oracle
from parity import REL_TOL, assert_parity, soa_vs_oracle


def _both(p, g, steps=None):
    acts = g["actions"] if steps is None else g["actions"][:steps]
    n = acts.shape[1]
    ref = oracle.drone_initial_state(n, g["init_position"], g["init_velocity"], g["init_ypr"])
    _, ref_acc, ref_done = oracle.drone_run(p, ref, acts.astype(np.float64), wind=g["wind"])
    s = lane_model.initial_state(p, n, g["init_position"], g["init_velocity"], g["init_ypr"])
    _, acc, done, rew = lane_model.run(p, s, acts, wind=g["wind"])
    return s, ref, acc, ref_acc, done, ref_done, rew, n


@pytest.mark.parametrize("name", ["g2_sin_4096", "g3_ema_noise", "g4_saturated", "g5_attitude_wind"])
def test_fp32_within_1e5_after_1000_steps(params_1k, name):
    s, ref, acc, ref_acc, done, ref_done, rew, n = _both(params_1k, load_golden(name))
    err = soa_vs_oracle(s, ref, n)
    assert_parity(err, REL_TOL, name)
    assert np.array_equal(done, ref_done)
    np.testing.assert_allclose(acc[:, :n].T, ref_acc, rtol=1e-4, atol=1e-4)   # third return value, R_new @ acc (an output: fp32 cancellation of ~100 m/s^2 terms)
    goal = params_1k.goal
    np.testing.assert_allclose(rew, -np.linalg.norm(ref[:, 0:3] - goal, axis=1), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("k", range(4))
def test_other_drone_types_fp32_within_1e5(k):
    """The kernel's fp32 arithmetic on the four other drone types of capture G14 (fps 120-2000, gravity 1.62-9.81,
    max_rates 90-1200 deg/s - type 3 takes 20 degrees per step, the range-reduced sin/cos path), against the oracle
    AND directly against what the reference produced."""
    g = load_golden(f"g14_drone_type_{k}")
    p = params_for_golden(g)
    s, ref, acc, ref_acc, done, ref_done, rew, n = _both(p, g)
    assert_parity(soa_vs_oracle(s, ref, n), REL_TOL, f"g14 type {k}")
    ref_direct = np.concatenate([g["state"][:, -1], g["R"][:, -1].reshape(n, 9), g["prev_rates"][:, -1],
                                 g["prev_thrust"][:, -1:]], axis=1)
    assert_parity(soa_vs_oracle(s, ref_direct, n), REL_TOL, f"g14 type {k} (reference capture)")
    assert np.array_equal(done, ref_done) and np.array_equal(done, g["done"][:, -1])


def test_fps60_large_step_angles(params_60):
    """dt = 1/60: 200 deg/s * dt = 3.3 deg per application - the short sin/cos polynomial still holds."""
    s, ref, *_rest, n = _both(params_60, load_golden("g1b_fps60_sin"))
    assert_parity(soa_vs_oracle(s, ref, n), REL_TOL, "fps60")


def test_config1_10k_steps_fp32_drift(params_1k):
    """Config 1 (10 000 zero-stick steps, climbing to z ~ 206 m): plain fp32 accumulation is NOT
    expected to hold 1e-5 (0.02 m increments against 200 m); document what it does hold."""
    s, ref, *_rest, n = _both(params_1k, load_golden("g1_zero_10k"))
    err = soa_vs_oracle(s, ref, n)
    assert err["pos_rel"] < 2e-4 and err["quat_abs"] < 1e-6, err
    s1k, ref1k, *_r, n = _both(params_1k, load_golden("g1_zero_10k"), steps=1000)
    assert_parity(soa_vs_oracle(s1k, ref1k, n), REL_TOL, "config1 first 1000 steps")


def test_ground_flag_sequence(params_1k):
    g = load_golden("g6_ground")
    acts = g["actions"]
    T, n = acts.shape[:2]
    s = lane_model.initial_state(params_1k, n, g["init_position"], g["init_velocity"], g["init_ypr"])
    seq = np.zeros((n, T), dtype=np.uint8)
    for t in range(T):
        _, _, done, _ = lane_model.run(params_1k, s, acts[t:t + 1], wind=g["wind"])
        seq[:, t] = done
    assert np.array_equal(seq, g["done"]), "the fp32 done flag must flip on exactly the reference's steps"


def test_big_angle_path_matches_small(params_1k):
    """max_rates large enough that the derive step selects library sincos: same trajectory."""
    g = load_golden("g3_ema_noise")
    n = g["actions"].shape[1]
    p_big = params_1k.replace(max_rates=2.0e5, dt=1e-3)          # half-angle bound 1.75 rad > pi/4
    acts = (g["actions"] * np.float32(1e-3)).astype(np.float32)   # same physical rates as max_rates=200
    acts[..., 3] = g["actions"][..., 3]
    s_big = lane_model.initial_state(p_big, n)
    lane_model.run(p_big, s_big, acts)
    ref = oracle.drone_initial_state(n, p_big.init_position, p_big.init_velocity, [0, 0, 0])
    oracle.drone_run(p_big, ref, acts.astype(np.float64))
    assert_parity(soa_vs_oracle(s_big, ref, n), 2e-5, "big-angle")


def test_auto_reset_and_ceiling(params_1k):
    p = params_1k.replace(ceiling=10.5)
    n = 4
    s = lane_model.initial_state(p, n)
    acts = np.zeros((n, 4), dtype=np.float32)
    acts[:, 3] = [1.0, 0.0, -1.0, 0.3]      # climbers hit the ceiling, the faller hits the ground later
    hit = np.zeros(n, dtype=bool)
    for t in range(400):
        _, _, done, _ = lane_model.run(p, s, acts, steps=1, auto_reset=True)
        for i in np.flatnonzero(done):
            hit[i] = True
            np.testing.assert_array_equal(s[0:3, i], p.init_position.astype(np.float32))
            np.testing.assert_array_equal(s[10:14, i], 0)
    assert hit[0] and hit[1], "full/half throttle must cross |z| > ceiling within 400 ms"
    assert np.all(np.abs(s[2, :n]) <= 10.5 + 0.1)


def _racer_trajectory_errors(p, g, rows=29):
    """Replay a Racer golden on the lane model, comparing at EVERY snapshot (not only the last)."""
    s = lane_model.initial_state(p, 1)
    assert s.shape[0] == rows
    prev, worst = 0, dict(quat=0.0, pos=0.0, omega=0.0)
    for k, t in enumerate(np.asarray(g["snap_steps"]).reshape(-1)):
        lane_model.run(p, s, g["actions"][prev:int(t)])
        prev = int(t)
        q = s[6:10, 0].astype(np.float64)
        x, y, z, w = g["quat_xyzw"][0, k]
        qr = np.array([w, x, y, z])
        q *= np.sign(q @ qr)
        pr = g["position"][0, k]
        worst["quat"] = max(worst["quat"], np.abs(q - qr).max())
        worst["pos"] = max(worst["pos"], np.abs(s[0:3, 0] - pr).max() / max(np.abs(pr).max(), 1e-3))
        worst["omega"] = max(worst["omega"], np.abs(s[10:13, 0].astype(np.float64) + s[20:23, 0] - g["omega"][0, k]).max())
    return worst


@pytest.mark.parametrize("name", ["g7_racer_main", "g8_racer_pid_thrust", "g15_racer_prop7"])
def test_racer_as_written_within_1e5_over_the_whole_trajectory(params_1k, name):
    """Racer.step as written rotates by omega [rad] per STEP (quirk Q7, racer_drone_test.py:99): the rate
    loop, omega and the attitude increment are therefore carried in float64 with fp32 (hi, lo) state rows
    (fpv_racer_step_lane<WIDE>).  Against the reference captures G7/G8 this holds the north-star bar
    1e-5 at every snapshot of the 1000 steps (measured 7e-7); plain fp32 held only 2e-3."""
    g = load_golden(name)
    worst = _racer_trajectory_errors(racer_params_for_golden(g), g)
    assert worst["quat"] < REL_TOL and worst["pos"] < REL_TOL and worst["omega"] < 1e-8, worst


def test_racer_with_components_pid_fp32_state(params_1k):
    """racer_pid_variant = 1 (components.PID.__call__, a16) inside the as-written Racer, vs capture G12."""
    from test_oracle_golden import _cpid_params
    g = load_golden("g12_racer_components_pid")
    worst = _racer_trajectory_errors(_cpid_params(params_1k, g), g)
    assert worst["quat"] < REL_TOL and worst["pos"] < REL_TOL, worst


def test_components_pid_fp32_arithmetic():
    """The kernel's fp32 PID (fpv_pid_axis<float, 1>) against the reference class outputs of G11.  The
    derivative term divides an fp32 error difference by dt = 1e-3, so an output carries up to
    |kD| * 1e3 * ulp(error) of rounding: 2e-5 absolute covers every case of the fixture."""
    g = load_golden("g11_components_pid")
    for c in range(g["gains"].shape[0]):
        out, st = lane_model.pid_run(g["gains"][c], g["current"][c], g["target"][c])
        np.testing.assert_allclose(out, g["out"][c], rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(st[0], g["integral"][c][-1], rtol=1e-5, atol=1e-7)
        assert st[3] == 0.0


def test_sincos_wide_matches_libm_to_1e15():
    import ctypes as C
    L = lane_model.lib()
    L.fpvl_sincos_wide.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-1e3, 1e3, 4000), rng.uniform(-1e6, 1e6, 2000), [0.0, -15.0, 40.0, 25.0, 1e-9, np.pi / 4, -np.pi / 2]])
    s, c = C.c_double(), C.c_double()
    worst = 0.0
    for x in xs:
        L.fpvl_sincos_wide(float(x), C.byref(s), C.byref(c))
        worst = max(worst, abs(s.value - np.sin(x)), abs(c.value - np.cos(x)))
    assert worst < 2e-15, worst


def test_racer_omega_dt_variant_is_well_conditioned(params_1k):
    g = load_golden("g8_racer_pid_thrust")
    p = params_1k.replace(mode=1, racer_pid=g["pid"], racer_omega_dt=True)
    acts = g["actions"]
    s = lane_model.initial_state(p, 1)
    lane_model.run(p, s, acts)
    ref = oracle.racer_initial_state(1)
    oracle.racer_run(p, ref, acts.astype(np.float64))
    qx, qy, qz, qw = ref[0, 6:10]
    q32 = s[6:10, 0].astype(np.float64)
    q32 *= np.sign(q32 @ np.array([qw, qx, qy, qz]))
    assert np.abs(q32 - [qw, qx, qy, qz]).max() < 1e-5
    np.testing.assert_allclose(s[0:3, 0], ref[0, 0:3], rtol=1e-5, atol=1e-6)


def test_ground_contact_fp32(params_1k):
    g = load_golden("g9_ground_contact")
    p = params_1k.replace(ground=True)
    acts = g["actions"]
    T, n = acts.shape[:2]
    s = lane_model.initial_state(p, n, g["init_position"], g["init_velocity"], g["init_ypr"])
    seq = np.zeros((n, T), dtype=np.uint8)
    for t in range(T):
        _, _, done, _ = lane_model.run(p, s, acts[t:t + 1])
        seq[:, t] = done
    assert np.array_equal(seq, g["done"])
    ref = np.concatenate([g["state"][:, -1], g["R"][:, -1].reshape(n, 9), g["prev_rates"][:, -1],
                          g["prev_thrust"][:, -1:]], axis=1)
    err = soa_vs_oracle(s, ref, n)
    # bouncing on an undamped 100 N/m spring for 0.6 s: measured 1.2e-6 (per component, 1 m floor) - the
    # float64 oracle itself moves by 1.4e-7 under an fp32-ulp perturbation of its initial state
    assert err["pos_comp"] < REL_TOL and err["quat_abs"] < REL_TOL, err


# ---- fp16 storage (BASELINE config 4): v, q, rates, thrust in eleven 16-bit words, p and all arithmetic in fp32 ----
# Tolerance RE-STATED for this config (measured on the golden profiles and on 512 noise-stick drones, then given 2-3x
# margin).  Round 3 stored eleven binary16 values: measured |dp|/|p| 8e-3, |dq| 6e-3, |dv|/|v| 1.6e-2 after 1000 steps,
# asserted 2e-2 / 1.5e-2 / 4e-2.  Round 4 spends the same 22 bytes on 15 mantissa bits for v and a smallest-three
# fixed-point quaternion (fpv_pack_half): measured 0.5-1.5e-3 / 1.0-2.1e-3 / 1.3-6.3e-3 - asserted 5x / 3x / 2.7x tighter.
FP16_TOL = dict(pos_rel=4e-3, vel_rel=1.5e-2, quat_abs=5e-3)


def test_fp16_conversions_match_ieee_and_stochastic_rounding_is_unbiased():
    L = lane_model.lib()
    lane_model.run_h(load_params_1k(), np.zeros((3, 64), np.float32), np.zeros(11 * 64, np.uint16),
                     np.zeros((1, 4), np.float32), steps=0, n=1)          # sets argtypes
    rng = np.random.default_rng(0)
    xs = rng.standard_normal(5000).astype(np.float32) * np.float32(10.0) ** rng.integers(-9, 5, 5000).astype(np.float32)
    xs = np.concatenate([xs, np.array([0, -0.0, 65504, 65519.9, 65520, 7e4, -7e4, 6e-8, 3e-8, 2.98e-8, 5.96e-8,
                                       6.1e-5, 6.09e-5, 1.0, -1.0], dtype=np.float32)])
    # every tie between two subnormal halves, (k + 1/2) 2^-24, and its two float32 neighbours, both signs: 2^-25 (1 + 2^-23) is
    # where adding 0.5f before truncating went wrong (the sum is not a float and rounds onto the tie)
    ties = ((np.arange(1024) + 0.5) * 2.0 ** -24).astype(np.float32)
    ties = np.concatenate([ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1))])
    xs = np.concatenate([xs, ties, -ties])
    with np.errstate(over="ignore"):
        ref = xs.astype(np.float16)
    for x, r in zip(xs, ref):
        h = L.fpvl_f32_to_f16(float(x), 0, 0)
        assert h == int(r.view(np.uint16)), (x, hex(h), hex(int(r.view(np.uint16))))
        back = L.fpvl_f16_to_f32(h)
        assert back == float(r) or (np.isnan(back) and np.isnan(float(r)))
    # stochastic: result is one of the two neighbours, mean over all 8192 offsets is exact to 1e-7
    for x in (1.0003, -3.14159, 19.37, 4.1e-4):
        vals = np.array([L.fpvl_f16_to_f32(L.fpvl_f32_to_f16(x, r, 1)) for r in range(8192)], dtype=np.float64)
        assert len(np.unique(vals)) <= 2 and abs(vals.mean() - np.float32(x)) < 2e-7 * max(1, abs(x))
    # exactly representable values are never perturbed
    for x in (1.0, 0.5, -2.0, 10.0, 0.0):
        assert all(L.fpvl_f16_to_f32(L.fpvl_f32_to_f16(x, r, 1)) == x for r in (0, 1, 4095, 8191))


def test_fp16_round_toward_zero_conversion_and_pair_packing():
    """Host side of v_cvt_pkrtz_f16_f32 (the stochastic rounding = 13 random bits added below the kept mantissa, then
    this conversion): truncation for normals, subnormal halves, saturation instead of overflow, against an
    independent construction from numpy.float16 (the largest half whose magnitude does not exceed |x|)."""
    rng = np.random.default_rng(1)
    xs = rng.standard_normal(6000).astype(np.float32) * np.float32(10.0) ** rng.integers(-10, 6, 6000).astype(np.float32)
    xs = np.concatenate([xs, np.array([0, -0.0, 65504, 65519.9, 65520, 65535.9, 65536, 7e4, -7e4, 3e38, 6e-8, 5.97e-8, 5.9e-8, 3e-8,
                                       6.1e-5, 6.09e-5, 6.103515625e-5, 1.0, -1.0, 1.0009765625, 1.00097, np.inf, -np.inf], dtype=np.float32)])
    got = lane_model.f32_to_f16_rtz(xs)
    with np.errstate(over="ignore"):
        rn = xs.astype(np.float16)
    # round-to-nearest result, stepped one half towards zero wherever it overshot |x|; finite overflow -> 65504
    bits = rn.view(np.uint16).copy()
    mag = bits & 0x7fff
    over = (np.abs(rn.astype(np.float64)) > np.abs(xs.astype(np.float64))) & np.isfinite(xs)
    mag = np.where(over, mag - 1, mag)
    want = ((bits & 0x8000) | mag).astype(np.uint16)
    assert np.array_equal(got, want), [(float(x), hex(g), hex(w)) for x, g, w in zip(xs, got, want) if g != w][:5]


def _words(w):
    """the eleven 16-bit storage words of one packed drone (fpvl_pack_state -> five pair words + the thrust half)"""
    return [int(w[0]) & 0xffff, int(w[0]) >> 16, int(w[1]) & 0xffff, int(w[1]) >> 16, int(w[2]) & 0xffff, int(w[2]) >> 16,
            int(w[3]) & 0xffff, int(w[3]) >> 16, int(w[4]) & 0xffff, int(w[4]) >> 16, int(w[5]) & 0xffff]


def _decode(words):
    """An INDEPENDENT float64 reading of the storage format: v = binary16 + 5-bit low word (the next five mantissa
    bits, i.e. + low * ulp(half) / 32 for a normal half), q = smallest three (15-bit two's complement / 23168, the dropped
    component positive), rates / thrust binary16."""
    h = np.array(words, dtype=np.uint16)
    f16 = h.view(np.float16).astype(np.float64)
    # magnitude grows with the low word (sign-magnitude): + for positive halves, - for negative ones
    v = [f16[k] + (-1.0 if words[k] & 0x8000 else 1.0) * ((words[3] >> (5 * k)) & 31) * (2.0 ** (((words[k] >> 10) & 31) - 25) / 32 if (words[k] >> 10) & 31 else 0.0) for k in range(3)]
    sx = lambda f: ((f & 0x7fff) ^ 0x4000) - 0x4000           # noqa: E731  sign-extend 15 bits
    a, b, c = (sx(words[4]) / 23168.0, sx(words[5]) / 23168.0, sx(words[6]) / 23168.0)
    idx = ((words[4] >> 15) & 1) | (((words[5] >> 15) & 1) << 1)
    d = np.sqrt(max(0.0, 1 - a * a - b * b - c * c))
    q = {0: (d, a, b, c), 1: (a, d, b, c), 2: (a, b, d, c), 3: (a, b, c, d)}[idx]
    return np.array(v), np.array(q), f16[7:10], f16[10], idx


def test_fp16_storage_format_one_state_through_the_packer():
    """fpv_pack_half against an independent reading of the format: v lands within one 15-bit-mantissa step of the value
    (32x finer than binary16) and visits both neighbours over the seeds (stochastic, unbiased), q comes back as the same
    ATTITUDE within the fixed-point grid with the largest component dropped and positive, rates / thrust are the nearest
    binary16, exactly representable values are never perturbed, and the host decoder (fpv_unpack_half) reads the same numbers."""
    st = np.array([1, 2, 3, 0.3337, -12.3456, 20.5457, 0.70712, -0.00123, 0.70709, 1e-6, -159.99, 3.3333, 0.01, 31.5085], dtype=np.float32)
    st[6:10] /= np.linalg.norm(st[6:10].astype(np.float64))
    seen = [set(), set(), set()]
    vsum, qsum = np.zeros(3), np.zeros(4)
    for seed in range(400):
        w = lane_model.pack_state(st, seed, 5)
        v, q, rates, thrust, idx = _decode(_words(w))
        assert np.array_equal(rates, st[10:13].astype(np.float16).astype(np.float64)) and thrust == float(np.float16(st[13])), "rates / thrust: round to nearest even"
        step = np.abs(np.spacing(st[3:6].astype(np.float16)).astype(np.float64)) / 32            # 15 mantissa bits
        assert np.all(np.abs(v - st[3:6]) <= step * 1.0001), (v, st[3:6])
        assert idx == 0 and q[0] > 0, "w = 0.70712 is the largest component: dropped, positive"
        assert np.abs(q - st[6:10]).max() <= 1.0 / 23168 * 1.5
        for k in range(3):
            seen[k].add(v[k])
        vsum += v; qsum += q
    assert all(len(x) == 2 for x in seen), "over 400 seeds a value between two grid points visits both neighbours"
    assert np.abs(vsum / 400 - st[3:6]).max() < 3e-5 * 20 and np.abs(qsum / 400 - st[6:10]).max() < 1.2e-5, "unbiased"
    # the dropped component follows the largest magnitude, the sign flips with it, and the host decoder agrees
    for q0, want_idx in (([0.1, -0.9, 0.3, 0.2], 1), ([0.2, 0.1, -0.95, 0.1], 2), ([-0.1, 0.2, 0.3, -0.92], 3), ([-0.99, 0.05, 0.1, 0.02], 0)):
        s2 = st.copy(); s2[6:10] = np.array(q0) / np.linalg.norm(q0)
        v, q, _, _, idx = _decode(_words(lane_model.pack_state(s2, 7, 9)))
        assert idx == want_idx and q[want_idx] > 0
        assert min(np.abs(q - s2[6:10]).max(), np.abs(q + s2[6:10]).max()) <= 1.5 / 23168
    exact = np.array([0, 0, 10, 1.5, -0.25, 0.0, 1, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    for seed in (0, 1, 77):
        v, q, _, _, idx = _decode(_words(lane_model.pack_state(exact, seed, 3)))
        assert np.array_equal(v, [1.5, -0.25, 0.0]) and np.array_equal(q, [1, 0, 0, 0]) and idx == 0
    full = np.zeros((14, 64), dtype=np.float32); full[:, 0] = st
    pos, sh = lane_model.split_half(full, seed=11, drone_id_offset=5)
    back = lane_model.join_half(pos, sh)[:, 0]
    v, q, rates, thrust, _ = _decode(_words(lane_model.pack_state(st, 11, 5)))
    assert np.allclose(back[3:6], v, rtol=0, atol=1e-12) and np.abs(back[6:10] - q).max() < 1e-7 and np.array_equal(back[10:13], rates)


def load_params_1k():
    from fpyv_amd import load_params
    return load_params(fps=1000)


@pytest.mark.parametrize("name", ["g2_sin_4096", "g3_ema_noise", "g5_attitude_wind"])
def test_fp16_storage_restated_tolerance(params_1k, name):
    g = load_golden(name)
    acts = g["actions"]
    n = acts.shape[1]
    ref = oracle.drone_initial_state(n, g["init_position"], g["init_velocity"], g["init_ypr"])
    oracle.drone_run(params_1k, ref, acts.astype(np.float64), wind=g["wind"])
    s = lane_model.initial_state(params_1k, n, g["init_position"], g["init_velocity"], g["init_ypr"])
    pos, sh = lane_model.split_half(s, seed=1)
    lane_model.run_h(params_1k, pos, sh, acts, wind=g["wind"], seed0=1)
    err = soa_vs_oracle(lane_model.join_half(pos, sh), ref, n)
    for k, tol in FP16_TOL.items():
        assert err[k] <= tol, (name, k, err[k])
    # and it must NOT stall: round-to-nearest storage would freeze slow rotations / small accelerations
    assert err["quat_abs"] > 1e-6, "suspiciously exact: is the fp16 path really exercised?"


def test_fp16_round_to_nearest_would_stall(params_1k):
    """Why the integrator rows are rounded stochastically: a slow roll (8 deg/s) moves q by 1.4e-4
    per step, below half an fp16 ulp near 1 - RN storage freezes it, SR follows the oracle."""
    n, T = 4, 1000
    acts = np.zeros((T, n, 4), dtype=np.float32)
    acts[..., 0] = 0.02
    ref = oracle.drone_initial_state(n, params_1k.init_position, params_1k.init_velocity, [0, 0, 0])
    oracle.drone_run(params_1k, ref, acts.astype(np.float64))
    q_ref = oracle.matrix_to_quat(ref[:, 6:15])
    s = lane_model.initial_state(params_1k, n)
    pos, sh = lane_model.split_half(s)
    lane_model.run_h(params_1k, pos, sh, acts, seed0=3)
    q = lane_model.join_half(pos, sh)[6:10, :n].T
    assert abs(q_ref[0, 1]) > 0.05, "the oracle must have rolled"
    assert np.abs(np.abs(q[:, 1]) - abs(q_ref[0, 1])).max() < 0.3 * abs(q_ref[0, 1])


def test_object_list_collisions_fp32(params_1k):
    """fp32 lane arithmetic on the G10 scenario (moving Target sphere, two Cylinders, Ground)."""
    from test_oracle_golden import _g10_objects
    g = load_golden("g10_objects")
    acts = g["actions"]
    T, n = acts.shape[:2]
    s = lane_model.initial_state(params_1k, n, g["init_position"], g["init_velocity"], g["init_ypr"])
    seq = np.zeros((n, T), dtype=np.uint8)
    try:
        for t in range(T):
            lane_model.set_objects(_g10_objects(g, t))
            _, _, done, _ = lane_model.run(params_1k, s, acts[t:t + 1])
            seq[:, t] = done
    finally:
        lane_model.set_objects(())
    first = lambda d: int(np.argmax(d)) if d.any() else -1      # noqa: E731
    for i in range(n):
        assert first(seq[i]) == first(g["done"][i]), (i, first(seq[i]), first(g["done"][i]))   # crash on the reference's step
    ok = ~g["done"].any(axis=1)                                  # compare end states of the survivors
    ref = np.concatenate([g["state"][:, -1], g["R"][:, -1].reshape(n, 9), g["prev_rates"][:, -1],
                          g["prev_thrust"][:, -1:]], axis=1)
    err = soa_vs_oracle(np.ascontiguousarray(s[:, np.flatnonzero(ok)]), ref[ok], int(ok.sum()))
    # contact episodes amplify rounding (stiff, undamped springs): measured 4.1e-6 m after 0.8 s; the float64
    # oracle itself moves by 1.7e-6 m under an fp32-ulp perturbation of its initial state
    assert err["pos_comp"] < REL_TOL and err["quat_abs"] < REL_TOL, err


def test_raised_objects_fp32(params_1k):
    """fp32 lane arithmetic on capture G16 (raised cylinders: the reference's relative-vs-absolute height test of the
    cylinder normal; Ground first; standing sphere): crashes on the reference's steps, survivors within 1e-5."""
    g = load_golden("g16_objects_raised")
    acts = g["actions"]
    T, n = acts.shape[:2]
    s = lane_model.initial_state(params_1k, n, g["init_position"], g["init_velocity"], g["init_ypr"])
    seq = np.zeros((n, T), dtype=np.uint8)
    try:
        lane_model.set_objects(tuple(tuple(o) for o in g["objects"]))
        for t in range(T):
            _, _, done, _ = lane_model.run(params_1k, s, acts[t:t + 1])
            seq[:, t] = done
    finally:
        lane_model.set_objects(())
    first = lambda d: int(np.argmax(d)) if d.any() else -1      # noqa: E731
    for i in range(n):
        assert first(seq[i]) == first(g["done"][i]), (i, first(seq[i]), first(g["done"][i]))
    ok = ~g["done"].any(axis=1)
    ref = np.concatenate([g["state"][:, -1], g["R"][:, -1].reshape(n, 9), g["prev_rates"][:, -1],
                          g["prev_thrust"][:, -1:]], axis=1)
    err = soa_vs_oracle(np.ascontiguousarray(s[:, np.flatnonzero(ok)]), ref[ok], int(ok.sum()))
    assert ok.sum() == 3 and err["pos_comp"] < REL_TOL and err["quat_abs"] < REL_TOL, err


def test_config1_10k_steps_with_kahan_compensation(params_1k):
    """The optional Kahan rows (fpv_buffers_t.pos_comp, [6][ld]: p and v) close the 10 000-step gap of
    config 1: from 1.2e-4 (plain fp32 sums) to < 1e-6 relative against the reference capture."""
    g = load_golden("g1_zero_10k")
    s = lane_model.initial_state(params_1k, 1)
    comp = np.zeros((6, s.shape[1]), dtype=np.float32)
    lane_model.set_pos_comp(comp)
    try:
        lane_model.run(params_1k, s, np.zeros((1, 4), np.float32), steps=10000)
    finally:
        lane_model.set_pos_comp(None)
    ref = np.concatenate([g["state"][:, -1], g["R"][:, -1].reshape(1, 9), g["prev_rates"][:, -1],
                          g["prev_thrust"][:, -1:]], axis=1)
    err = soa_vs_oracle(s, ref, 1)
    assert err["pos_rel"] < 1e-6 and err["vel_rel"] < 1e-6 and err["quat_abs"] < 1e-6, err


def test_config0_default_fps60_10k_steps_with_kahan_compensation(params_60):
    """BASELINE configs[0] to the letter (fps = 60, zero sticks, 10 000 steps; capture G1 @ fps 60) in the kernel's fp32
    arithmetic: 0.34 m increments into a coordinate that reaches 3.4 km.  Plain fp32 sums drift; the Kahan rows hold
    the north-star bar against the reference capture at every 100th step."""
    g = load_golden("g1_zero_10k_fps60")
    plain = lane_model.initial_state(params_60, 1)
    lane_model.run(params_60, plain, np.zeros((1, 4), np.float32), steps=10000)
    ref = np.concatenate([g["state"][:, -1], g["R"][:, -1].reshape(1, 9), g["prev_rates"][:, -1], g["prev_thrust"][:, -1:]], axis=1)
    assert 1e-6 < soa_vs_oracle(plain, ref, 1)["pos_rel"] < 1e-3, "plain fp32 accumulation: documented drift"
    s = lane_model.initial_state(params_60, 1)
    comp = np.zeros((6, s.shape[1]), dtype=np.float32)
    lane_model.set_pos_comp(comp)
    worst = 0.0
    try:
        prev = 0
        for k, t in enumerate(np.asarray(g["snap_steps"]).reshape(-1)):
            lane_model.run(params_60, s, np.zeros((1, 4), np.float32), steps=int(t) - prev)
            prev = int(t)
            ref = np.concatenate([g["state"][:, k], g["R"][:, k].reshape(1, 9), g["prev_rates"][:, k], g["prev_thrust"][:, k:k + 1]], axis=1)
            err = soa_vs_oracle(s, ref, 1)
            worst = max(worst, err["pos_rel"], err["pos_comp"], err["vel_rel"], err["quat_abs"])
    finally:
        lane_model.set_pos_comp(None)
    assert worst < 1e-6, worst


def test_object_culls_never_skip_a_contact(params_1k):
    """The collision pass skips work three times over - a list-level test (ground reach + the box around all cylinders and
    spheres), a per-object test on the drone's centre, and lazily formed contact normals.  Every one of them must be
    CONSERVATIVE: a culled drone gets exactly zero object force and no crash flag, so a cull that is too tight shows up
    as a missing force against the float64 oracle, which culls nothing.  20 000 drones placed within +-0.6 m of every
    surface and every cull boundary of a five-object world, random attitudes, one step."""
    rng = np.random.default_rng(77)
    objs = ((2, 1.5, -2.0, 3.0, 0.8, 0.0), (1, 3.0, 0.5, 0.0, 1.0, 5.0), (1, -2.0, 2.5, 1.0, 0.6, 1.5), (2, -4.0, -4.0, 0.3, 0.5, 0.0), (0, 0, 0, 0, 0, 0))
    reach = float(np.linalg.norm(params_1k.motor_xy, axis=1).max() + params_1k.motor_radius + 1e-3)
    pts = []
    for (t, x, y, z, r, h) in objs[:-1]:
        m = 4000
        d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        if t == 2:
            rad = r + rng.choice([0.0, reach], m) + rng.uniform(-0.6, 0.6, m)
            pts.append(np.array([x, y, z]) + d * rad[:, None])
        else:
            ang = rng.uniform(0, 2 * np.pi, m)
            rad = r + rng.choice([0.0, reach], m) + rng.uniform(-0.6, 0.6, m)
            zz = np.where(rng.random(m) < 0.5, rng.uniform(z - reach - 0.6, z + h + reach + 0.6, m),
                          rng.choice([z, z + h], m) + rng.choice([0.0, -reach, reach], m) + rng.uniform(-0.3, 0.3, m))
            rad = np.where(rng.random(m) < 0.3, rng.uniform(0, r + reach + 0.6, m), rad)        # also above / below the caps
            pts.append(np.stack([x + rad * np.cos(ang), y + rad * np.sin(ang), zz], axis=1))
    g = np.stack([rng.uniform(-6, 6, 4000), rng.uniform(-6, 6, 4000), rng.choice([0.0, reach], 4000) + rng.uniform(-0.3, 0.3, 4000)], axis=1)
    pos = np.concatenate(pts + [g]).astype(np.float32)
    n = len(pos)
    ypr = rng.uniform([-180, -80, -180], [180, 80, 180], (n, 3))
    vel = rng.normal(size=(n, 3)) * 3
    p = params_1k.replace(objects=objs)
    act = np.zeros((1, n, 4), dtype=np.float32)
    ref = oracle.drone_initial_state(n, pos.astype(np.float64), vel, ypr)
    s = lane_model.initial_state(params_1k, n, pos, vel, ypr)
    v0 = ref[:, 3:6].copy()
    _, _, ref_done = oracle.drone_run(p, ref, act.astype(np.float64))
    try:
        lane_model.set_objects(objs)
        _, _, done, _ = lane_model.run(params_1k, s, act)
    finally:
        lane_model.set_objects(())
    # a flag may legitimately differ only where a float64 distance is within fp32 rounding of zero
    differ = np.flatnonzero(done != ref_done)
    assert len(differ) <= 5, len(differ)
    # the velocity change of one step IS the acceleration (incl. the spring forces): a skipped contact is off by ~k d / m dt
    dv, dv_ref = s[3:6, :n].T - v0.astype(np.float32), ref[:, 3:6] - v0
    keep = np.setdiff1d(np.arange(n), differ)
    assert np.abs(dv[keep] - dv_ref[keep]).max() < 2e-5, np.abs(dv[keep] - dv_ref[keep]).max()
    # the scenario is what it claims: many drones feel a spring, many crash, many do neither
    free = oracle.drone_initial_state(n, pos.astype(np.float64), vel, ypr)
    oracle.drone_run(params_1k, free, act.astype(np.float64))
    springs = np.linalg.norm(ref[:, 3:6] - free[:, 3:6], axis=1) > 1e-6
    assert springs.sum() > 500 and ref_done.sum() > 500 and (~ref_done.astype(bool) & ~springs).sum() > 500, (springs.sum(), ref_done.sum())


def test_guidance_override_fp32(params_1k):
    """The kernel's fp32 arithmetic for Drone.step(..., rotation_matrix=, thrust_force=) (matrix -> quaternion by
    Shepperd's method, then the usual step) against the reference capture G13, every step of every case."""
    from parity import soa_vs_oracle
    g = load_golden("g13_guidance_override")
    acts = g["actions"]
    T, n = acts.shape[:2]
    worst = {}
    for cases, objs in (([0, 1], ()), ([2], [(0, 0, 0, 0, 0, 0)])):
        m = len(cases)
        model = lane_model.initial_state(params_1k, m, g["init_position"][cases], g["init_velocity"][cases], g["init_ypr"][cases])
        lane_model.set_objects(objs)
        try:
            for t in range(T):
                lane_model.set_override(g["rotation_override"][t, cases], g["thrust_force"][t, cases])
                _, _, done, _ = lane_model.run(params_1k, model, acts[t:t + 1, cases])
                assert np.array_equal(done, g["done"][cases, t])
                if (t + 1) % 50 == 0:
                    ref = np.concatenate([g["state"][cases, t], g["R"][cases, t].reshape(m, 9), g["prev_rates"][cases, t],
                                          g["prev_thrust"][cases, t][:, None]], axis=1)
                    err = soa_vs_oracle(model, ref, m)
                    for k, v in err.items():
                        worst[k] = max(worst.get(k, 0.0), v)
        finally:
            lane_model.set_override(None)
            lane_model.set_objects(())
    assert worst["pos_comp"] < 1e-5 and worst["quat_abs"] < 1e-5 and worst["qnorm"] < 5e-7, worst


def test_reset_attitude_fp32_against_float64():
    """fpv_quat_from_rpy_deg (the reset kernel's per-drone ypr -> quaternion, range-reduced fp32 sin/cos) against the
    float64 host formula, over +-720 degrees: 5e-7 absolute (the fp32 half angle itself carries 2.4e-7 at 6.3 rad), unit norm."""
    from fpyv_amd.params import ypr_to_quat
    rng = np.random.default_rng(3)
    ang = np.concatenate([rng.uniform(-720, 720, (500, 3)), [[0, 0, 0], [180, 0, 0], [0, 90, 0], [0, -90, 0], [0, 0, 360], [45, 45, 45]]])
    worst = 0.0
    for a in ang:
        q32 = lane_model.quat_from_rpy_deg(*a).astype(np.float64)
        q64 = ypr_to_quat(*np.float32(a).astype(np.float64))
        worst = max(worst, np.abs(q32 - q64).max())
        assert abs(np.linalg.norm(q32) - 1) < 3e-7
    assert worst < 5e-7, worst


def test_quat_from_rot_every_branch():
    """fpv_quat_from_rot (the override's matrix -> quaternion step): random attitudes plus half-turns about
    x, y, z and near them (trace <= 0: the three diagonal branches) reproduce R(q) = R to fp32 rounding."""
    rng = np.random.default_rng(42)
    q = rng.standard_normal((400, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for ax in range(3):                                     # half-turns and their neighbourhood: w ~ 0
        for eps in (0.0, 1e-4, -3e-3, 0.05):
            v = np.zeros(4); v[0] = eps; v[1 + ax] = 1.0; v[1 + (ax + 1) % 3] = 0.3 * eps
            q = np.vstack([q, v / np.linalg.norm(v)])
    R = oracle.quat_to_matrix(q)
    got = lane_model.quat_from_rot(R).astype(np.float64)
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 2e-7
    assert np.abs(oracle.quat_to_matrix(got) - R).max() < 1e-6
    sign = np.sign(np.sum(got * q, axis=1, keepdims=True))
    assert np.abs(got * sign - q).max() < 5e-7


def test_square_frame_ground_flag_shortcut_is_exact(params_1k):
    """The X-frame shortcut of the ground flag (two heights, `pz < max(|hA|, |hB|)`) against the four-height
    evaluation it replaces: identical `done` and identical state bits on random attitudes with the centre placed
    within fp32 rounding of the flip height, and over a crash / recover trajectory."""
    from fpyv_amd import _lib as abi, sticks
    rng = np.random.default_rng(7)
    n = 4096
    ypr = rng.uniform([-180, -89, -180], [180, 89, 180], (n, 3))
    s0 = lane_model.initial_state(params_1k, n, [0, 0, 0.05], [0.5, -0.2, -0.3], ypr)
    # put every drone's centre exactly at, one ulp above and one ulp below the height at which its lowest motor
    # touches z = 0: c * (|r20| + |r21|) with R from the quaternion
    q = s0[abi.QW:abi.QZ + 1, :n].astype(np.float64)
    r20, r21 = 2 * (q[1] * q[3] - q[0] * q[2]), 2 * (q[2] * q[3] + q[0] * q[1])
    c = float(np.float32(params_1k.motor_xy[0][0]))
    flip = (abs(c) * (np.abs(r20) + np.abs(r21))).astype(np.float32)
    flip = np.where(np.arange(n) % 3 == 0, flip, np.where(np.arange(n) % 3 == 1, np.nextafter(flip, np.float32(10)), np.nextafter(flip, np.float32(-10))))
    s0[abi.PZ, :n] = flip
    acts = sticks.ema_noise(40, range(n), seed=3)
    outs = []
    for general in (False, True):
        s = s0.copy()
        lane_model.set_general_motors(general)
        try:
            dones = []
            for t in range(acts.shape[0]):
                _, _, d, _ = lane_model.run(params_1k, s, acts[t:t + 1])
                dones.append(d.copy())
        finally:
            lane_model.set_general_motors(False)
        outs.append((s, np.stack(dones)))
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert 0.2 < outs[0][1][0].mean() < 0.8, "the first step must sit on the flip boundary"


@pytest.mark.parametrize("seed", range(6))
def test_random_drone_types_within_1e5(params_1k, seed):
    """The 1e-5 bar on position / quaternion after 1000 steps for drone types far from params.yaml (mass, frame,
    thrust curve, drag, rates, low-pass constants, gravity, dt 1/250 .. 1/2000 s, random initial pose)."""
    from fpyv_amd import sticks
    from parity import assert_parity_random_type, random_drone_params
    rng = np.random.default_rng(1000 + seed)
    p = random_drone_params(params_1k, rng)
    n, steps = 333, 1000
    acts = sticks.ema_noise(steps, range(n), seed=seed)
    acts[..., 3] += np.float32(rng.uniform(-0.7, -0.3))
    ref = oracle.drone_initial_state(n, p.init_position, p.init_velocity, p.init_orientation_deg)
    oracle.drone_run(p, ref, acts.astype(np.float64))
    s = lane_model.initial_state(p, n)
    lane_model.run(p, s, acts)
    assert_parity_random_type(s, ref, n, p, REL_TOL, f"random drone type {seed} (dt {p.dt:g}, max_rates {p.max_rates:.0f})")
