"""The four functions of csrc/fpv_math.h whose device branch is NOT the code the host lane model compiles - fpv_sqrt_flushed
(v_sqrt_f32 + a two-sided correction against sqrtf), fpv_clamp (v_med3_f32 against fminf(fmaxf())), fpv_f32_to_f16_rn and
fpv_f16_to_f32 (hardware conversions against integer emulation) - on the inputs a flight never visits.  Every expected value is a
float64 restatement narrowed once (numpy.sqrt, numpy.clip, astype(numpy.float16)); the lane model is compared in addition where it
says so.  Each function is reached through the public surface, on a channel where its result leaves the kernel unmasked:

  A  square root   reward = -sqrt(|p - goal|^2) one step after a reset with zero velocity (the position does not move)
  B  clip          state rows 10..12 one step after a reset: prev_rates = 0, so the low-pass returns the clipped command itself
  C  fp16 RN       the rx, ry, rz and thrust halves of an fp16-state handle after that same step, and the widening kernel on them
"""
import dataclasses
import fractions
import functools

import numpy as np
import pytest
import torch

from fpyv_amd import _lib, objects, physics
from gpu_helpers import DEV, _drone_batch
from oracle import lane_model

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU: the stepper has no CPU path")]

f32, f64, u32 = np.float32, np.float64, np.uint32
# fpv_sqrt_flushed's documented rule (csrc/fpv_math.h): arguments below 2^-96 give 0, every other one - +inf included -
# the correctly rounded root, on the device and on the host alike
FLUSH_BELOW = f32(2.0 ** -96)
SMALLEST_NORMAL = f32(2.0 ** -126)


# ---- A: the argument of the square root, exactly known on the host ---------------------------------------------------------------
def sqrt_argument(gx, gy):
    """fl32(gx^2 + fl32(gy^2)) - what fma(gx, gx, fma(gy, gy, 0 * 0)) gives - without an fma: gy^2 is exact in float64 and narrowed
    once; for gy = 0 or |gx| / 4 <= |gy| <= |gx| the sum has at most 49 significant bits, so float64 holds it exactly and the
    last narrowing is the kernel's one rounding."""
    with np.errstate(over="ignore", under="ignore"):
        gy2 = (gy.astype(f64) * gy.astype(f64)).astype(f32)
        return (gx.astype(f64) * gx.astype(f64) + gy2.astype(f64)).astype(f32)


def assert_argument_is_exact(gx, gy, x, rng, samples=2000):
    assert np.all((gy == 0) | ((np.abs(gy) >= np.abs(gx) * f32(0.25)) & (np.abs(gy) <= np.abs(gx)))), "the 49-bit argument needs gy = 0 or |gx|/4 <= |gy| <= |gx|"
    F = fractions.Fraction
    for i in rng.choice(len(gx), samples, replace=False):
        a, b = float(gx[i]), float(gy[i])
        if not np.isfinite(x[i]):
            continue
        b2 = float(f32(b * b))
        assert F(b * b) == F(b) * F(b), "gy^2 must be exact in float64"
        s = a * a + b2
        assert F(s) == F(a) * F(a) + F(b2), ("gx^2 + fl32(gy^2) must be exact in float64", a, b)
        assert f32(s) == x[i]


@functools.lru_cache(maxsize=None)
def sqrt_sweep():
    """The lanes of the sweep as a dict of arrays: gx, gy (float32), block (0 binade draws, 1 near powers of two, 2 below the smallest
    normal and zero, 3 overflow), rank (position inside the lane's binade row, block 0)."""
    rng = np.random.default_rng(20261)
    per = 2048 + 16
    e = np.repeat(np.arange(-126, 128), per).astype(f64)
    target = np.ldexp(1.0 + rng.random(e.size), e.astype(np.int64))
    rank = np.tile(np.arange(per), 254)
    sub = np.ldexp(1.0 + rng.random(4096), rng.integers(-156, -126, 4096))            # the block below the smallest normal
    target = np.concatenate([target, sub])
    rho = np.where(rng.random(target.size) < 1 / 16, 0.0, rng.uniform(0.26, 0.99, target.size))   # gy = 0: exact squares
    gx = np.sqrt(target / (1.0 + rho * rho)).astype(f32)
    gy = (rho * gx.astype(f64)).astype(f32)
    gx *= rng.choice(f32([-1, 1]), gx.size)
    gy *= rng.choice(f32([-1, 1]), gy.size)
    block = np.concatenate([np.zeros(e.size, np.int8), np.full(sub.size, 2, np.int8)])
    rank = np.concatenate([rank, np.arange(sub.size)])
    # arguments within a few ulp of 4^j (gy = 0) and of 2 * 4^j (gy = gx): gx = 2^j (1 + i ulp), both sides of the power
    j = np.repeat(np.arange(-63, 64), 9)
    i = np.tile(np.arange(-4, 5), 127)
    near = np.ldexp(np.where(i < 0, 1.0 + i * 2.0 ** -24, 1.0 + i * 2.0 ** -23), j).astype(f32)
    sgn = np.where(np.arange(near.size) % 2 == 0, f32(1), f32(-1))
    gx = np.concatenate([gx, near * sgn, near * sgn])
    gy = np.concatenate([gy, np.zeros_like(near), near])
    block = np.concatenate([block, np.ones(2 * near.size, np.int8)])
    rank = np.concatenate([rank, np.arange(2 * near.size)])
    # +0 in every sign combination, and arguments that overflow to +inf
    zx, zy = f32([0.0, -0.0, 0.0, -0.0] * 4), f32([0.0, 0.0, -0.0, -0.0] * 4)
    ox, oy = f32([1e20, -1e20, 1e20, -1e20, 1e20, 3e19]), f32([0, 0, 5e19, -5e19, -1e20, 0])
    gx, gy = np.concatenate([gx, zx, ox]), np.concatenate([gy, zy, oy])
    block = np.concatenate([block, np.full(zx.size, 2, np.int8), np.full(ox.size, 3, np.int8)])
    rank = np.concatenate([rank, np.arange(zx.size), np.arange(ox.size)])
    return dict(gx=gx, gy=gy, block=block, rank=rank)


def binade(x):
    """floor(log2 x) of a float32 array; -127 stands for everything below the smallest normal, zero included"""
    return (x.view(u32) >> 23 & 0xff).astype(np.int64) - 127


def near_midpoint(x):
    """True where the exact root of x lies within 2^-6 ulp of the midpoint between two floats: float64's root carries 29 bits below
    the float32 ulp, which settles a 2^-6 window."""
    with np.errstate(invalid="ignore"):
        m, _ = np.frexp(np.sqrt(x.astype(f64)))
        frac = m * 2.0 ** 24 % 1.0
    return np.isfinite(x) & (x >= SMALLEST_NORMAL) & (np.abs(frac - 0.5) < 2.0 ** -6)


def classify(x):
    """the classes of the realised arguments whose minimum counts the tests assert"""
    mant = x.view(u32) & 0x7fffff
    pow2 = np.isfinite(x) & (x >= SMALLEST_NORMAL) & ((mant <= 8) | (mant >= 0x7ffff8))
    even = binade(x) % 2 == 0
    return dict(mid=near_midpoint(x), near_4k=pow2 & (even ^ (mant >= 0x7ffff8)), near_2_4k=pow2 & ~(even ^ (mant >= 0x7ffff8)))


def assert_coverage(gx, gy, x, per_binade):
    """Conditions on the inputs, met on the host before anything is launched."""
    b, c = binade(x), classify(x)
    normal = np.isfinite(x) & (x >= SMALLEST_NORMAL)
    counts = np.bincount(b[normal] + 126, minlength=254)
    assert counts.min() >= per_binade, ("mantissas per binade", int(counts.argmin()) - 126, int(counts.min()))
    assert np.count_nonzero((x > 0) & (x < SMALLEST_NORMAL)) >= 512 and np.count_nonzero(x == 0) >= 4 and np.count_nonzero(np.isinf(x)) >= 4
    for sx in (False, True):
        for sy in (False, True):
            assert np.count_nonzero((np.signbit(gx) == sx) & (np.signbit(gy) == sy) & (gy != 0)) >= 1000, "both signs of gx and gy"
    squares = normal & (gy == 0)
    assert np.count_nonzero(squares) >= 1000
    assert np.count_nonzero(c["near_4k"]) >= 256 and np.count_nonzero(c["near_2_4k"]) >= 256
    assert np.count_nonzero(c["mid"]) >= 256
    for lo, hi in ((-126, -110), (-96, -80)):            # the bottom of the normal range, and the bottom of what is not flushed
        assert np.count_nonzero(c["mid"] & (b >= lo) & (b < hi)) >= 64, (lo, hi)
    return squares


def expected_reward_bits(x, minus_zero=True):
    """-float32(sqrt(float64(x))), the flushed arguments giving zero; float64's root narrowed to 24 bits is the correctly rounded
    float32 root (53 >= 2 * 24 + 2: no double rounding).  minus_zero=False is the gate reward's form 0 - root."""
    with np.errstate(invalid="ignore"):
        root = np.sqrt(x.astype(f64))
    root = np.where(x < FLUSH_BELOW, 0.0, root)
    return ((-root) if minus_zero else (0.0 - root)).astype(f32).view(u32)


def assert_rewards(tag, x, got, want):
    got = np.ascontiguousarray(got).view(u32)
    bad = got != want
    if bad.any():
        b = binade(x)
        per = {int(k): int(v) for k, v in zip(*np.unique(b[bad], return_counts=True))}
        first = [(hex(int(x.view(u32)[i])), hex(int(got[i])), hex(int(want[i]))) for i in np.flatnonzero(bad)[:5]]
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} rewards differ from -float32(sqrt(float64(x))); mismatches per binade of x "
                             f"(-127: below the smallest normal) {per}; first (x, got, want): {first}")


def sqrt_lanes(full):
    """(gx, gy) of the full sweep, or of the reduced one: 256 mantissas per binade, every lane of the other blocks, and every
    binade lane whose root sits near a rounding boundary at the bottom of the normal range or of the unflushed range."""
    s = sqrt_sweep()
    gx, gy = s["gx"], s["gy"]
    if full:
        return gx, gy
    x = sqrt_argument(gx, gy)
    b = binade(x)
    low = near_midpoint(x) & (((b >= -126) & (b < -110)) | ((b >= -96) & (b < -80)))
    keep = (s["block"] != 0) | (s["rank"] < 256 + 16) | low
    return gx[keep], gy[keep]


def _zeros(n, cols=4):
    return torch.zeros((n, cols), dtype=torch.float32, device=DEV)


def _pos(gx, gy):
    return np.stack([gx, gy, np.zeros_like(gx)], axis=1)


def _reward_after_one_step(env, gx, gy, **step_kw):
    n = gx.size
    env.reset(position=_pos(gx, gy), velocity=np.zeros((n, 3), f32))
    env.step(_zeros(n), return_imu=False, **step_kw)
    torch.cuda.synchronize()
    return env.reward.cpu().numpy()


def _sqrt_case(params_1k, full):
    p = dataclasses.replace(params_1k, goal=(0.0, 0.0, 0.0))
    gx, gy = sqrt_lanes(full)
    x = sqrt_argument(gx, gy)
    assert gx.size <= 1 << 20
    squares = assert_coverage(gx, gy, x, 2048 if full else 256)
    assert_argument_is_exact(gx, gy, x, np.random.default_rng(5))
    want = expected_reward_bits(x)
    keep = squares & (x >= FLUSH_BELOW)
    assert np.array_equal(want[keep], (-np.abs(gx[keep])).view(u32)), "sqrt(fl(gx^2)) = |gx|: the reference itself"
    return p, gx, gy, x, want


def test_sqrt_plain_single_step_full_sweep(params_1k):
    """fpv_drone_step_kernel: every binade of the argument from 2^-126 to 2^127 with 2048 mantissas, the block below the smallest
    normal, +0, +inf, exact squares, neighbours of 4^k and 2 * 4^k, roots near a rounding boundary - bitwise -float32(sqrt(float64(x)))
    for x >= 2^-96 and -0.0 below (fpv_sqrt_flushed's documented rule)."""
    p, gx, gy, x, want = _sqrt_case(params_1k, True)
    got = _reward_after_one_step(_drone_batch(p, gx.size, with_accel=False), gx, gy)
    assert_rewards("plain single step", x, got, want)


@pytest.mark.parametrize("k", [1, 3])
def test_sqrt_kstep_rollout_rewards_of_every_step(params_1k, k):
    """fpv_drone_rollout_kernel with per-step rewards: step 0 against the float64 root; from step 1 on gravity has moved pz and the
    argument is an ordinary number (about 1e-10 and up) that the host does not know without an fma - those rows are held to the
    lane model bit for bit."""
    p, gx, gy, x, want = _sqrt_case(params_1k, False)
    n = gx.size
    env = _drone_batch(p, n, with_accel=False)
    env.reset(position=_pos(gx, gy), velocity=np.zeros((n, 3), f32))
    rewards = torch.zeros((k, n), dtype=torch.float32, device=DEV)
    env.rollout(torch.zeros((k, n, 4), dtype=torch.float32, device=DEV), rewards=rewards)
    torch.cuda.synchronize()
    got = rewards.cpu().numpy()
    assert_rewards(f"k-step rollout, k = {k}, step 0", x, got[0], want)
    model = lane_model.initial_state(p, n, position=_pos(gx, gy), velocity=np.zeros((n, 3), f32))
    acts = np.zeros((1, n, 4), f32)
    for t in range(k):
        rew = lane_model.run(p, model, acts)[3]
        assert np.array_equal(got[t].view(u32), rew.view(u32)), f"step {t}: kernel != lane model"


@pytest.mark.parametrize("family", ["objects", "physics", "fp16", "racer"])
def test_sqrt_other_kernel_families(params_1k, family):
    """The reduced sweep through the other kernels that instantiate fpv_sqrt_flushed for their reward: a step with an object list,
    a per-drone-physics table handle, an fp16-state handle (the position stays fp32) and the Racer, whose reward is its own call."""
    p, gx, gy, x, want = _sqrt_case(params_1k, False)
    n = gx.size
    if family == "objects":
        got = _reward_after_one_step(_drone_batch(p, n, with_accel=False), gx, gy, object_list=[objects.Cylinder((5.0, 5.0, 0.0), 1.0, 2.0)])
    elif family == "physics":
        got = _reward_after_one_step(_drone_batch(p, n, with_accel=False, per_drone_physics=True), gx, gy)
    elif family == "fp16":
        got = _reward_after_one_step(_drone_batch(p, n, with_accel=False, fp16_state=True), gx, gy)
    else:
        from fpyv_amd.env import RacerBatch
        env = RacerBatch(p, n, device=DEV)
        env.reset()                                         # the Racer resets to its zero state: the positions go into the rows
        env.state[_lib.PX, :n] = torch.from_numpy(gx).to(DEV)
        env.state[_lib.PY, :n] = torch.from_numpy(gy).to(DEV)
        env.step(_zeros(n))                                 # no force, no velocity: the position stays
        torch.cuda.synchronize()
        got = env.reward.cpu().numpy()
    assert_rewards(family, x, got, want)


def test_sqrt_gate_handle(params_1k):
    """A gate handle replaces the reward by progress * (d0 - d1) + events, d0 and d1 the distances to the gate's centre before and
    after the step.  The drone starts ON the centre (d0 = sqrt(+0) = 0, nothing crossed) with a per-drone velocity, so that
    e = p' - c = fl(v dt) and the reward is 0 - sqrt(fl(ex^2 + fl(ey^2))): the sweep's (gx, gy) are realised as e on the host."""
    p = dataclasses.replace(params_1k, goal=(0.0, 0.0, 0.0))
    gx0, gy0 = sqrt_lanes(False)
    dt = f64(f32(p.dt))                                     # K.dt
    with np.errstate(over="ignore", under="ignore"):
        vx, vy = (gx0.astype(f64) / dt).astype(f32), (gy0.astype(f64) / dt).astype(f32)
        gx, gy = (vx.astype(f64) * dt).astype(f32), (vy.astype(f64) * dt).astype(f32)       # fma(v, dt, 0): one rounding
    x = sqrt_argument(gx, gy)
    n = gx.size
    assert_coverage(gx, gy, x, 256)
    assert_argument_is_exact(gx, gy, x, np.random.default_rng(6))
    env = _drone_batch(p, n, with_accel=False, gates=[objects.Gate((0.0, 0.0, 0.0), np.eye(3), 1.0)],
                       gate_rewards=dict(progress=1.0, crash=0.0))
    env.reset(position=np.zeros((n, 3), f32), velocity=np.stack([vx, vy, np.zeros_like(vx)], axis=1))
    env.step(_zeros(n), return_imu=False)
    torch.cuda.synchronize()
    assert not bool(env.gate_event.any()), "no drone may cross the gate's plane"
    got = env.reward.cpu().numpy()
    assert_rewards("gate handle", x, got, expected_reward_bits(x, minus_zero=False))
    # and the host build of the same gate function (fpv_gate_eval) on the realised segment 0 -> e
    from fpyv_amd import gates
    _, host, _, _ = gates.evaluate(gates.derive([objects.Gate((0.0, 0.0, 0.0), np.eye(3), 1.0)]), np.zeros((n, 3), f32), _pos(gx, gy),
                                   np.tile(f32([1, 0, 0, 0]), (n, 1)), np.zeros(n, bool), np.zeros(n, u32), gate_rewards=dict(progress=1.0, crash=0.0))
    assert np.array_equal(got.view(u32), host.view(u32)), "kernel != host gate evaluator"


# ---- B and C: sticks whose rate command lands where wanted -----------------------------------------------------------------------
def rate_constants(p):
    """(rate_lim, rate_gain, omkr, omkt) as the library narrows them (fpv_physics_derive: the function that fills FpvK)"""
    row = physics.derive(_lib.pack_params(p), None, 1)[:, 0]
    return f32(row[0]), f32(-row[0]), f32(row[1]), f32(row[2])


def rate_product(a, gain):
    """fl32(a * rate_gain): the product of two floats is exact in float64 and narrowed once"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (a.astype(f64) * f64(gain)).astype(f32)


def sticks_for_products(targets, gain):
    """For every target a stick a with fl32(a * gain) == target bit for bit, searched among the neighbours of target / gain;
    returns (sticks, targets) of the targets that have one."""
    targets = np.asarray(targets, f32)
    with np.errstate(over="ignore", under="ignore"):
        a0 = (targets.astype(f64) / f64(gain)).astype(f32)
    sign, mag = a0.view(u32) & u32(0x80000000), (a0.view(u32) & u32(0x7fffffff)).astype(np.int64)
    found, stick = np.zeros(targets.size, bool), np.zeros(targets.size, f32)
    for j in (0, -1, 1, -2, 2, -3, 3, -4, 4):
        cand = (np.clip(mag + j, 0, 0x7f7fffff).astype(u32) | sign).view(f32)
        hit = ~found & (rate_product(cand, gain).view(u32) == targets.view(u32))
        stick[hit], found = cand[hit], found | hit
    return stick[found], targets[found]


def spread_over_axes(cands, copies):
    """[n, 3] rate sticks: every candidate `copies` times on every axis, the three axes out of step with each other"""
    col = np.tile(np.asarray(cands, f32), copies)
    return np.stack([col, np.roll(col, 101), np.roll(col, 257)], axis=1)


def expected_rates(a, lim, gain, omkr):
    """state rows 10..12 after the first step as a float64 restatement: 0 * omkr + clip(fl32(a gain), -lim, lim), narrowed once"""
    prod = rate_product(a, gain).astype(f64)
    return (0.0 * f64(omkr) + np.clip(prod, -f64(lim), f64(lim))).astype(f32)


def _step_or_rollout(env, act, fused):
    a = torch.from_numpy(act).to(DEV)
    if fused:
        env.rollout(a[None].contiguous())
    else:
        env.step(a, return_imu=False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("fused", [False, True], ids=["single-step", "k-step"])
def test_clip_at_the_limits_and_on_special_products(params_1k, fused):
    """fpv_clamp through the low-passed rates: products exactly on +-rate_lim, one ulp inside and outside, +-0, denormal, +-FLT_MAX,
    +-inf and NaN, on all three axes - the float64 clip narrowed once, and the lane model, bit for bit."""
    lim, gain, omkr, _ = rate_constants(params_1k)
    inside, outside = np.nextafter(lim, f32(0)), np.nextafter(lim, f32(np.inf))
    flt_max = np.finfo(f32).max
    # +-FLT_MAX itself and the floats next to it (the products of neighbouring sticks lie about two ulp apart up there), the
    # smallest normal and the largest denormal
    top = (flt_max.view(u32) - np.arange(8, dtype=u32)).view(f32)
    targets = np.concatenate([f32([lim, -lim, inside, -inside, outside, -outside]), top, -top, f32([1.1754944e-38, -1.1754944e-38, 1.1754942e-38, -1.1754942e-38])])
    hit_sticks, hit_targets = sticks_for_products(targets, gain)
    assert set(hit_targets.view(u32).tolist()) >= set(targets[:6].view(u32).tolist()), "the limits and their neighbours must be reachable"
    direct = f32([0.0, -0.0, np.inf, -np.inf, flt_max, -flt_max, 1.0, -1.0, 5, -7, 1.0000001, -1.5, 0.5, -0.25,
                  1e-45, -1e-45, 1e-41, -1e-41, 5e-41, -7e-41, 8e-41, -3e-42])           # the last eight: denormal products
    rnd = np.random.default_rng(8).uniform(-2, 2, 64).astype(f32)
    finite = np.concatenate([hit_sticks, direct, rnd])
    act = np.zeros((finite.size * 6 + 64, 4), f32)
    act[:finite.size * 6, :3] = spread_over_axes(finite, 6)
    nan_rows = np.arange(finite.size * 6, act.shape[0])
    for k in range(3):                                      # a NaN on each axis in turn, and on all of them
        act[nan_rows[k::4], k] = np.nan
    act[nan_rows[3::4], :3] = np.nan
    act[:, 3] = np.linspace(-1, 1, act.shape[0], dtype=f32)
    n = act.shape[0]
    prod = rate_product(act[:, :3], gain)
    # conditions on the inputs
    assert np.count_nonzero(np.abs(prod) == lim) >= 32 and np.count_nonzero(np.abs(prod) == outside) >= 32 and np.count_nonzero(np.abs(prod) == inside) >= 32
    for k in range(3):
        col = prod[:, k]
        for v in (lim, -lim, inside, -inside, outside, -outside, np.inf, -np.inf):
            assert np.count_nonzero(col == v), (k, v)
        assert np.count_nonzero((col == 0) & np.signbit(col)) and np.count_nonzero((col == 0) & ~np.signbit(col))
        assert np.count_nonzero((col != 0) & (np.abs(col) < SMALLEST_NORMAL)) >= 8, "denormal products"
        assert np.count_nonzero(np.isfinite(col) & (col >= f32(2.0 ** 127))) and np.count_nonzero(np.isfinite(col) & (col <= f32(-2.0 ** 127))), "finite products at the top of the range"
        assert np.count_nonzero(np.isnan(col)) >= 16
    env = _drone_batch(params_1k, n, with_accel=False)
    env.reset()
    _step_or_rollout(env, act, fused)
    got = env.state.cpu().numpy()[10:13, :n].T
    want = expected_rates(act[:, :3], lim, gain, omkr)
    nan = np.isnan(prod)
    assert not np.isnan(want[~nan]).any()
    same = got.view(u32) == want.view(u32)
    assert same[~nan].all(), ("clip != float64 clip", act[:, :3][~nan & ~same][:5], got[~nan & ~same][:5], want[~nan & ~same][:5])
    # a NaN stick: -rate_lim, the documented answer of v_med3_f32 and of fminf(fmaxf(NaN, lo), hi) alike
    assert nan.sum() >= 48 and np.all(got[nan].view(u32) == f32(-lim).view(u32)), got[nan][:5]
    model = lane_model.initial_state(params_1k, n)
    lane_model.run(params_1k, model, act[None])
    assert np.array_equal(got.view(u32), model[10:13, :n].T.view(u32)), "kernel != lane model"


def test_fp16_round_to_nearest_and_widening_on_edge_rates(params_1k):
    """fpv_f32_to_f16_rn and fpv_f16_to_f32 (v_cvt_f16_f32 / v_cvt_f32_f16 against the host's integer emulation) through an
    fp16-state handle one step after a reset: the rx, ry, rz halves are the conversion of the clipped command c of the test above,
    the thrust half of the first low-passed thrust.  c covers subnormal halves, values below half the smallest subnormal, exact
    ties with even and odd kept mantissa (normal and subnormal halves) and zero; the stored words equal astype(float16) and the lane
    model's packing, and the widening kernel returns astype(float32) of the halves, bit for bit."""
    lim, gain, omkr, _ = rate_constants(params_1k)
    rng = np.random.default_rng(9)
    # ties of normal halves: the low 13 bits are 0x1000; kept mantissa bit (bit 13) odd and even; 2^-14 <= |c| < rate_lim
    e = rng.integers(127 - 14, 127 + 7, 600).astype(u32)
    ties = ((e << 23) | (rng.integers(0, 1 << 10, 600).astype(u32) << 13) | u32(0x1000) | (rng.integers(0, 2, 600).astype(u32) << 31)).view(f32)
    # subnormal halves: anything in [2^-25, 2^-14), and their ties (k + 1/2) 2^-24
    sub = (np.ldexp(1.0 + rng.random(300), rng.integers(-25, -14, 300)) * rng.choice([-1, 1], 300)).astype(f32)
    sub_ties = ((np.arange(0, 1024, 7) + 0.5) * 2.0 ** -24 * np.where(np.arange(0, 1024, 7) % 2, 1, -1)).astype(f32)
    # at and below half the smallest subnormal: +-2^-25 is the tie that goes to zero, its neighbours, smaller values, fp32 denormals
    tiny = f32([2.0 ** -25, -2.0 ** -25, np.nextafter(f32(2.0 ** -25), f32(1)), -np.nextafter(f32(2.0 ** -25), f32(1)),
                np.nextafter(f32(2.0 ** -25), f32(0)), 1e-9, -1e-9, 1e-30, -1e-30, 1e-40, -1e-40, 1.4e-45])
    tiny = np.concatenate([tiny, (np.ldexp(1.0 + rng.random(40), rng.integers(-40, -25, 40)) * rng.choice([-1, 1], 40)).astype(f32)])
    around = rng.uniform(-1.2, 1.2, 300).astype(f32) * f32(lim)                                  # ordinary values, some clipped
    sticks_, _ = sticks_for_products(np.concatenate([ties, sub, sub_ties, tiny, around]), gain)
    sticks_ = np.concatenate([sticks_, f32([0.0, -0.0, 1.0, -1.0])])
    act = np.zeros((sticks_.size, 4), f32)
    act[:, :3] = spread_over_axes(sticks_, 1)
    act[:, 3] = rng.uniform(-1, 1, sticks_.size).astype(f32)
    n = act.shape[0]
    c = expected_rates(act[:, :3], lim, gain, omkr)
    # conditions on the inputs
    cb = c.view(u32)
    tie = (cb & 0x1fff == 0x1000) & (np.abs(c) >= f32(2.0 ** -14)) & (np.abs(c) < f32(65504))
    assert np.count_nonzero(tie & (cb >> 13 & 1 == 1)) >= 64 and np.count_nonzero(tie & (cb >> 13 & 1 == 0)) >= 64, "exact ties, odd and even"
    assert np.count_nonzero((np.abs(c) < f32(2.0 ** -14)) & (np.abs(c) > f32(2.0 ** -25))) >= 256, "subnormal halves"
    scaled = np.abs(c.astype(f64)) * 2.0 ** 24
    assert np.count_nonzero((np.abs(c) < f32(2.0 ** -14)) & (scaled % 1.0 == 0.5)) >= 64, "ties of subnormal halves"
    assert np.count_nonzero((c != 0) & (np.abs(c) <= f32(2.0 ** -25))) >= 16 and np.count_nonzero((c < 0) & (np.abs(c) <= f32(2.0 ** -25))) >= 4
    assert np.count_nonzero(c == 0) >= 4 and np.count_nonzero(np.abs(c) == lim) >= 4
    env = _drone_batch(params_1k, n, with_accel=False, fp16_state=True, rounding_seed=77)
    env.reset()
    env.step(torch.from_numpy(act).to(DEV), return_imu=False)
    wide = env.rows_f32(10, 14)                             # fpv_widen_state
    torch.cuda.synchronize()
    words = env.storage_words().cpu().numpy().view(np.uint16)[:, :n]          # vx vy vz v_low qa qb qc rx ry rz thrust
    want_rates = c.astype(np.float16)
    assert np.array_equal(words[7:10].T, want_rates.view(np.uint16)), "rate halves != astype(float16)"
    # the same sticks through an fp32 handle of the lane model give the fp32 thrust the half is rounded from
    model = lane_model.initial_state(params_1k, n)
    lane_model.run(params_1k, model, act[None])
    assert np.array_equal(model[10:13, :n].T.view(u32), c.view(u32))
    assert np.array_equal(words[10], model[13, :n].astype(np.float16).view(np.uint16)), "thrust halves != astype(float16)"
    # the lane model's own fp16 step: every storage word
    pos, sh = lane_model.split_half(lane_model.initial_state(params_1k, n), seed=77)
    lane_model.run_h(params_1k, pos, sh, act[None], seed0=77)
    lm = pos.shape[1]
    want_words = np.concatenate([sh[:10 * lm].reshape(5, lm, 2)[:, :n].transpose(0, 2, 1).reshape(10, n), sh[10 * lm:10 * lm + n][None]])
    assert np.array_equal(words, want_words), "storage words != lane model"
    assert np.array_equal(env.state.cpu().numpy()[:, :n].view(u32), pos[:, :n].view(u32))
    # widening: the halves as float32, subnormals included
    halves = words[7:11].T.copy().view(np.float16)
    assert np.array_equal(wide.cpu().numpy().view(u32), halves.astype(f32).view(u32)), "fpv_widen_state != astype(float32)"
