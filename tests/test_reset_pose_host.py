"""Reset sources (include/fpv_abi.h "Reset sources", ABI 9) on the host - no GPU needed: fpv_reset_pose_sample runs the kernels'
own jitter function (csrc/fpv_math.h fpv_reset_jitter) and is held here against a float64 NumPy restatement of the documented
counter convention built on oracle/philox.py, against the uniform distribution, and against the parameter checks of fpv_create."""
import ctypes as C
import math

import numpy as np
import pytest

from fpyv_amd import _lib, load_params
from oracle import philox

FPV_EINVAL, FPV_EPARAM = -1, -5
POS = [[-1.5, -0.25, 2.0], [1.5, 0.75, 6.0]]
VEL = [[-0.5, -0.5, -2.0], [0.5, 1.0, 0.0]]
YPR = [[-20.0, -10.0, -180.0], [20.0, 10.0, 180.0]]
SEED = 0x0123_4567_89AB_CDEF


def _params(**kw):
    base = dict(reset_position_range=POS, reset_velocity_range=VEL, reset_ypr_range_deg=YPR, reset_seed=SEED)
    base.update(kw)
    return load_params(fps=1000, **base)


def _sample(cp, gid, step, e, base):
    L = _lib.lib()
    b = np.ascontiguousarray(base, dtype=np.float32)
    out = np.empty(10, dtype=np.float32)
    rc = L.fpv_reset_pose_sample(C.byref(cp), int(gid), int(step), int(e), b.ctypes.data, out.ctypes.data)
    return rc, out


def _samples(cp, gids, steps, es, base=None):
    base = np.array([0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32) if base is None else base
    out = np.empty((len(gids), 10), dtype=np.float32)
    for k, (g, t, e) in enumerate(zip(gids, steps, es)):
        rc, out[k] = _sample(cp, g, t, e, base)
        assert rc == 0, _lib.lib().fpv_last_error()
    return out


def _reference_u(gids, steps, es):
    """[n, 3 blocks, 3 words] uniforms of the documented counter convention, float64"""
    gids = np.asarray(gids, dtype=np.uint64)
    steps = np.asarray(steps, dtype=np.uint64)
    es = np.asarray(es, dtype=np.uint64)
    key = np.array([[SEED & 0xFFFFFFFF, SEED >> 32]] * len(gids), dtype=np.uint32)
    u = np.empty((len(gids), 3, 3))
    for b in range(3):
        ghi = (gids >> np.uint64(32)) ^ np.uint64(b << 28) ^ (es << np.uint64(31))
        ctr = np.stack([gids & np.uint64(0xFFFFFFFF), ghi & np.uint64(0xFFFFFFFF), steps & np.uint64(0xFFFFFFFF),
                        steps >> np.uint64(32)], axis=-1).astype(np.uint32)
        w = philox.philox4x32(ctr, key, rounds=7)
        u[:, b, :] = (w[:, :3] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return u


def _boxes():
    lo = np.array([POS[0], VEL[0], YPR[0]], dtype=np.float64)
    hi = np.array([POS[1], VEL[1], YPR[1]], dtype=np.float64)
    lo32 = lo.astype(np.float32).astype(np.float64)
    span32 = (hi - lo).astype(np.float32).astype(np.float64)       # span in double, then narrowed (fpv_derive_reset_jitter)
    return lo32, span32


def _quat64(r, p, y):
    """q = qz(yaw) (x) qy(pitch) (x) qx(roll), float64 (params.ypr_to_quat, vectorised)"""
    r, p, y = (np.radians(a) * 0.5 for a in (r, p, y))
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.stack([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr,
                     sy * cp * cr - cy * sp * sr], axis=-1)


def _hamilton64(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def _pairs(n, seed=11):
    rng = np.random.default_rng(seed)
    gids = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
    gids[: n // 4] = rng.integers(0, 2 ** 20, size=n // 4, dtype=np.uint64)         # small ids (one shard) ...
    gids[n // 4: n // 2] += np.uint64(1 << 32)                                       # ... and ids above 2^32
    steps = rng.integers(0, 2 ** 40, size=n, dtype=np.uint64)
    steps[: n // 3] = rng.integers(0, 2 ** 16, size=n // 3, dtype=np.uint64)        # step indices below and above 2^32
    es = rng.integers(0, 2, size=n)
    return gids, steps, es


def _ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def test_sample_matches_float64_restatement_of_the_counter_convention():
    cp = _lib.pack_params(_params())
    assert cp.flags & _lib.FPV_FLAG_RESET_JITTER
    gids, steps, es = _pairs(10_000)
    got = _samples(cp, gids, steps, es).astype(np.float64)
    lo, span = _boxes()
    want = lo[None] + span[None] * _reference_u(gids, steps, es)                    # [n, 3, 3]
    for b, rows in ((0, slice(0, 3)), (1, slice(3, 6))):
        err = np.abs(got[:, rows] - want[:, b, :])
        assert np.all(err <= _ulp32(got[:, rows])), (b, err.max())
    q64 = _quat64(want[:, 2, 0], want[:, 2, 1], want[:, 2, 2])                     # identity base: q = the jitter rotation
    assert np.abs(got[:, 6:10] - q64).max() < 2e-6


def test_nonzero_base_adds_in_fp32_and_rotates_in_the_body_frame():
    cp = _lib.pack_params(_params())
    gids, steps, es = _pairs(2000, seed=5)
    rng = np.random.default_rng(3)
    qb = rng.normal(size=4)
    qb /= np.linalg.norm(qb)
    base = np.concatenate([rng.uniform(-50, 50, 3), rng.uniform(-5, 5, 3), qb]).astype(np.float32)
    got = _samples(cp, gids, steps, es, base).astype(np.float64)
    lo, span = _boxes()
    want = lo[None] + span[None] * _reference_u(gids, steps, es)
    for b, rows in ((0, slice(0, 3)), (1, slice(3, 6))):
        sum32 = (base[rows].astype(np.float64)[None] + want[:, b, :].astype(np.float32)).astype(np.float32)
        assert np.all(np.abs(got[:, rows] - sum32) <= _ulp32(sum32)), b
    q = _hamilton64(base[6:].astype(np.float64)[None], _quat64(want[:, 2, 0], want[:, 2, 1], want[:, 2, 2]))
    assert np.abs(got[:, 6:10] - q).max() < 2e-6


def test_samples_are_uniform_on_their_box_and_the_streams_independent():
    cp = _lib.pack_params(_params())
    n = 100_000
    gids = np.arange(n, dtype=np.uint64) + np.uint64(7 << 32)
    steps = np.full(n, 123_456, dtype=np.uint64)
    a = _samples(cp, gids, steps, np.zeros(n, dtype=int))
    b = _samples(cp, gids, steps, np.ones(n, dtype=int))
    lo = np.array(POS[0] + VEL[0], dtype=np.float32)
    hi = np.array(POS[1] + VEL[1], dtype=np.float32)
    for s in (a, b):
        assert np.all(s[:, :6] >= lo) and np.all(s[:, :6] <= hi)                  # bounds exactly representable
        m, v = s[:, :6].astype(np.float64).mean(0), s[:, :6].astype(np.float64).var(0)
        span = (hi - lo).astype(np.float64)
        assert np.all(np.abs(m - (lo + hi) / 2) < 4 * span / math.sqrt(12 * n))
        assert np.all(np.abs(v / (span ** 2 / 12) - 1) < 0.02)
        assert np.allclose(np.linalg.norm(s[:, 6:10].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the blocks (position vs velocity vs angles) and e = 0 vs e = 1 draw from different counters: uncorrelated
    pairs = [(a[:, 0], a[:, 3]), (a[:, 1], a[:, 4]), (a[:, 0], a[:, 9]), (a[:, 0], b[:, 0]), (a[:, 3], b[:, 3]), (a[:, 0], a[:, 1])]
    for x, y in pairs:
        assert abs(np.corrcoef(x.astype(np.float64), y.astype(np.float64))[0, 1]) < 0.015


def test_without_jitter_the_pose_is_the_base_bit_for_bit():
    cp = _lib.pack_params(load_params(fps=1000))
    assert not cp.flags & _lib.FPV_FLAG_RESET_JITTER
    rng = np.random.default_rng(1)
    for k in range(50):
        base = rng.normal(size=10).astype(np.float32) * np.float32(10.0 ** int(rng.integers(-3, 4)))
        rc, out = _sample(cp, rng.integers(0, 2 ** 63), rng.integers(0, 2 ** 63), k & 1, base)
        assert rc == 0 and out.view(np.uint32).tolist() == base.view(np.uint32).tolist()


def test_zero_angle_box_keeps_the_base_quaternion_bitwise():
    cp = _lib.pack_params(_params(reset_ypr_range_deg=None, reset_velocity_range=None))
    rng = np.random.default_rng(2)
    for k in range(200):
        q = rng.normal(size=4)
        q = (q / np.linalg.norm(q)) if k else np.array([1.0, 0.0, 0.0, 0.0])
        base = np.concatenate([rng.normal(size=6), q]).astype(np.float32)
        rc, out = _sample(cp, k, 1000 + k, k & 1, base)
        assert rc == 0
        assert out[6:].view(np.uint32).tolist() == base[6:].view(np.uint32).tolist()
        assert out[3:6].view(np.uint32).tolist() == base[3:6].view(np.uint32).tolist()      # a zero box adds +0


def test_pack_params_sets_flag_boxes_and_seed():
    cp = _lib.pack_params(_params(reset_velocity_range=None))
    assert cp.flags & _lib.FPV_FLAG_RESET_JITTER and cp.reset_seed == SEED
    assert [list(r) for r in cp.reset_pos_range] == POS and [list(r) for r in cp.reset_vel_range] == [[0.0] * 3] * 2
    assert [list(r) for r in cp.reset_ypr_range_deg] == YPR
    with pytest.raises(ValueError):
        _lib.pack_params(_params(reset_position_range=[[0, 0, 0]]))


@pytest.mark.parametrize("bad", [
    dict(reset_position_range=[[0.0, 1.0, 0.0], [1.0, 0.5, 1.0]]),            # lo > hi
    dict(reset_velocity_range=[[float("nan"), 0.0, 0.0], [1.0, 1.0, 1.0]]),   # NaN bound
    dict(reset_ypr_range_deg=[[0.0, 0.0, 0.0], [1.0, float("inf"), 1.0]]),    # infinite bound
])
def test_create_and_sample_reject_bad_boxes(bad):
    L = _lib.lib()
    cp = _lib.pack_params(_params(**bad))
    h = C.c_void_p()
    assert L.fpv_create(C.byref(cp), 1024, 0, C.byref(h)) == FPV_EPARAM          # checked before the device is asked for
    assert b"reset_" in L.fpv_last_error()
    assert _sample(cp, 0, 0, 0, np.zeros(10))[0] == FPV_EPARAM


def test_racer_handle_with_jitter_is_refused():
    L = _lib.lib()
    cp = _lib.pack_params(_params(mode=1))
    h = C.c_void_p()
    assert L.fpv_create(C.byref(cp), 1024, 0, C.byref(h)) == FPV_EINVAL
    assert b"RESET_JITTER" in L.fpv_last_error()


def test_sizeof_matches_the_ctypes_structs():
    L = _lib.lib()
    assert L.fpv_abi_version() == _lib.FPV_ABI_VERSION == 9
    for which, struct in ((0, _lib.FpvParams), (1, _lib.FpvBuffers)):
        assert L.fpv_sizeof(which) == C.sizeof(struct)
    assert _lib.FpvBuffers.reset_pose.offset == C.sizeof(_lib.FpvBuffers) - 8           # appended last
    assert _lib.FpvParams.reset_seed.offset == C.sizeof(_lib.FpvParams) - 8
    assert "fpv_reset_pose_sample" in _lib.EXPORTS
