"""Every sensor and the pursuit task on one env at once: range rays, depth camera, box detector with the own-target slot, point-cloud
camera with its centroid, a guided pursuit task and a gate course, each on its own cadence, with in-kernel auto-resets, a masked
reset and a moving Target.  384 drones in two partitions are the column ranges [0, 128) and [128, 384): a pointer of a partition
moved by the wrong step lands in the other one's columns.  The unpartitioned env, the env with partitions=2 driven by step() and a
third one driven by step_async / step_wait agree BIT FOR BIT after every call - obs, reward, done, every sensor output and every
info entry -, and what step_wait(k) hands out is the [lo:hi] slice of the whole population's entry."""
import numpy as np
import pytest
import torch

from attached_env import COLUMNS_LAST, DEV, INFO_KEYS, N, OUTPUTS, VIEWS, env as _env, same as _same, world as _world

pytestmark = pytest.mark.gpu
STEPS, RESET_AFTER = 7, 3


def _whole(env, one, what):
    """every output of `env` is the unpartitioned env's, bit for bit"""
    torch.cuda.synchronize()
    assert _same(env.obs, one.obs) and _same(env.batch.reward, one.batch.reward) and _same(env.batch.done, one.batch.done), what
    for name in OUTPUTS:
        assert _same(getattr(env.batch, name), getattr(one.batch, name)), (what, name)
    for g, h in zip(env.batch.pursuit_guidance, one.batch.pursuit_guidance):
        assert _same(g, h), what
    for name in VIEWS:
        assert _same(getattr(env, name), getattr(one, name)), (what, name)


def _results(got, want, what, lo=None, hi=None):
    """a step's (obs, reward, done, info) is another's - or, with [lo, hi), that range of its columns - bit for bit, key for key"""
    cut = (lambda t, last=False: t) if lo is None else (lambda t, last=False: t[..., lo:hi] if last else t[lo:hi])
    for a, b in zip(got[:3], want[:3]):
        assert _same(a, cut(b)), what
    assert set(got[3]) == set(want[3]) == INFO_KEYS, what
    for key in INFO_KEYS:
        assert _same(got[3][key], cut(want[3][key], key in COLUMNS_LAST)), (what, key)


def test_partitions_and_split_phase_change_no_bit_of_an_env_with_every_attachment():
    objs, target = _world()
    (one, pos, vel), (two, _, _), (split, _, _) = _env(objs, 1), _env(objs, 2), _env(objs, 2)
    assert two.partitions == 2 and [split.partition_range(k) for k in (0, 1)] == [(0, 128), (128, 384)]
    for e in (one, two, split):
        e.reset(position=pos, velocity=vel)
    _whole(two, one, "reset"); _whole(split, one, "reset")
    sticks = torch.from_numpy(np.random.default_rng(5).uniform(-0.2, 0.2, (STEPS, N, 4)).astype(np.float32)).to(DEV)
    sticks[..., 3] = 0.8
    mask = torch.arange(N, device=DEV) % 3 == 0
    resets = 0
    for t in range(STEPS):
        target.update()
        want = one.step(sticks[t])
        _results(two.step(sticks[t]), want, t)
        for k in (0, 1):
            lo, hi = split.partition_range(k)
            split.step_async(k, sticks[t, lo:hi])
        parts = {k: split.step_wait(k) for k in (1, 0)}
        torch.cuda.synchronize()
        for k, got in parts.items():
            _results(got, want, (t, k), *split.partition_range(k))
        _whole(two, one, t); _whole(split, one, t)
        resets += int(want[2].sum())
        if t + 1 == RESET_AFTER:
            for e in (one, two, split):
                e.reset(mask)
            _whole(two, one, "masked reset"); _whole(split, one, "masked reset")
    assert resets > 10 and one.batch.range_rows.any() and one.depth.any() and one.box_visible.any() and one.points_image.any()
    target.update()
    for call in ("render_depth", "detect", "render_points"):
        outs = [getattr(e, call)() for e in (one, two, split)]
        _whole(two, one, call); _whole(split, one, call)
        assert _same(outs[1], outs[0]) and _same(outs[2], outs[0]), call
    for e in (one, two, split):
        e.close()
