"""The object table, the seeded scene and the float64 restatement that tests/test_range_host.py (CPU) and tests/test_gpu_range.py
share (include/fpv_abi.h "Range scan").

The restatement is written from the definition, not from csrc/fpv_range.h: fp32 inputs widened to float64, d = R(q) d_b without
renormalisation, the textbook quadratic for ball and circle, one interval per convex solid.
"""
import functools

import numpy as np

from fpyv_amd import rays as RY
from fpyv_amd.objects import Cylinder, Ground, Target

MAX_RANGE = 20.0
MARGIN = 1.0e-4


def table():
    """the eight objects of the issue's table, in its order; the first four are the G10 world"""
    return [Target([1.5, -6.0, 3.0], 0.8), Cylinder([3.0, 0.0, 0.0], 1.0, 5.0), Cylinder([-2.0, 2.5, 0.0], 0.6, 1.5), Ground(),
            Target([-5.0, -5.0, 2.0], 1.5), Cylinder([6.0, 6.0, 0.0], 0.5, 7.0), Target([0.0, 4.0, 6.0], 1.0),
            Cylinder([-6.0, 3.0, 1.0], 2.0, 2.0)]


def world(count):
    """the object lists of length 0 (nothing), 1 (ground only), 4 (the G10 world) and 8 (the whole table)"""
    t = table()
    return {0: [], 1: [t[3]], 4: t[:4], 8: t}[count]


@functools.lru_cache(maxsize=None)
def scene(n=1024, rays=16, seed=11):
    """(p [n, 3], q [n, 4] wxyz, ray set [rays, 3]) float32: p uniform in [-8, 8]^2 x [0.2, 8], q a random unit quaternion, random
    unit rays.  Computed once; treat as read-only."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0.2, 8, n)], 1).astype(np.float32)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return p, q, RY.derive(rng.normal(size=(rays, 3)))


def rot64(q):
    """R(q) [n, 3, 3] in float64 from fp32 quaternions (wxyz), the algebraic form the stepper uses everywhere"""
    w, x, y, z = (q.astype(np.float64)[:, k] for k in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def _quadratic(oc, d, r):
    """the interval of |oc - t d| <= r over the given components: (t_in, t_out, margin); parallel: all or nothing, margin inf"""
    a, b, c = (d * d).sum(-1), (oc * d).sum(-1), (oc * oc).sum(-1) - r * r
    par = a == 0.0
    a1 = np.where(par, 1.0, a)
    disc = b * b - a1 * c
    s = np.sqrt(np.maximum(disc, 0.0))
    t_in = np.where(par, np.where(c <= 0, -np.inf, np.inf), np.where(disc >= 0, (b - s) / a1, np.inf))
    t_out = np.where(par, np.where(c <= 0, np.inf, -np.inf), np.where(disc >= 0, (b + s) / a1, -np.inf))
    return t_in, t_out, np.where(par, np.inf, np.abs(disc) / (a1 * r * r))          # the discriminant relative to r^2


def _slab(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    inside = (lo <= o) & (o <= hi)
    par = d == 0.0
    return (np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2)),
            np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2)))


class Nearest:
    """The nearest thing per ray so far, for origins o [n, 3] and directions d [n, ..., 3] (any shape between), and what the
    restatements return of it: `take` a thing's t, where it is hit, where its margins are wide enough to call, its index and centre."""

    def __init__(self, o, d):
        self.shape = d.shape[:-1]
        self.oo = o.reshape((o.shape[0],) + (1,) * (d.ndim - 2) + (3,))
        self.best, self.which = np.full(self.shape, np.inf), np.full(self.shape, -1)
        self.keep, self.centre = np.ones(self.shape, bool), np.zeros(self.shape)
        self.pairs = self.dropped = 0

    def take(self, t, hit, ok, k, c):
        self.pairs += ok.size
        self.dropped += int((~ok).sum())
        self.keep &= ok
        t = np.where(hit, t, np.inf)
        nearer = t < self.best
        self.best, self.which = np.where(nearer, t, self.best), np.where(nearer, k, self.which)
        self.centre = np.where(nearer, np.broadcast_to(np.linalg.norm(c - self.oo, axis=-1), self.shape), self.centre)

    def result(self, limit):
        """(distance, nearest thing or -1, keep, scale): `scale` is max(distance, distance from the origin to the nearest thing's
        centre) - what an error is measured in"""
        seen = self.best < limit
        dist = np.where(seen, self.best, limit)
        return dist, np.where(seen, self.which, -1), self.keep, np.maximum(dist, np.where(seen, self.centre, 0.0))


def solids(near, d, object_list):
    """THE float64 loop over the solids, from the definition: every object of `object_list` against the rays of `near` (a Nearest)
    along d.  A ray is not kept where, for some object, the discriminant is below MARGIN of r^2 or the entry / exit gap below
    MARGIN of |t_in| + |t_out|."""
    from fpyv_amd.objects import to_rows
    rows = np.asarray(to_rows(object_list), dtype=np.float32).astype(np.float64).reshape(-1, 6)
    oo, shape = near.oo, near.shape
    for k, (typ, x, y, z, r, h) in enumerate(rows):
        c = np.array([x, y, z])
        margin = np.full(shape, np.inf)
        if typ == 0:
            t_in, t_out = _slab(oo[..., 2], d[..., 2], -np.inf, 0.0)
        elif typ == 1:
            t_in, t_out, margin = _quadratic((c - oo)[..., :2], d[..., :2], r)
            z_in, z_out = _slab(oo[..., 2], d[..., 2], z, z + h)
            t_in, t_out = np.maximum(t_in, z_in), np.minimum(t_out, z_out)
        else:
            t_in, t_out, margin = _quadratic(c - oo, d, r)
        t_in, t_out = np.broadcast_to(t_in, shape), np.broadcast_to(t_out, shape)
        fin = np.isfinite(t_in) & np.isfinite(t_out)
        with np.errstate(invalid="ignore"):
            gap = np.where(fin, np.abs(t_out - t_in) / np.maximum(np.abs(t_in) + np.abs(t_out), 1e-300), np.inf)
        near.take(np.maximum(t_in, 0.0), (t_in <= t_out) & (t_out >= 0), (margin >= MARGIN) & (gap >= MARGIN), k, c)


def restate(p, q, rays, object_list, max_range=MAX_RANGE):
    """float64, from the definition.  Returns (range [R, n], nearest [R, n] object index or -1, keep [R, n] bool, scale [R, n]):
    `keep` is False where a margin of `solids` is too small to call; `scale` is max(range, distance from the drone to the nearest
    object's centre) - what an error is measured in."""
    d = np.einsum("nij,rj->rni", rot64(q), rays.astype(np.float64)).transpose(1, 0, 2)      # [n, R, 3]
    near = Nearest(p.astype(np.float64), d)
    solids(near, d, object_list)
    return tuple(np.ascontiguousarray(a.T) for a in near.result(max_range))
