"""The edge-lane set that tests/test_edge_lanes_host.py (CPU) and tests/test_gpu_edge_lanes.py share: a few hundred drones, each put
by construction on one input that no flight visits - a non-finite or absurd coordinate, a denormal, a quaternion off the unit
sphere, an exact turn, a target on the camera origin, on an image border or at max_depth, a force parallel to a cross product's
operand, the thrust limit's three outcomes, commands and caller's rows holding anything, an origin on a surface, a grazing ray, a
garbage counter word - next to flight-like controls that see the target and hit things.  The law and sensor headers
(csrc/fpv_chase.h 4., fpv_pns.h 1. 5. 6., fpv_range.h "Parallel rays", fpv_depth.h, fpv_pursuit.h) define what each of them gives;
the host module pins that every class reaches its branch, the GPU module that the kernels answer with the host functions' bits.

A lane is a pose (p, v, q) plus what each call reads per drone: a target of its own, the caller's pixel, the four commands, the
guidance PID's rows, prev_pixel, a restart byte, the pursuit task's target row and done byte.  Lanes that are about one of these
stand on a pose that faces the shared target, so that the input is read by a guided lane.  Built once; treat as read-only.

Two inputs that fp32 cannot be put on, and what stands in for them.  czp = -0: czp = fmaf(rr2, bx, fmaf(rr5, by, rr8 bz)) is -0 only
when each of the three products is; with this camera (rr2, rr8 > 0, rr5 = +0) that needs bx = bz = -0 and by < 0, and b = R^T (c - o)
has a -0 component only when all its three products are -0 - with differences that cancel to +0, four entries of R's 2 x 2 block
across x and z negative or -0 at once, which fpv_rot gives for no quaternion (r02 and r20 hold +wy and -wy).  The `origin` lanes have
czp = +0 with cxp of both signs (a level drone and one rolled half round); the host module asserts it with `camera_frame`.  A
discriminant of exactly 0: disc = fmaf(b, b, c) is ONE rounding of b^2 + c, 0 only when the 48-bit square equals the 24-bit -c, or
b = 0 and Fmax^2 - no fp32 value - equals an fp32 |B|^2.  The `limit` lanes hold the two neighbouring speeds between which it
changes its sign.
"""
import functools
import pathlib
import re

import numpy as np

import depth_scene as DS
import gate_course as gc
import pursuit_task as PT
import range_scene as RS
from chase_law import quat_of
from fpyv_amd import _lib, load_params
from fpyv_amd import gates as G
from fpyv_amd import rays as RY
from fpyv_amd.camera import DepthCamera, gate_rows
from fpyv_amd.chase import ChaseGuidance
from fpyv_amd.objects import Gate
from fpyv_amd.pns import PointAndShoot
from gate_course import rot_zyx
from oracle import lane_model
from pns_law import PnsLaw

FPS = 250
CENTRE = np.array([2.0, -1.0, 4.0], dtype=np.float32)          # the shared target (tests/test_gpu_pns.py's)
RADIUS = 0.5
MAX_DEPTH = 15.0                                                # the laws' reach (simulator.py:102)
PAIRS = [("world", "level"), ("world", "frontarget"), ("drone", "level"), ("drone", "frontarget")]
NAN, INF = np.float32(np.nan), np.float32(np.inf)
DENORMAL = np.float32(1e-40)
FLUSH = np.float32(2.0 ** -48)                                  # fpv_sqrt_flushed: |v|^2 below 2^-96 is 0
K_PATH = PT.TASK_KW["path"]["resolution"]                       # the pursuit task's path resolution K
CAPTURE = PT.TASK_KW["capture_distance"]
GRAZE_RAY = 8 + 8                                               # the ray of ray_set() that the `graze` lanes are built on
AXIS_RAYS = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1e-13, 0], [1e-13, 0, 1]]   # test_range_host's list
# the origins of tests/test_range_host.py::test_parallel_and_degenerate_rays_give_no_nan: over the ground, inside a cylinder, above its
# axis, on the ground at a cylinder's foot, a ball's centre, the world's origin, on a cap, below the ground
AXIS_ORIGINS = [[0, 0, 5], [3, 0, 2], [3, 0, 9], [-6, 3, 0], [1.5, -6, 3], [0, 0, 0], [6, 6, 7], [-2, 2.5, -1]]


def params():
    return load_params(fps=FPS)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def up(x):
    return np.nextafter(np.float32(x), INF)


def down(x):
    return np.nextafter(np.float32(x), -INF)


def ray_set():
    """the axis list and range_scene's 16 seeded rays: 24 unit directions"""
    return np.concatenate([RY.derive(AXIS_RAYS), RS.scene()[2]])


def level_rays(which):
    """the ray list with |d_z| an ulp either side of fpv_range.h's 1e-12: (1, 0, +-z) normalised is (1, 0, +-z) in fp32"""
    z = np.float32(1e-12)
    return f32([[1, 0, up(z)], [1, 0, down(z)], [1, 0, -up(z)], [1, 0, -down(z)], [1, 0, z]])[which]


class _Law:
    """the camera of the params in float64 and the placement of a drone that sees CENTRE at a chosen pixel and depth"""

    def __init__(self):
        self.law = PnsLaw.from_params(params(), MAX_DEPTH)

    def place(self, R, pixel, depth, centre=CENTRE):
        """(p, q) fp32 of the drone with attitude R whose camera projects `centre` to `pixel` at z-depth `depth` (up to the fp32
        rounding of p and q)"""
        L = self.law
        pc = np.array([(pixel[0] - L.w / 2) / L.f * depth, (pixel[1] - L.h / 2) / L.f * depth, depth])
        p = np.asarray(centre, dtype=np.float64) - R @ (L.rel + L.rr @ pc)
        return f32(p), f32(quat_of(R))

    def limit_terms(self, p, v, R, pixel, frame="world"):
        """(discriminant, root r, min_output, max_output) of the thrust limit's quadratic (csrc/fpv_pns.h 5.) in float64, as
        tests/pns_law.py forms them: which end the root is clipped at is not among the host function's outputs"""
        L = self.law
        p, v, R = (np.asarray(x, dtype=np.float64) for x in (p, v, R))
        d = R @ (L.rr @ np.array([(pixel[0] - L.w / 2) / L.f, (pixel[1] - L.h / 2) / L.f, 1.0]))
        d = d / np.linalg.norm(d)
        g, w = (R @ L.g, R @ v) if frame == "drone" else (L.g, v)
        s = np.linalg.norm(v)
        drag = np.zeros(3) if s == 0.0 else L.vdrag * (-(w @ d / s - 1.0) / 2.0) * (-w) * s
        lift = float(p[2] < L.tof) * -(L.tof - p[2]) * L.vlift * g * -min(v[2], 0.0)
        B = drag + lift - g
        b = d @ B
        disc = b * b - B @ B + L.fmax ** 2
        return disc, (np.sqrt(disc) if disc >= 0 else 0.0) - b, L.lo, L.hi

    def pixel_of(self, R, world_dir):
        """the pixel whose direction is `world_dir` for a drone with attitude R"""
        L = self.law
        d = L.rr.T @ (R.T @ np.asarray(world_dir, dtype=np.float64))
        return f32([L.f * d[0] / d[2] + L.w / 2, L.f * d[1] / d[2] + L.h / 2])


def _fma(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64, so this is the sum rounded twice - the fp32 fma up to a
    double rounding, and exactly it wherever the sum is exact (a zero and its sign, which is what `camera_frame` is read for)"""
    return f32(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))


def camera_frame(p, q, centre=CENTRE):
    """(cxp, cyp, czp) [n] fp32: the target's centre in the camera's frame, operation by operation as csrc/fpv_chase.h 1. forms it
    (fpv_rot, the origin o = p + R rel, b = R^T (c - o), rel_rot^T b) - the host function does not give them out, and the sign of a
    zero czp is what the `origin` lanes are about"""
    s = ChaseGuidance(params(), max_depth=MAX_DEPTH).derive((CENTRE, RADIUS))
    rr, rel = f32(list(s.relative_rotation)), f32(list(s.relative_position))
    p, q, c = f32(p).reshape(-1, 3), f32(q).reshape(-1, 4), f32(centre)
    w, x, y, z = q.T
    with np.errstate(all="ignore"):
        x2, y2, z2 = x + x, y + y, z + z
        xx, yy, zz, wx, wy, wz = x * x2, y * y2, z * z2, w * x2, w * y2, w * z2
        ax, ay = np.float32(1.0) - xx, np.float32(1.0) - yy
        R = [[ay - zz, _fma(x, y2, -wz), _fma(x, z2, wy)], [_fma(x, y2, wz), ax - zz, _fma(y, z2, -wx)], [_fma(x, z2, -wy), _fma(y, z2, wx), ax - yy]]
        o = [_fma(R[k][0], rel[0], _fma(R[k][1], rel[1], _fma(R[k][2], rel[2], p[:, k]))) for k in range(3)]
        d = [c[k] - o[k] for k in range(3)]
        b = [_fma(R[0][k], d[0], _fma(R[1][k], d[1], R[2][k] * d[2])) for k in range(3)]
        return tuple(_fma(rr[k], b[0], _fma(rr[3 + k], b[1], rr[6 + k] * b[2])) for k in range(3))


def _bisect(make, pred, lo, hi, trips=80):
    """the two values of a float64 parameter, next to each other, between which pred(make(t)) changes: (t with pred == pred(lo), t with
    pred == pred(hi))"""
    a, b = pred(make(lo)), pred(make(hi))
    assert a != b, "the bracket does not hold the threshold"
    for _ in range(trips):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if pred(make(mid)) == a:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _bisect_f32(pred, lo, hi):
    """the two neighbouring fp32 values in [lo, hi] (same sign) between which pred changes"""
    lo, hi = np.float32(lo), np.float32(hi)
    a = pred(lo)
    assert a != pred(hi), "the bracket does not hold the threshold"
    while np.nextafter(lo, hi) != hi:
        mid = np.float32(0.5 * (np.float64(lo) + np.float64(hi)))
        if mid == lo or mid == hi:
            mid = np.nextafter(lo, hi)
        if pred(mid) == a:
            lo = mid
        else:
            hi = mid
    return lo, hi


class Lanes:
    """The set.  Arrays over the N lanes: p, v [N, 3], q [N, 4], cls [N] (the class tag), note [N]; own [N, 3] the lane's own target,
    pixel [N, 2] the caller's pixel, action [N, 4], pid [4, N], prev [2, N], restart [N] uint8; the pursuit rows tgt [8, N] (words
    bit-cast) and done [N] uint8."""

    def __init__(self):
        self._rows = []

    def add(self, cls, p, v, q, note="", **extra):
        self._rows.append(dict(cls=cls, p=f32(p).copy(), v=f32(v).copy(), q=f32(q).copy(), note=note, **extra))
        return len(self._rows) - 1

    def freeze(self):
        rows, n = self._rows, len(self._rows)
        rng = np.random.default_rng(77)
        self.n = n
        self.cls = np.array([r["cls"] for r in rows])
        self.note = [r["note"] for r in rows]
        self.p, self.v, self.q = (np.stack([r[k] for r in rows]) for k in ("p", "v", "q"))
        get = lambda key, default: np.stack([f32(r[key]) if key in r else f32(d) for r, d in zip(rows, default)])  # noqa: E731
        self.own = get("own", np.tile(CENTRE, (n, 1)))
        self.pixel = get("pixel", rng.uniform([60, 60], [580, 420], (n, 2)))
        self.action = get("action", rng.uniform(-0.4, 0.4, (n, 4)))
        self.pid = get("pid", np.tile([0.0, 0.0, 0.0, 1.0], (n, 1))).T.copy()
        self.prev = get("prev", np.full((n, 2), np.nan)).T.copy()
        # the restart bytes of a second call: every third lane, and the lanes that hold a byte of their own (0xFF)
        self.on = np.array([r.get("on", -1) for r in rows])                  # the object whose surface p stands on ...
        self.camera_on = np.array([r.get("camera_on", -1) for r in rows])    # ... and the camera's origin (level: p + rel)
        self.restart = np.array([r.get("restart", int(i % 3 == 0)) for i, r in enumerate(rows)], dtype=np.uint8)
        self.done = np.array([r.get("done", int(i % 3 == 0 and r["cls"] in ("base", "nonfinite", "overflow", "tiny", "quat", "turn")))
                              for i, r in enumerate(rows)], dtype=np.uint8)
        # the pursuit rows: the target stands at the lane's own target (PATH_R 0) unless the lane says otherwise
        tgt = np.zeros((8, n), dtype=np.float32)
        words = tgt.view(np.uint32)
        tgt[0:3] = self.own.T
        for i, r in enumerate(rows):
            tgt[_lib.TGT_PATH_R, i] = r.get("path_r", 1.5 if (r["cls"] == "base" and i % 2) else 0.0)
            tgt[_lib.TGT_RADIUS, i] = r.get("radius", RADIUS)
            tgt[_lib.TGT_PREV_DIST, i] = r.get("prev_dist", 3.0 + 0.01 * i)
            words[_lib.TGT_COUNT, i] = r.get("count", (i % K_PATH) | (_lib.FPV_TGT_FRESH if i % 2 else 0))
            words[_lib.TGT_SPAWNS, i] = r.get("spawns", (i % 5) | ((i % 3) << 16))
        self.tgt = tgt
        for a in (self.p, self.v, self.q, self.own, self.pixel, self.action, self.pid, self.prev, self.restart, self.done, self.tgt):
            a.setflags(write=False)
        return self

    def of(self, *classes):
        return np.flatnonzero(np.isin(self.cls, classes))

    def counts(self):
        names, c = np.unique(self.cls, return_counts=True)
        return dict(zip(names.tolist(), c.tolist()))


FINITE_DEGENERATE = ("tiny", "turn", "surface", "inside", "graze", "cull", "reach", "fallback1", "fallback2", "still", "limit", "tof")
POSE_CLASSES = ("base", "nonfinite", "overflow", "tiny", "quat", "turn")


@functools.lru_cache(maxsize=None)
def lanes():
    S, cam, P = Lanes(), _Law(), params()
    L = cam.law
    rng = np.random.default_rng(2024)
    chase = ChaseGuidance(P, max_depth=MAX_DEPTH)
    pns = PointAndShoot(P, max_depth=MAX_DEPTH)
    tof = np.float32(P.point_and_shoot["tof_effective_distance"])

    def sees(p, q, v=(0, 0, 0)):
        return bool(chase.evaluate([p], [v], [q], (CENTRE, RADIUS))[3][0])

    # ---- base: flight-like controls.  28 face the target (8 of them from below the tof height), 12 look away
    for i in range(40):
        low = 20 <= i < 28
        while True:                                             # (over the ground: below the tof height or above it, as the lane asks)
            R = rot_zyx(yaw=rng.uniform(-180, 180), pitch=rng.uniform(-10, 10), roll=rng.uniform(-10, 10))
            pixel = (rng.uniform(60, 580), rng.uniform(20, 100) if low else rng.uniform(60, 420))
            p, q = cam.place(R, pixel, rng.uniform(1.7, 2.5) if low else rng.uniform(2.5, 13.0))
            if 0.3 < p[2] < tof or (not low and p[2] > tof):
                break
        if i >= 28:
            q = f32(quat_of(R @ rot_zyx(yaw=180.0)))
        v = rng.uniform(-4, 4, 3)
        if i % 5 == 2:
            v *= rng.uniform(15.0, 45.0) / np.linalg.norm(v)        # the thrust limit is out of reach
        if i % 5 == 3:
            v = (p - CENTRE) * rng.uniform(9.0, 12.5) / np.linalg.norm(p - CENTRE)      # flying away from the target: the limit binds
        if i == 4:
            v = np.zeros(3)
        S.add("base", p, v, q, own=CENTRE + (rng.uniform(-0.3, 0.3, 3) if i % 4 == 1 else 0.0))
    B = cam.place(rot_zyx(yaw=30.0, pitch=4.0, roll=-3.0), (300.0, 400.0), 5.0)        # 4.6 m over the ground
    base = np.concatenate([B[0], f32([1.5, -2.0, 0.5]), B[1]])
    names = ["p.x", "p.y", "p.z", "v.x", "v.y", "v.z", "q.w", "q.x", "q.y", "q.z"]

    def one_coordinate(cls, values):
        for c in range(10):
            for val in values:
                x = base.copy()
                x[c] = val
                S.add(cls, x[0:3], x[3:6], x[6:10], note=f"{names[c]} = {val!r}")

    # ---- nonfinite, overflow, tiny: one coordinate of the base pose at a time
    one_coordinate("nonfinite", [NAN, INF, -INF])
    one_coordinate("overflow", [3e38, -3e38, 1e30, -1e30, 1e19, -1e19])
    S.add("overflow", base[0:3], [1e20, 1e20, 1e20], base[6:10], note="v = 1e20 on all axes")
    S.add("overflow", base[0:3], [-1e20, 1e20, -1e20], base[6:10], note="v = +-1e20 on all axes")
    one_coordinate("tiny", [DENORMAL, -DENORMAL, np.float32(0.0), np.float32(-0.0), np.float32(1e-20)])
    for vx, what in ((0.0, "|v| = 0"), (DENORMAL, "|v| denormal"), (FLUSH, "|v| = 2^-48: kept"), (down(FLUSH), "|v| an ulp below 2^-48: flushed"),
                     (up(FLUSH), "|v| an ulp above 2^-48")):
        S.add("tiny", base[0:3], [vx, 0, 0], base[6:10], note=what)
        S.add("tiny", base[0:3], [0, 0, -vx], base[6:10], note=what + " (v.z)")
    # ---- quat: off the unit sphere
    qb = base[6:10]
    S.add("quat", base[0:3], base[3:6], np.zeros(4), note="q = 0")
    S.add("quat", [0, 0, 5], [1, 0, 0], np.zeros(4), note="q = 0")
    S.add("quat", base[0:3], base[3:6], 2.0 * qb, note="2 q")
    S.add("quat", base[0:3], base[3:6], 0.5 * qb, note="q / 2")
    S.add("quat", base[0:3], base[3:6], -qb, note="-q")
    for c in range(4):
        for val in (np.float32(0.0), np.float32(-0.0), DENORMAL):
            x = qb.copy()
            x[c] = val
            S.add("quat", base[0:3], base[3:6], x, note=f"{names[6 + c]} = {val!r}")
    # ---- turn: the identity and the 90 and 180 degree turns about each axis - R holds exact zeros
    h = np.float32(np.sqrt(0.5))
    turns = [[1, 0, 0, 0], [h, h, 0, 0], [h, -h, 0, 0], [h, 0, h, 0], [h, 0, -h, 0], [h, 0, 0, h], [h, 0, 0, -h], [0, 1, 0, 0], [0, 0, 1, 0],
             [0, 0, 0, 1]]
    for t in turns:
        for o in ([0, 0, 5], [3, 0, 9], [6, 6, 7], [1.0, -1.0, 3.0]):
            S.add("turn", o, [0.5, 0.0, -0.25], t)
    # ---- surface / inside: the origin on a surface of the range_scene / depth_scene world, or inside a solid
    level, tilted = f32([1, 0, 0, 0]), f32(quat_of(rot_zyx(yaw=40.0, pitch=-20.0, roll=10.0)))
    rel_x = np.float32(L.rel[0])
    # (the third entry: the object of range_scene.table() whose surface it is, -1 for none of them)
    on = [([0, 0, 0], "ground", 3), ([5, 5, -0.0], "ground, z = -0", 3), ([4, 0, 2], "cylinder wall", 1), ([3, 0, 5], "cylinder cap", 1),
          ([4, 0, 5], "cylinder rim", 1), ([1.5, -6, 3.8], "ball, top", 0), ([2.3, -6, 3], "ball, side", 0), ([7.0, 0, 3], "gate 0's plane", -1),
          ([-6, 3, 0], "ground at a cylinder's foot", 3), ([6, 6, 7], "cap", 5)]
    for o, what, k in on:
        S.add("surface", o, [0, 0, 0], level, note=what, on=k)
        S.add("surface", o, [0, 0, 0], tilted, note=what + ", tilted", on=k)
        # ... and with the CAMERA's origin there: p.x + rel.x == o.x in fp32 (level attitude: o = p + rel)
        px = np.float32(np.float32(o[0]) - rel_x)
        for cand in (px, up(px), down(px), up(up(px)), down(down(px))):
            if np.float32(cand + rel_x) == np.float32(o[0]):
                S.add("surface", [cand, o[1], o[2]], [0, 0, 0], level, note=what + ", camera origin", camera_on=k)
                break
    for o, k in zip(AXIS_ORIGINS, (-1, -1, -1, 3, -1, 3, 5, -1)):
        S.add("surface", o, [0, 0, 0], level, note="the axis rays' origins", on=k)
    for o in ([3, 0, 2], [1.5, -6, 3], [-2, 2.5, -1], [-5, -5, 2], [6, 6, 3], [0, 4, 6], [-6, 3, 2], [-2, 2.5, 0.7]):
        S.add("inside", o, [0, 0, 0], level)
        S.add("inside", o, [0, 0, 0], tilted)
    # ---- graze: the +x ray past the ball (1.5, -6, 3) r 0.8 and past the wall of the cylinder (3, 0, 0) r 1: h2 either side of 0
    # The ray is one of the seeded 16 (GRAZE_RAY of ray_set()) on a level drone, 4.5 m before the object and `t` to the side: no other
    # ray of the set is along it or against it, so the restatement's margin leaves out that ray alone (an axis ray takes its opposite
    # and the two nearly-axis rays with it: a sixth of the lane)
    g_ray = ray_set()[GRAZE_RAY:GRAZE_RAY + 1]
    gd = g_ray[0].astype(np.float64)
    flat = np.array([-gd[1], gd[0], 0.0]) / np.hypot(gd[0], gd[1])
    for obj, aim, side, bracket in ((RS.table()[0], [1.5, -6.0, 3.0], flat, (0.5, 1.1)), (RS.table()[1], [3.0, 0.0, 2.0], flat, (0.7, 1.3)),
                                    (RS.table()[0], [1.5, -6.0, 3.0], np.cross(gd, flat), (0.5, 1.1))):
        def origin(t, aim=aim, side=side):
            return f32(np.asarray(aim) - 4.5 * gd + t * side)

        def hits(o, obj=obj):
            return bool(RY.evaluate(g_ray, RS.MAX_RANGE, [o], [level], [obj])[0, 0] < RS.MAX_RANGE)
        for t in _bisect(origin, hits, *bracket):
            S.add("graze", origin(t), [0, 0, 0], level, note=f"ray {GRAZE_RAY} grazing: hit = {hits(origin(t))}")
    # ---- cull: the distance to a bounding sphere / a gate's centre either side of the cull's threshold (computed as the headers do)
    ball = RS.table()[0].as_row()
    thr = up(np.float32((float(np.float32(ball[4])) + RS.MAX_RANGE) * (1.0 + 2.0e-4) + 1.0e-3))     # fpv_range_bounds: centre exact in fp32
    near = lambda x: bool(np.float32(np.float32(x - np.float32(ball[1])) ** 2) < np.float32(thr * thr))  # noqa: E731
    for x in _bisect_f32(near, ball[1] + 20.0, ball[1] + 22.0):
        S.add("cull", [x, ball[2], ball[3]], [0, 0, 0], f32([0, 0, 0, 1]), note=f"range cull of the ball: near = {near(x)}")   # looks back along -x
    for res in ((8, 8), (12, 8)):
        r = DepthCamera(resolution=res, max_depth=DS.MAX_DEPTH).derive()
        reach = up(np.float32(float(r.max_depth) * float(r.dir_len_max) * (1.0 + 1.0e-4)))
        # the ball's bounding sphere against the CAMERA's origin (fpv_depth.h "Objects": fpv_range_bounds with `reach`): a drone turned
        # half round looks back at the ball from o.x = p.x - rel.x
        othr = up(np.float32((float(np.float32(ball[4])) + float(reach)) * (1.0 + 2.0e-4) + 1.0e-3))
        onear = lambda x: bool(np.float32(np.float32(np.float32(x - rel_x) - np.float32(ball[1])) ** 2) < np.float32(othr * othr))  # noqa: E731
        for x in _bisect_f32(onear, ball[1] + 20.0, ball[1] + 200.0):
            S.add("cull", [x, ball[2], ball[3]], [0, 0, 0], f32([0, 0, 0, 1]), note=f"depth cull of the ball at {res}: near = {onear(x)}")
        g = np.asarray(gate_rows(DS.course(64)))[0]
        fw = np.float32(r.gate_frame_width)
        ext = np.float32(np.float32(g[12] + fw) + np.float32(g[13] + fw))
        gthr = np.float32(np.float32(ext + reach) * np.float32(1.001) + np.float32(1.0e-3))          # (an fmaf on the device: see the host module)
        gnear = lambda z: bool(np.float32(np.float32(z - g[2]) ** 2) < np.float32(gthr * gthr))  # noqa: E731
        for z in _bisect_f32(gnear, g[2] + 20.0, g[2] + 100.0):
            px = down(np.float32(g[0] - rel_x))
            S.add("cull", [px, g[1], z], [0, 0, 0], level, note=f"depth cull of gate 0 at {res}: about the threshold")
    # ---- reach: a hit at exactly max_range / just inside it (the -z axis ray over the ground)
    for z in (RS.MAX_RANGE, down(RS.MAX_RANGE), up(RS.MAX_RANGE), DS.MAX_DEPTH, down(DS.MAX_DEPTH)):
        S.add("reach", [0.5, 0.5, z], [0, 0, 0], level, note=f"ground at {z!r} below")
    # ---- byte: two neighbouring heights over the ground between which the u8 image's pixel (3, 7) changes by one level: 255 (1 - d /
    # max_depth) either side of an integer.  A level drone outside the gate ring, looking away from everything but the ground
    for res in ((8, 8), (12, 8)):
        cam8 = DepthCamera(resolution=res, max_depth=DS.MAX_DEPTH, encoding="u8")

        def level_of(z, cam8=cam8):
            return int(cam8.evaluate([[7.5, -3.0, z]], [level], DS.world(1))[0, 7, 3])
        assert level_of(1.0) > 100 > level_of(20.0)
        for z in _bisect_f32(lambda z: level_of(z) > 100, 1.0, 20.0):
            S.add("byte", [7.5, -3.0, z], [0, 0, 0], level, note=f"{res}: pixel (3, 7) of the u8 image = {level_of(z)}")
    # ---- the laws' extras, each on a pose that faces the target --------------------------------------------------------------------
    yaw30 = rot_zyx(yaw=30.0)
    # the target's centre on the camera origin (czp = 0, 0 / 0), in the camera's plane (czp = +-0, cxp != 0), behind it
    # (rolled half round the camera sees the plane's other side: cxp changes its sign.  czp is +0 in all of them - see `camera_frame`)
    for q, sign in ((level, 1.0), (f32([0, 1, 0, 0]), 1.0), (f32([0, 0, 0, 1]), -1.0)):
        px = np.float32(CENTRE[0] - np.float32(sign) * rel_x)
        cands = [c for c in (px, up(px), down(px), up(up(px)), down(down(px))) if np.float32(c + np.float32(sign) * rel_x) == CENTRE[0]]
        if not cands:                                           # no fp32 p.x puts the origin exactly there at this attitude
            continue
        S.add("origin", [cands[0], CENTRE[1], CENTRE[2]], [1, 0, 0], q, note="target on the camera origin")
        for dy in (3.0, -3.0):
            S.add("origin", [cands[0], CENTRE[1] + np.float32(dy), CENTRE[2]], [1, 0, 0], q, note="target in the camera's plane")
    for depth in (-5.0, -0.5):
        S.add("behind", *_pvq(cam.place(yaw30, (320.0, 240.0), depth)), note="target behind the camera")
    # at max_depth, and on each image border: the neighbouring poses either side of `seen`
    for make, lo, hi, what in ((lambda t: cam.place(yaw30, (320.0, 240.0), t), 14.0, 16.0, "depth about max_depth"),
                               (lambda t: cam.place(yaw30, (t, 240.0), 6.0), -3.0, 3.0, "u about 0"),
                               (lambda t: cam.place(yaw30, (t, 240.0), 6.0), 637.0, 643.0, "u about W"),
                               (lambda t: cam.place(yaw30, (320.0, t), 6.0), -3.0, 3.0, "v about 0"),
                               (lambda t: cam.place(yaw30, (320.0, t), 6.0), 477.0, 483.0, "v about H")):
        for t in _bisect(make, lambda pq: sees(*pq), lo, hi):
            p, q = make(t)
            S.add("border", p, [1.0, 0.5, 0.0], q, note=f"{what}: seen = {sees(p, q)}")
    # first fallback axis.  level: the direction straight up and no velocity (F = m d - g vertical): by the caller's pixel on a level
    # drone, and by a target straight above the camera of a drone pitched nose-up.  frontarget: the target straight below a drone
    # pitched nose-down (tests/test_chase_host.py)
    S.add("fallback1", [0, 0, 5], [0, 0, 0], level, pixel=cam.pixel_of(np.eye(3), [0, 0, 1]), note="level: pixel straight up")
    S.add("fallback1", [1, 2, 6], [0, 0, 0], level, pixel=cam.pixel_of(np.eye(3), [0, 0, 1]), note="level: pixel straight up")
    up_pixel = cam.pixel_of(np.eye(3), [0, 0, 1])
    for k in range(12):                                         # (a lane just off the parallel is ill-conditioned in any precision: the
        S.add("fallback1", [k - 6.0, 2.0 - k, 5.0 + 0.5 * k], [0, 0, 0], level, pixel=up_pixel, note="level: pixel straight up")     # exact ones outnumber them)

    def parallel(t):
        """does the level law take the fallback axis with the pixel t pixels off the zenith (in x and y)?  Its y column is F x (1, 0, 0),
        no x component at all; off the parallel it is F x g, whose x component is F.y g.z"""
        rot = chase.evaluate([[0, 0, 5]], [[0, 0, 0]], [level], (CENTRE, RADIUS), None, [up_pixel + np.float32(t)])[0][0]
        return bool(rot[0, 1] == 0.0)
    lo, hi = _bisect_f32(parallel, 1e-6, 1.0)
    for t, what in ((lo, "the last pixel offset that is parallel"), (hi, "the first that is not")):
        S.add("fallback1", [0, 0, 5], [0, 0, 0], level, pixel=up_pixel + np.float32(t), note=f"near the parallel, level: {what}")
    for pitch in (-20.0, -30.0):
        R = rot_zyx(pitch=pitch)                                # nose up: the camera's view holds the zenith
        q = f32(quat_of(R))
        p = f32(CENTRE.astype(np.float64) - [0.0, 0.0, 5.0] - RS.rot64(q[None])[0] @ L.rel)
        S.add("fallback1", p, [0, 0, 0], q, pixel=cam.pixel_of(R, [0, 0, 1]), note="level: target straight above")
    Rdown = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    qdown = f32([np.cos(np.pi / 4), 0.0, np.sin(np.pi / 4), 0.0])
    for hgt in (5.0, 7.0):
        p = f32(CENTRE.astype(np.float64) + [0.0, 0.0, hgt] - RS.rot64(qdown[None])[0] @ L.rel)
        S.add("fallback1", p, [0, 0, 0], qdown, pixel=cam.pixel_of(Rdown, [0, 0, -1]), note="frontarget: target straight below")
    # second fallback axis: frame = drone with the body pitched 90 degrees (g along the world x axis) and the pixel's direction along
    # x too: F, g and d are all parallel to the first replacement (1, 0, 0).  By the caller's pixel (the view does not hold it)
    for sgn in (1.0, -1.0):
        q = f32([np.cos(np.pi / 4), 0.0, sgn * np.sin(np.pi / 4), 0.0])
        R = RS.rot64(q[None])[0]
        for x in (1.0, -1.0):
            d = L.rr.T @ (R.T @ np.array([x, 0.0, 0.0]))
            if d[2] > 0:
                S.add("fallback2", [0, 0, 5], [0, 0, 0], q, pixel=cam.pixel_of(R, [x, 0, 0]), note=f"drone frame: g and d along {x:+g} x")
                S.add("fallback2", [3, -2, 8], [0, 0, 0], q, pixel=cam.pixel_of(R, [x, 0, 0]), note=f"drone frame: g and d along {x:+g} x")
    # still: facing, no velocity, above tof - with the mass at 1e-30 kg and the multiplier pinned to 0 these lanes have F = 0
    for yaw in (0.0, 100.0, -140.0):
        S.add("still", *_pvq(cam.place(rot_zyx(yaw=yaw), (330.0, 390.0), 5.0), v=[0, 0, 0]), note="F = 0 when the law's mass is 1e-30 and m = 0")
    # limit: point and shoot's thrust limit.  The host tests' lanes, then a host search for each outcome, then the two speeds either
    # side of |F| = Fmax and of the change from the solved root to out of reach
    S.add("limit", [0, 0, 5], [8, 21.25, 0], level, pixel=[320.0, 470.0], action=[0, -0.9, 0, 0], note="limited = 1, solved")
    S.add("limit", [0, 0, 5], [-40, 3, 1], level, pixel=[320.0, 240.0], action=[0, 0.2, 0, 0], note="limited = 2, out of reach")
    S.add("limit", [0, 0, 5], [0, 40, 0], level, pixel=[320.0, 240.0], action=[0, 0, 0, 0], note="limited = 2, negative discriminant")
    fmax = np.float32(P.max_throttle_in_force)

    def outcome(v, pixel, a1, p=(0, 0, 5)):
        o = pns.evaluate([p], [v], [level], pixel=[pixel], action=[0, a1, 0, 0])
        return int(o["limited"][0]), np.float32(o["thrust"][0])
    # the four outcomes: the root taken (thrust = Fmax); the root above max_output and clipped there (|F| below Fmax: the one way to
    # limited = 1 without Fmax - a root below min_output leaves |F| above Fmax and is out of reach); out of reach with a root below
    # min_output; out of reach with a negative discriminant
    found, solved = {"solved": 0, "clipped at max_output": 0, "out of reach, clipped at min_output": 0, "out of reach, negative discriminant": 0}, []
    for _ in range(6000):
        v, pixel, a1 = rng.normal(size=3) * rng.uniform(5, 30), rng.uniform([0, 0], [640, 900]), rng.uniform(-1, 1)
        lim, thrust = outcome(v, pixel, a1)
        disc, root, lo_out, hi_out = cam.limit_terms([0, 0, 5], v, np.eye(3), pixel)
        if abs(disc) < 1e-3 * float(fmax) ** 2 or min(abs(root - lo_out), abs(root - hi_out)) < 1e-3:
            continue                                            # too close to call in float64
        kind = {0: None, 1: "solved" if thrust == fmax else "clipped at max_output" if root > hi_out else None,
                2: "out of reach, negative discriminant" if disc < 0 else "out of reach, clipped at min_output" if root < lo_out else None}[lim]
        if kind and found[kind] < 3:
            found[kind] += 1
            if kind == "solved":
                solved.append((v, pixel, a1))
            S.add("limit", [0, 0, 5], v, level, pixel=pixel, action=[0, a1, 0, 0], note=f"limited = {lim}, {kind}")
        if min(found.values()) >= 3:
            break
    for s in _bisect_f32(lambda s: outcome([0, s, 0], [320.0, 240.0], 0.0)[0] > 0, 1.0, 40.0):
        S.add("limit", [0, 0, 5], [0, s, 0], level, pixel=[320.0, 240.0], action=[0, 0, 0, 0], note="|F| about Fmax")
    edges = 0
    for v, pixel, a1 in solved:                                 # a solved lane, faster and faster until the limit is out of reach
        if outcome(v * 10.0, pixel, a1)[0] == 2:
            for s in _bisect_f32(lambda s: outcome(f32(v) * s, pixel, a1)[0] > 1, 1.0, 10.0):       # noqa: B023
                S.add("limit", [0, 0, 5], f32(v) * s, level, pixel=pixel, action=[0, a1, 0, 0], note="about the change from the solved root to out of reach")
            edges += 1
    assert edges >= 1
    # commands
    F = cam.place(yaw30, (300.0, 380.0), 6.0)                   # over the ground and above the tof height
    for k in range(4):
        for val in (NAN, INF, -INF, 1e30, -1e30, 3e38, -3e38):
            a = f32([0.1, -0.2, 0.05, 0.1])
            a[k] = val
            S.add("command", *_pvq(F), action=a, pixel=[300.0, 220.0], note=f"a{k} = {val!r}")
    a1 = np.float32(100.0 / 240.0 - 1.0)                          # (H / 2)(1 + a1) about the integer 100, and negative
    for val, what in ((a1, "about 100"), (up(a1), "about 100"), (down(a1), "about 100"), (up(up(a1)), "about 100"), (-1.5, "= -120"),
                      (np.float32(-1.0 - 0.5 / 240.0), "about -0.5: truncated toward zero"), (np.float32(-1.0 - 1.75 / 240.0), "about -1.75")):
        S.add("command", *_pvq(F), action=[0.0, val, 0.0, 0.0], pixel=[300.0, 220.0], note=f"(H / 2)(1 + a1) {what}")
    # the caller's pixel
    for pix in ([NAN, 200.0], [300.0, NAN], [INF, 200.0], [300.0, -INF], [1e30, 200.0], [300.0, -1e30], [DENORMAL, DENORMAL], [-0.0, 0.0]):
        S.add("pixel", *_pvq(F), pixel=pix, note=f"pixel = {pix!r}")
    # the rows the caller filled
    fresh = [0.0, 0.0, 0.0, 1.0]
    for row in range(3):
        for val in (NAN, INF, DENORMAL):
            st = f32([0.3, -0.2, 1.5, 0.0])
            st[row] = val
            S.add("rows", *_pvq(F), pid=st, prev=[310.0, 230.0], pixel=[300.0, 220.0], note=f"PID row {row} = {val!r}")
    for val in (2.0, -0.0, NAN):
        S.add("rows", *_pvq(F), pid=[0.3, -0.2, 1.5, val], prev=[310.0, 230.0], pixel=[300.0, 220.0], note=f"IS_FIRST = {val!r}")
    for prev in ([INF, 230.0], [NAN, 230.0], [310.0, NAN], [310.0, -INF]):
        S.add("rows", *_pvq(F), pid=[0.3, -0.2, 1.5, 0.0], prev=prev, pixel=[300.0, 220.0], note=f"prev_pixel = {prev!r}")
    S.add("rows", *_pvq(F), pid=[0.3, -0.2, 1.5, 0.0], prev=[310.0, 230.0], restart=0xFF, pixel=[300.0, 220.0], note="restart byte 0xFF")
    S.add("rows", *_pvq(F), pid=fresh, restart=0xFF, pixel=[NAN, NAN], note="restart byte 0xFF on a lane that is not guided")
    # p.z exactly tof and an ulp below it, v.z = +-0: the lift's two selects
    for z in (tof, down(tof)):
        for vz in (0.0, -0.0):
            p = f32([CENTRE[0] - 3.0, CENTRE[1] - 1.0, z])
            yaw = np.rad2deg(np.arctan2(float(CENTRE[1] - p[1]), float(CENTRE[0] - p[0])))
            S.add("tof", p, [1.0, 0.5, vz], f32(quat_of(rot_zyx(yaw=yaw))), note=f"p.z = {z!r}, v.z = {vz!r}")
    # ---- the pursuit task's words and geometry -------------------------------------------------------------------------------------
    fresh_bit = _lib.FPV_TGT_FRESH
    for count in (K_PATH - 1, (K_PATH - 1) | fresh_bit, K_PATH, 0x1FFFF, 0x1FFFF | fresh_bit, 0x7FFFFFFF, 0):
        S.add("word", *_pvq(F), count=count, path_r=1.5, done=0, note=f"COUNT = {count:#x}")
        S.add("word", *_pvq(F), count=count, path_r=0.0, done=0, note=f"COUNT = {count:#x}, standing")
    inside_target = f32(F[0]) + f32([0.3, 0.0, 0.0])
    for spawns in (0x0000FFFF, 0xFFFF0000, 0xFFFFFFFF):
        S.add("word", *_pvq(F), spawns=spawns, own=inside_target, done=0, note=f"SPAWNS = {spawns:#x} on a lane that captures")
        S.add("word", *_pvq(F), spawns=spawns, own=f32(F[0]) + f32([0.0, 0.3, 0.0]), done=0, note=f"SPAWNS = {spawns:#x} on a lane that captures")
        S.add("word", *_pvq(F), spawns=spawns, done=1, note=f"SPAWNS = {spawns:#x} on a lane that rebases")
        S.add("word", *_pvq(F), spawns=spawns, done=0, note=f"SPAWNS = {spawns:#x} on a lane that does neither")
    for pd in (NAN, INF, -INF):
        S.add("prevdist", *_pvq(F), prev_dist=pd, done=0, note=f"PREV_DIST = {pd!r}")
        S.add("prevdist", *_pvq(F), prev_dist=pd, done=1, note=f"PREV_DIST = {pd!r}, rebasing")
    # dist either side of capture_distance: a standing target beside the drone (dist = offset - radius)
    Fp = f32(F[0])

    def captured(t):
        d = np.float32(np.float32(Fp[0] + t) - Fp[0])
        return bool(np.float32(np.float32(np.sqrt(np.float32(d * d))) - np.float32(RADIUS)) <= np.float32(CAPTURE))
    for t in _bisect_f32(captured, 0.5, 1.0):
        S.add("capture", *_pvq(F), own=[np.float32(Fp[0] + t), Fp[1], Fp[2]], done=0, note=f"dist about capture_distance: captured = {captured(t)}")
    S.freeze()
    if S.n % 64 == 0:
        raise AssertionError("the lane count must not be a multiple of 64")
    assert S.n < 512, S.n
    return S


def _pvq(pq, v=(1.0, 0.5, -0.25)):
    return pq[0], v, pq[1]


# ---- the gate step's own small set -------------------------------------------------------------------------------------------------
GATE_N = 150
_ABI = (pathlib.Path(__file__).resolve().parent.parent / "include" / "fpv_abi.h").read_text()
GATE_MAX_PASSED = int(re.search(r"#define FPV_GATE_MAX_PASSED (0x[0-9a-fA-F]+)u", _ABI).group(1), 16)      # the word's count saturates here


def gate_kinds(n=GATE_N):
    """what lane k of the gate step's set is about: lanes 0..63 own gate k"""
    kinds = np.array(["free"] * n, dtype=object)
    for k in range(64):
        kinds[k] = ("through", "edge", "outside", "start_on_plane", "standing", "through", "edge_z", "outside")[k % 8]
    kinds[64:80] = "garbage"
    return kinds


AXES = (np.eye(3), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]))      # columns n u w: n along +x, n along +y
GATE_SIZE = 1.0                                                 # a = hz = 0.5: exact in fp32


@functools.lru_cache(maxsize=None)
def gate_scene():
    """(params, init [14, ld], acts [3, n, 4], course, words [n] uint32, host states [4, 14, n], physics done [3, n]): lane k < 64 flies
    at 5 m/s along the normal of gate k, and gate k stands where the lane model puts that lane after the first step (gate_kinds:
    through the centre, on the aperture's edge, outside it), or where the lane starts (s0 == 0), or the lane stands still on its
    plane (p_new == p_old); lanes 64..79 hold garbage words; the others fly a flight-like start."""
    n = GATE_N
    p = load_params(fps=1000)
    kinds = gate_kinds(n)
    pos, vel, ypr = (a[:n].copy() for a in gc.starts())
    for k in range(64):
        normal = AXES[k % 2][:, 0]
        vel[k] = 5.0 * normal + [0.0, 0.0, 0.1]
        if kinds[k] == "standing":
            vel[k] = 0.0
    ypr[:64] = 0.0
    acts = np.zeros((3, n, 4), np.float32)
    acts[..., 3] = -0.646                                       # the hover sticks of the chase tests
    acts[:, 80:] = gc.acts(3, n)[:, 80:]
    init = lane_model.initial_state(p, n, pos, vel, ypr)
    s = init.copy()
    states, pdone = np.empty((4, 14, n), np.float32), np.zeros((3, n), bool)
    states[0] = s[:, :n]
    for t in range(3):
        _, _, d, _ = lane_model.run(p, s, acts[t:t + 1], n=n)
        states[t + 1], pdone[t] = s[:, :n], d.astype(bool)
    P0, P1 = states[0, 0:3].T.astype(np.float64), states[1, 0:3].T.astype(np.float64)
    course, half = [], GATE_SIZE / 2
    for k in range(64):
        A = AXES[k % 2]
        u, w = A[:, 1], A[:, 2]
        c = {"through": P1[k], "edge": P1[k] - half * u, "edge_z": P1[k] - half * w, "outside": P1[k] - 2.0 * half * u, "start_on_plane": P0[k],
             "standing": P0[k]}[kinds[k]]
        course.append(Gate(np.float32(c).astype(np.float64), A, GATE_SIZE, "rectangle"))
    words = (np.arange(n) % 64).astype(np.uint32)
    through = [k for k in range(64) if kinds[k] == "through"]
    top = GATE_MAX_PASSED
    for k, extra in zip(through, (0, (top - 1) << 10, top << 10, 63 << 10, 3 << 8, (3 << 8) | (62 << 10), 7 << 10, 0)):
        words[k] |= np.uint32(extra)
    words[64:80] = [0x40, 0xFF, 0xC8, 0x340, 0x3FF, (top << 10) | 0xFF, (63 << 10) | 0x80, 0xFFFFFFFF, 0xFFFFFF00, 0x100, 0x200, 0x300,
                    (top << 10) | 0x300, 0x7F, 0x80000000, 0x1FF]
    return p, init, acts, course, words, states, pdone


def gate_expectation(steps):
    p, init, acts, course, words, states, pdone = gate_scene()
    rows = G.derive(course)
    word, out = words.copy(), []
    for t in range(steps):
        word, r, d, o = G.evaluate(rows, states[t, 0:3].T, states[t + 1, 0:3].T, states[t + 1, 6:10].T, pdone[t], word, laps=1)
        out.append((word.copy(), r, d, o))
    return rows, out


# ---- the host calls both modules make (fpyv_amd's evaluate methods, with room for a change to the derived struct) -------------------
def fzero(s):
    """the struct change of tests/test_pns_host.py::test_zero_force_gives_the_identity_and_zero_thrust: a mass of 1e-30 kg and a
    multiplier pinned to 0, so that a drone without velocity has |F|^2 below 2^-96"""
    s.mass, s.pid.min_output, s.pid.max_output = 1e-30, 0.0, 0.0


def chase_host(G, p, v, q, pid, pixel=None, tweak=None):
    """fpv_chase_eval against the shared target: dict(rotation [n, 9], thrust, pixel [n, 2], visible uint8, pid [4, n] after)"""
    import ctypes as C
    from fpyv_amd.chase import _aligned8
    n = len(p)
    pp, vv, qq = (np.ascontiguousarray(f32(a)) for a in (p, v, q))
    st = np.array(pid, dtype=np.float32, order="C").reshape(4, n)
    s = G.derive((CENTRE, RADIUS))
    if tweak:
        tweak(s)
    rot, thrust, pix_out, vis = np.zeros((n, 9), np.float32), np.zeros(n, np.float32), _aligned8(n), np.zeros(n, np.uint8)
    if pixel is not None:
        pix_in = _aligned8(n)
        pix_in[...] = pixel
        s.pixel = pix_in.ctypes.data
    s.pid_state, s.pid_ld = st.ctypes.data, n
    s.rotation, s.thrust, s.pixel_out, s.visible = rot.ctypes.data, thrust.ctypes.data, pix_out.ctypes.data, vis.ctypes.data
    _lib.check(_lib.lib().fpv_chase_eval(C.byref(s), n, pp.ctypes.data, vv.ctypes.data, qq.ctypes.data))
    return dict(rotation=rot, thrust=thrust, pixel=np.array(pix_out), visible=vis, pid=st)


def pns_host(G, p, v, q, pid, prev, source, own, pixel, action=None, restart=None, tweak=None):
    """fpv_pns_eval: `source` "shared" (CENTRE), "rows" (own [n, 3]) or "pixel" (pixel [n, 2]).  dict(rotation [n, 9], thrust, throttle,
    velocity [n, 2], limited, visible uint8, pid [4, n], prev [2, n] after)"""
    import ctypes as C
    from fpyv_amd.chase import _aligned8
    from fpyv_amd.pns import _aligned16
    n = len(p)
    pp, vv, qq = (np.ascontiguousarray(f32(a)) for a in (p, v, q))
    st, pv = np.array(pid, dtype=np.float32, order="C").reshape(4, n), np.array(prev, dtype=np.float32, order="C").reshape(2, n)
    s = G.derive()
    if tweak:
        tweak(s)
    keep = []
    if source == "shared":
        t = np.ascontiguousarray(CENTRE)
        s.target = t.ctypes.data
        keep.append(t)
    elif source == "rows":
        t = np.ascontiguousarray(f32(own).T)
        s.target_rows, s.target_ld = t.ctypes.data, n
        keep.append(t)
    else:
        pix_in = _aligned8(n)
        pix_in[...] = pixel
        s.pixel = pix_in.ctypes.data
        keep.append(pix_in)
    if action is not None:
        act = _aligned16(n)
        act[...] = action
        s.action = act.ctypes.data
        keep.append(act)
    if restart is not None:
        rs = np.ascontiguousarray(np.asarray(restart, dtype=np.uint8))
        s.restart = rs.ctypes.data
        keep.append(rs)
    rot, thrust, throttle = np.zeros((n, 9), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    vel, lim, vis = _aligned8(n), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    s.pid_state, s.pid_ld, s.prev_pixel, s.prev_pixel_ld = st.ctypes.data, n, pv.ctypes.data, n
    s.rotation, s.thrust, s.throttle = rot.ctypes.data, thrust.ctypes.data, throttle.ctypes.data
    s.pixel_velocity, s.limited, s.visible = vel.ctypes.data, lim.ctypes.data, vis.ctypes.data
    _lib.check(_lib.lib().fpv_pns_eval(C.byref(s), n, pp.ctypes.data, vv.ctypes.data, qq.ctypes.data))
    return dict(rotation=rot, thrust=thrust, throttle=throttle, velocity=np.array(vel), limited=lim, visible=vis, pid=st, prev=pv)


def pursuit_task(guide=None):
    return PT.task(capture_distance=CAPTURE, guide=None if guide is None else dict(ref_frame=guide[0], mode=guide[1], max_depth=MAX_DEPTH))


PURSUIT_NAN_CHANNELS = ("obs", "paid", "reward", "ep", "prev_dist")     # the five channels that may hold an arithmetic NaN


def canonical(a):
    """the words of an fp32 array with every NaN mapped to 0x7fc00000"""
    w = np.ascontiguousarray(f32(a)).view(np.uint32).copy()
    w[np.isnan(f32(a))] = 0x7FC00000
    return w


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)
