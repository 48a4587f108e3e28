"""The pursuit task in float64 NumPy, written from its definition (csrc/fpv_pursuit.h) - the restatement the g20 capture of
the reference pins (tests/test_pursuit_host.py) and the yardstick of the fp32 host function - and the seeded scene the host and GPU
tests share.  Nothing here is used by the product."""
import functools

import numpy as np

from oracle import philox

TAG = 0x54475254                    # "TRGT": word 3 of the respawn draw's counter
EPS = 2.0 ** -24                    # half an ulp of 1: one fp32 rounding, relative


def circle64(k):
    """the reference's path angles (helper_functions.py:152): (cos, sin) [K, 2] float64"""
    theta = np.linspace(0, 2 * np.pi, k + 1)[:-1]
    return np.stack([np.cos(theta), np.sin(theta)], axis=1)


def rot64(q):
    """R(q) [n, 3, 3] in float64 from fp32 quaternions (wxyz), the algebraic form the stepper uses everywhere"""
    w, x, y, z = (np.asarray(q, dtype=np.float64)[:, k] for k in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def words(seed, gid, index):
    """the two Philox4x32-7 blocks of a respawn draw, [2, 4] uint32 (arrays with a leading axis: NumPy scalars warn on the wrap)"""
    key = np.array([[seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]], dtype=np.uint32)
    return np.stack([philox.philox4x32(np.array([[gid & 0xFFFFFFFF, ((gid >> 32) & 0xFFFFFFFF) ^ (b << 28), index, TAG]], dtype=np.uint32),
                                       key, rounds=7)[0] for b in (0, 1)])


def draw64(seed, gid, index, lo, hi, rlo, rhi, k):
    """the respawn draw of (seed, global id, respawn index) built on oracle/philox.py: centre [3], radius, path index.  lo and the
    span hi - lo are the fp32 numbers the library narrows them to (the box is an input); the arithmetic on them is float64."""
    w = words(seed, gid, index)
    u = (w[0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    lo4 = np.float32(list(lo) + [rlo]).astype(np.float64)
    span = np.float32(np.array(list(hi) + [rhi], dtype=np.float64) - np.array(list(lo) + [rlo], dtype=np.float64)).astype(np.float64)
    x = lo4 + span * u
    return x[:3], float(x[3]), int((int(w[1][0]) * k) >> 32)


class Restated:
    """n drones' targets and what a call does to them, float64.  `task` is a fpyv_amd.pursuit.PursuitTask (its constants only)."""

    def __init__(self, task, rows, n, dt, drone_id_offset=0):
        r = np.asarray(rows)[:, :n]
        self.task, self.n, self.dt, self.gid0 = task, n, float(dt), int(drone_id_offset)
        self.k = task.resolution
        self.circle = circle64(self.k)
        self.centre = r[0:3].T.astype(np.float64)
        self.path_r, self.radius, self.prev = (r[j].astype(np.float64) for j in (3, 4, 5))
        words = np.ascontiguousarray(r[6:8]).view(np.uint32)
        self.index = (words[0] & 0x1FFFF).astype(np.int64)
        self.fresh = (words[0] >> 31).astype(bool)
        self.respawns, self.captures = (words[1] & 0xFFFF).astype(np.int64), (words[1] >> 16).astype(np.int64)
        self.tol_prev = np.zeros(n)

    def where(self, index):
        c = self.circle[index]
        return self.centre + np.stack([self.path_r * c[:, 0], self.path_r * c[:, 1], np.zeros(self.n)], axis=1)

    def next_position(self):
        """where the next advancing call puts every target"""
        return self.where(self.index)

    def measure(self, p, advance=True):
        """(dist, tol_dist) the next call would measure at the poses p, before any respawn; changes nothing"""
        at = np.where(advance | self.fresh, self.index, (self.index - 1) % self.k)
        p = np.asarray(p, dtype=np.float64)
        m = 2 * np.abs(self.centre).sum(1) + 2 * self.path_r + np.abs(p).sum(1) + 2 * self.radius
        return np.linalg.norm(self.where(at) - p, axis=1) - self.radius, 16 * EPS * m

    def count_words(self):
        return (self.index.astype(np.uint32) | (self.fresh.astype(np.uint32) << np.uint32(31))).astype(np.uint32)

    def spawn_words(self):
        return (self.respawns | (self.captures << 16)).astype(np.uint32)

    def call(self, p, v, q, done=None, reset=False, advance=True):
        """One call.  Returns a dict: paid, event, obs [7, n], position [3, n], measured [n] (dist before any respawn), active [n]
        (False: a reset call left the lane alone) and the bounds of a correct fp32 evaluation: tol_dist, tol_paid, tol_w, tol_v (module docstring of test_pursuit_host.py)."""
        t = self.task
        p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
        flag = np.ones(self.n, bool) if (done is None and reset) else (np.zeros(self.n, bool) if done is None else np.asarray(done).astype(bool))
        active = flag if reset else np.ones(self.n, bool)
        rebase = flag if not reset else flag.copy()
        before = (self.index - 1) % self.k
        at = np.where(advance | self.fresh, self.index, before)
        pos = self.where(at)
        vel = np.zeros((self.n, 3))
        if advance:
            moving = ~self.fresh
            vel[moving] = ((pos - self.where(before)) / self.dt)[moving]
        new_index = np.where(advance, (self.index + 1) % self.k, self.index)
        new_fresh = self.fresh & (not advance)
        w = pos - p
        dist = np.linalg.norm(w, axis=1) - self.radius
        captured = ~rebase & (dist <= t.capture_distance)
        paid = np.where(rebase, 0.0, t.progress * (self.prev - dist)) + np.where(captured, t.capture, 0.0)
        respawn = captured | (rebase & t.respawn_on_done)
        measured = dist.copy()                          # (a respawn replaces dist by the distance to the new target)
        centre, radius = self.centre.copy(), self.radius.copy()
        respawns = self.respawns.copy()
        captures = np.where(rebase, 0, self.captures) + captured
        for i in np.nonzero(respawn & active)[0]:
            c, r, j = draw64(t.spawn_seed, self.gid0 + int(i), int(self.respawns[i]), t.spawn_lo, t.spawn_hi, t.radius_lo, t.radius_hi, self.k)
            centre[i], radius[i], new_index[i], new_fresh[i] = c, r, j, True
            respawns[i] = (respawns[i] + 1) & 0xFFFF
            cs = self.circle[j]
            pos[i] = c + self.path_r[i] * np.array([cs[0], cs[1], 0.0])
            vel[i] = 0.0
            w[i] = pos[i] - p[i]
            dist[i] = np.linalg.norm(w[i]) - r
        R = rot64(q)
        obs = np.concatenate([np.einsum("nji,nj->ni", R, w), np.einsum("nji,nj->ni", R, vel - v), dist[:, None]], axis=1).T
        # what one correct fp32 evaluation may differ by (test_pursuit_host.py has the derivation)
        m = np.abs(centre).sum(1) + np.abs(self.centre).sum(1) + 2 * self.path_r + np.abs(p).sum(1) + radius + self.radius
        tol_dist = 16 * EPS * m
        tol_paid = abs(t.progress) * (tol_dist + self.tol_prev) + 4 * EPS * (np.abs(paid) + abs(t.capture))
        tol_v = 3 * (8 * EPS * m / self.dt) + 16 * EPS * (np.abs(vel).sum(1) + np.abs(v).sum(1))
        out = dict(paid=paid, event=captured.astype(np.uint8), obs=obs, position=pos.T.copy(), active=active, rebase=rebase, measured=measured,
                   tol_dist=tol_dist, tol_paid=tol_paid, tol_w=2 * tol_dist, tol_v=tol_v, respawned=respawn & active)
        a = active
        self.centre[a], self.radius[a], self.prev[a] = centre[a], radius[a], dist[a]
        self.index[a], self.fresh[a], self.respawns[a], self.captures[a] = new_index[a], new_fresh[a], respawns[a], captures[a]
        self.tol_prev[a] = tol_dist[a]
        return out


# ---- the scene of H2 / G1: 257 drones, 40 calls ----------------------------------------------------------------------------------
N, CALLS, DT = 257, 40, 1.0 / 250.0
TASK_KW = dict(path=dict(radius=2.0, resolution=29), capture_distance=0.25, rewards=dict(progress=1.5, capture=7.0),
               respawn=dict(lo=(-6.0, -6.0, 1.0), hi=(6.0, 6.0, 5.0), radius=(0.3, 0.8), seed=0x5EED0020D00D), respawn_on_done=True)
TWICE = (5, 70, 200)                # lanes steered onto their new target right after a capture: captures on consecutive calls
EXACT, EXACT_CALL = 9, 3            # lane whose dist is exactly capture_distance in call 3


def task(**kw):
    from fpyv_amd.pursuit import PursuitTask
    return PursuitTask(**{**TASK_KW, **kw})


def start_targets(n=N, seed=20):
    """dict of arrays for PursuitTask(targets=): centres in the spawn box, a third of the targets standing still; the first n of the
    257 (the same targets whatever n)"""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(-6, 6, N), rng.uniform(-6, 6, N), rng.uniform(1, 5, N)], axis=1).astype(np.float32)
    path_r = np.where(np.arange(N) % 3 == 0, 0.0, rng.uniform(0.5, 4.0, N)).astype(np.float32)
    radius = rng.uniform(0.3, 0.8, N).astype(np.float32)
    phase = rng.integers(0, TASK_KW["path"]["resolution"], N)
    centre[EXACT], path_r[EXACT], radius[EXACT] = (1.0, 2.0, 3.0), 0.0, 0.5
    return dict(centre=centre[:n], radius=radius[:n], path_radius=path_r[:n], phase=phase[:n])


@functools.lru_cache(maxsize=None)
def scene(n=N, calls=CALLS, seed=20):
    """The poses and done bytes of `calls` calls for the first n lanes of the 257-drone scene, built against the float64 restatement.
    Call 0 is the reset call: its `done` row is the mask, every lane but EXACT (whose target stays the one it was given).  Every
    drone flies 35 % of the way to where its target will be, plus noise; about 3 % of the lanes are done in a call; the TWICE lanes
    jump onto their new target after a capture; the EXACT lane sits 0.75 m beside its 0.5 m target in call 3, so that its dist is
    exactly capture_distance in fp32 and in float64.  A drone whose dist would be within fp32 rounding of capture_distance (4 x the
    bound of one evaluation) is moved a centimetre along x until it is not: no event of the scene depends on a rounding.
    Returns (p [calls, n, 3], v, q [calls, n, 4], done [calls, n] uint8, stats) - float32, read-only.  The lanes of a smaller n are
    the first lanes of the full scene, bit for bit (the scene is always built at 257)."""
    if n != N:
        p, v, q, done, stats = scene(N, calls, seed)
        return p[:, :n], v[:, :n], q[:, :n], done[:, :n], stats
    rng = np.random.default_rng(seed)
    t = task(targets=start_targets())
    model = Restated(t, t.rows(N), N, DT)
    P, V, Q, D = (np.zeros((calls, N, k), dtype=np.float32) for k in (3, 3, 4, 1))
    p = np.stack([rng.uniform(-8, 8, N), rng.uniform(-8, 8, N), rng.uniform(0.5, 6, N)], axis=1).astype(np.float32)
    p[EXACT] = (9.0, 9.0, 7.0)
    stats = dict(captures=0, rebases=0, twice=0, exact=0, near_threshold=0)
    last_event = np.zeros(N, bool)
    for c in range(calls):
        qq = rng.normal(size=(N, 4))
        Q[c] = (qq / np.linalg.norm(qq, axis=1, keepdims=True)).astype(np.float32)
        V[c] = rng.normal(size=(N, 3)).astype(np.float32) * 3.0
        done = (rng.uniform(size=N) < 0.03) & (c > 0)
        done[EXACT] = False
        done[list(TWICE)] = False
        if c > 0:
            goal = model.next_position()
            step = p.astype(np.float64) + 0.35 * (goal - p) + rng.normal(size=(N, 3)) * 0.05
            for i in TWICE:
                if last_event[i]:
                    step[i] = goal[i]
            step[EXACT] = (1.75, 2.0, 3.0) if c == EXACT_CALL else (9.0, 9.0, 7.0)
            p = step.astype(np.float32)
            for _ in range(100):
                dist, tol = model.measure(p)
                close = (np.abs(dist - t.capture_distance) <= 8 * tol) & ~done
                close[EXACT] = False
                if not close.any():
                    break
                p[close, 0] += np.float32(0.01)
        else:
            done = np.arange(N) != EXACT
        P[c], D[c, :, 0] = p, done
        out = model.call(P[c], V[c], Q[c], done=done, reset=c == 0)
        ev = out["event"].astype(bool)
        stats["captures"] += int(ev.sum())
        stats["rebases"] += int(done.sum()) if c > 0 else 0
        stats["twice"] += int((ev & last_event).sum())
        gap = np.abs(out["measured"] - t.capture_distance)
        if c > 0:
            stats["exact"] += int((out["measured"][~done] == t.capture_distance).sum())
            undecided = (gap <= 4 * out["tol_dist"]) & ~done
            undecided[EXACT] &= c != EXACT_CALL
            stats["near_threshold"] += int(undecided.sum())
        last_event = ev
    for a in (P, V, Q, D):
        a.setflags(write=False)
    return P, V, Q, D[:, :, 0].astype(np.uint8), stats


# ---- the closed loop of G4: 64 drones, each guided towards a target of its own -------------------------------------------------------
LOOP_N, LOOP_SEEN, LOOP_STEPS, LOOP_FPS = 64, 16, 200, 250
LOOP_TASK_KW = dict(path=dict(radius=25.0, resolution=55000), capture_distance=7.88, rewards=dict(progress=1.0, capture=10.0),
                    respawn=dict(lo=(-30.0, -30.0, 2.0), hi=(30.0, 30.0, 8.0), radius=(0.5, 0.5), seed=4), respawn_on_done=False,
                    guide=dict(ref_frame="world", mode="level", max_depth=15.0))
HOVER_STICKS = np.array([0.0, 0.0, 0.0, -0.646])


def loop_scene(seed=6):
    """(targets dict, position [64, 3], ypr_deg [64, 3]) float32.  Every drone has a 0.5 m target of its own on a 25 m circle around a
    centre of its own; it starts 8.5 m from the first point of that path (dist = 8 m: inside the 13 m UWB range, beyond the 6 m
    keep_distance).  The first LOOP_SEEN drones look at their target within 15 degrees of yaw - the camera sees it -, the others look
    away and are never guided.  200 steps at 250 fps are 0.8 s: a guided drone closes in by 8 to 18 cm (float64 oracle); with
    capture_distance = 7.88 m the quicker ones capture and the others end nearer than they started."""
    rng = np.random.default_rng(seed)
    n = LOOP_N
    centre = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(3.0, 5.0, n)], axis=1).astype(np.float32)
    t0 = centre.astype(np.float64) + np.array([25.0, 0.0, 0.0])
    phi = np.deg2rad(rng.uniform(-130.0, -50.0, n))
    dz = rng.uniform(-0.5, 2.0, n)
    rho = np.sqrt(8.5 ** 2 - dz ** 2)
    p = t0 + np.stack([rho * np.cos(phi), rho * np.sin(phi), dz], axis=1)
    yaw = np.rad2deg(phi) + 180.0 + rng.uniform(-15.0, 15.0, n)
    yaw[LOOP_SEEN:] += 180.0
    ypr = np.stack([np.zeros(n), np.zeros(n), yaw], axis=1)
    targets = dict(centre=centre, radius=np.full(n, 0.5, dtype=np.float32), path_radius=np.full(n, 25.0, dtype=np.float32),
                   phase=np.zeros(n, dtype=np.int64))
    return targets, p.astype(np.float32), ypr.astype(np.float32)
