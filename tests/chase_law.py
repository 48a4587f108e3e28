"""The target chase in float64 NumPy, written from its definition (csrc/fpv_chase.h) - the restatement the g18 captures
of the reference pin (tests/test_chase_host.py) and the yardstick of the fp32 host function and of the closed-loop tests.  One drone
per call; nothing here is used by the product."""
import numpy as np

PARALLEL = 1.0e-12


class Law:
    """The uniform inputs: camera (focal length, W, H, rel_rot, rel_pos), the five constants, the mass and the PID's constants"""

    def __init__(self, focal, width, height, rel_rot, rel_pos, mass, vdrag, vlift, tof, keep, uwb, pid, max_depth=15.0):
        self.f, self.w, self.h = float(focal), float(width), float(height)
        self.rr, self.rel = np.asarray(rel_rot, dtype=np.float64).reshape(3, 3), np.asarray(rel_pos, dtype=np.float64).reshape(3)
        self.g = np.array([0.0, 0.0, -9.81 * float(mass)])
        self.vdrag, self.vlift, self.tof, self.keep, self.uwb, self.max_depth = vdrag, vlift, tof, keep, uwb, float(max_depth)
        self.kP, self.kI, self.kD, self.dt, self.iclip, self.lo, self.hi, self.drate = (float(x) for x in pid)

    @classmethod
    def from_golden(cls, g):
        return cls(g["focal_length"], g["camera_resolution"][0], g["camera_resolution"][1], g["relative_rotation"], g["camera_position"],
                   g["mass"], float(g["virtual_drag_coefficient"]), float(g["virtual_lift_coefficient"]), float(g["tof_effective_distance"]),
                   float(g["keep_distance"]), float(g["UWB_sensor_max_range"]), g["pid_gains"], float(g["max_depth"]))

    @classmethod
    def from_params(cls, p, max_depth=15.0):
        """from a DroneParams, the camera derived as DESIGN 3.8 does"""
        c, law, k = p.camera, p.point_and_shoot, dict(p.force_multiplier_pid)
        w, h = c["resolution"]
        f = w / (2.0 * np.tan(np.deg2rad(c["fov"]) / 2.0))
        s, cs = np.sin(np.deg2rad(c["camera_angle"])), np.cos(np.deg2rad(c["camera_angle"]))
        return cls(f, w, h, [[0.0, s, cs], [1.0, 0.0, 0.0], [0.0, -cs, s]], c["position_relative_to_frame"], p.mass,
                   law["virtual_drag_coefficient"], law["virtual_lift_coefficient"], law["tof_effective_distance"], p.keep_distance,
                   p.UWB_sensor_max_range, [k["kP"], k["kI"], k["kD"], p.dt, k["integral_clip"], p.min_throttle_in_force,
                                            p.max_throttle_in_force, k["derivative_transition_rate"]], max_depth)

    def project(self, p, R, c):
        """(pixel (x, y), depth, seen) of the target's centre c"""
        o = p + R @ self.rel
        pc = self.rr.T @ (R.T @ (c - o))
        with np.errstate(all="ignore"):
            u, v = self.f * pc[0] / pc[2] + self.w / 2, self.f * pc[1] / pc[2] + self.h / 2
        seen = bool(pc[2] > 0 and pc[2] <= self.max_depth and 0 <= u < self.w and 0 <= v < self.h)
        return np.array([u, v]), pc[2], seen

    def pid(self, st, current):
        """components.PID.__call__(current, keep_distance) on st = [integral, prev_derivative, previous_error, is_first]"""
        integ, dflt, last, first = st
        err = current - self.keep
        integ = np.clip(0.99 * integ + err * self.dt, -self.iclip, self.iclip)
        d = np.clip(0.0 if first else (err - last) / self.dt, -1.0, 1.0)
        d = (1.0 - self.drate) * dflt + self.drate * d
        return np.clip(self.kP * err + self.kI * integ + self.kD * d, self.lo, self.hi), np.array([integ, d, err, 0.0])

    def __call__(self, p, v, R, c, r, st, pixel=None, frame="world", mode="level"):
        """-> (rotation [3, 3], thrust, pixel [2], seen, PID state after).  Not seen: identity, NaN, NaN pixel, the state as given."""
        p, v, R, c = (np.asarray(x, dtype=np.float64) for x in (p, v, R, c))
        st = np.asarray(st, dtype=np.float64)
        if pixel is None:
            pixel, _, seen = self.project(p, R, c)
        else:
            pixel = np.asarray(pixel, dtype=np.float64)
            seen = not np.any(np.isnan(pixel))
        if not seen:
            return np.eye(3), np.nan, np.full(2, np.nan), False, st
        d = R @ (self.rr @ np.array([(pixel[0] - self.w / 2) / self.f, (pixel[1] - self.h / 2) / self.f, 1.0]))
        d = d / np.linalg.norm(d)
        g, w = (R @ self.g, R @ v) if frame == "drone" else (self.g, v)
        s = np.linalg.norm(v)
        drag = np.zeros(3) if s == 0.0 else self.vdrag * (-(w @ d / s - 1.0) / 2.0) * (-w) * s
        lift = float(p[2] < self.tof) * -(self.tof - p[2]) * self.vlift * g * (1.0 + abs(v[2]))
        dist = min(np.linalg.norm(p - c) - r, self.uwb)
        m, st = self.pid(st, dist)
        F = np.clip(m, self.lo, self.hi) * d + drag + lift - g
        ff = F @ F
        if ff == 0.0:
            return np.eye(3), 0.0, pixel, True, st
        b = g if mode == "level" else d
        y = np.cross(F, b)
        if not y @ y > PARALLEL * ff * (b @ b):
            y = np.cross(F, [1.0, 0.0, 0.0])
            if not y @ y > PARALLEL * ff:
                y = np.cross(F, [0.0, 1.0, 0.0])
        x = np.cross(y, F)
        rot = np.stack([x / np.linalg.norm(x), y / np.linalg.norm(y), F / np.sqrt(ff)], axis=1)
        return rot, float(np.sqrt(ff)), pixel, True, st


def quat_of(R):
    """unit quaternion (wxyz) of a rotation matrix, float64 (the largest-component branch of Shepperd's method)"""
    R = np.asarray(R, dtype=np.float64)
    t = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(t))
    if k == 0:
        q = np.array([t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], t[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], t[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], t[3]])
    return q / np.linalg.norm(q)


# ---- the closed loop of tests/test_gpu_chase.py: a target that flies away along its circle, drones that start behind it -------
CHASE_TARGET = dict(position=[0.0, 0.0, 3.0], radius=0.5, path=dict(radius=25.0, resolution=55000))   # 0.71 m/s at fps = 250
HOVER_STICKS = np.array([0.0, 0.0, 0.0, -0.646])


def chase_starts(n, seed=5):
    """(position [n, 3], ypr_deg [n, 3]) float32: 8..11 m behind the first point of the target's path - it moves along +y -, 2.5..6 m
    up, the nose within 15 degrees of the target: the camera sees it at the start"""
    rng = np.random.default_rng(seed)
    t0 = np.array([25.0, 0.0, 3.0])
    phi = np.deg2rad(rng.uniform(-130.0, -50.0, n))
    rho = rng.uniform(8.0, 11.0, n)
    p = t0 + np.stack([rho * np.cos(phi), rho * np.sin(phi), rng.uniform(-0.5, 3.0, n)], axis=1)
    ypr = np.stack([np.zeros(n), np.zeros(n), np.rad2deg(phi) + 180.0 + rng.uniform(-15.0, 15.0, n)], axis=1)
    return p.astype(np.float32), ypr.astype(np.float32)
