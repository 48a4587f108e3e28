"""Point and shoot in float64 NumPy, written from its definition (csrc/fpv_pns.h) - the restatement the g21 captures of
the reference pin (tests/test_pns_host.py) and the yardstick of the fp32 host function.  One drone per call; nothing here is used by
the product."""
import numpy as np

from chase_law import PARALLEL, Law


class PnsLaw(Law):
    """The chase's uniform inputs (its keep_distance and UWB range are not read) with the thrust limit and the inverse polynomial"""

    def __init__(self, *a, fmax, inv, **kw):
        super().__init__(*a, **kw)
        self.fmax, self.inv = float(fmax), np.asarray(inv, dtype=np.float64)

    @classmethod
    def from_golden(cls, g):
        return cls(g["focal_length"], g["camera_resolution"][0], g["camera_resolution"][1], g["relative_rotation"], g["camera_position"],
                   g["mass"], float(g["virtual_drag_coefficient"]), float(g["virtual_lift_coefficient"]), float(g["tof_effective_distance"]),
                   float(g["keep_distance"]), float(g["UWB_sensor_max_range"]), g["pid_gains"], float(g["max_depth"]),
                   fmax=g["max_throttle_in_force"], inv=g["thrust2throttle_poly"])

    @classmethod
    def from_params(cls, p, max_depth=15.0):
        base = Law.from_params(p, max_depth)
        return cls(base.f, base.w, base.h, base.rr, base.rel, p.mass, base.vdrag, base.vlift, base.tof, base.keep, base.uwb,
                   [base.kP, base.kI, base.kD, base.dt, base.iclip, base.lo, base.hi, base.drate], max_depth,
                   fmax=p.max_throttle_in_force, inv=p.thrust2throttle_poly)

    def throttle(self, thrust):
        return float(np.clip(np.polyval(self.inv, thrust) / 100.0 * 2.0 - 1.0, -1.0, 1.0))

    def __call__(self, p, v, R, action, st, prev, pixel=None, target=None, frame="world", mode="level", restart=False):
        """-> dict(rot [3, 3], thrust, throttle, velocity [2], limited, seen, guided, pid [4], prev [2]).  st = [integral,
        prev_derivative, previous_error, is_first], prev = prev_pixel (NaN = None).  Not guided: identity, NaN, the rows as given."""
        p, v, R = (np.asarray(x, dtype=np.float64) for x in (p, v, R))
        st, prev = np.array(st, dtype=np.float64), np.array(prev, dtype=np.float64)
        a = np.zeros(4) if action is None else np.asarray(action, dtype=np.float64)
        if restart:
            st, prev = np.array([0.0, 0.0, 0.0, 1.0]), np.full(2, np.nan)
        if pixel is None:
            pixel, _, seen = self.project(p, R, np.asarray(target, dtype=np.float64))
        else:
            pixel = np.asarray(pixel, dtype=np.float64)
            seen = not np.any(np.isnan(pixel))
        seen = bool(seen and np.all(np.isfinite(a)))
        off = dict(rot=np.eye(3), thrust=np.nan, throttle=np.nan, velocity=np.full(2, np.nan), limited=0, seen=seen, guided=False, pid=st, prev=prev)
        if not seen:
            return off
        pixel = pixel + a[2:] * np.array([self.w / 2, self.h / 2])
        want = float(np.trunc(self.h / 2 * (1.0 + a[1])))
        velocity = np.zeros(2) if np.any(np.isnan(prev)) else (pixel - prev) / self.dt
        d = R @ (self.rr @ np.array([(pixel[0] - self.w / 2) / self.f, (pixel[1] - self.h / 2) / self.f, 1.0]))
        d = d / np.linalg.norm(d)
        g, w = (R @ self.g, R @ v) if frame == "drone" else (self.g, v)
        s = np.linalg.norm(v)
        drag = np.zeros(3) if s == 0.0 else self.vdrag * (-(w @ d / s - 1.0) / 2.0) * (-w) * s
        lift = float(p[2] < self.tof) * -(self.tof - p[2]) * self.vlift * g * -min(v[2], 0.0)
        self.keep = want                                                    # the PID's target of this call
        m, pid = self.pid(st, pixel[1])
        B = drag + lift - g
        F = m * d + B
        thrust, limited = np.linalg.norm(F), 0
        if thrust > self.fmax:
            b = d @ B
            disc = b * b - B @ B + self.fmax ** 2
            r = (np.sqrt(disc) if disc >= 0 else 0.0) - b
            m = float(np.clip(r, self.lo, self.hi))
            F = m * d + B
            solved = disc >= 0 and m == r
            thrust, limited = (self.fmax if solved else np.linalg.norm(F)), 1
            if not disc >= 0 or (not solved and np.linalg.norm(F) > self.fmax):
                F = self.lo * d + B
                thrust, limited = self.fmax, 2
        ff = F @ F
        if ff == 0.0:
            rot = np.eye(3)
        else:
            b = g if mode == "level" else d
            y = np.cross(F, b)
            if not y @ y > PARALLEL * ff * (b @ b):
                y = np.cross(F, [1.0, 0.0, 0.0])
                if not y @ y > PARALLEL * ff:
                    y = np.cross(F, [0.0, 1.0, 0.0])
            x = np.cross(y, F)
            rot = np.stack([x / np.linalg.norm(x), y / np.linalg.norm(y), F / np.sqrt(ff)], axis=1)
        if not (np.all(np.isfinite(rot)) and np.isfinite(thrust) and np.all(np.isfinite(velocity))):
            return off
        return dict(rot=rot, thrust=float(thrust), throttle=self.throttle(thrust), velocity=velocity, limited=limited, seen=True, guided=True,
                    pid=pid, prev=pixel)
