"""Same import shape as the reference's `utils.components` for the classes that are on (or feed)
the per-drone step: `from fpyv_amd.components import Drone, Ground, Cylinder, Target, Gate, Trail, PID`.

    reference class (src/utils/components.py)      here
    Drone   :72-248, :258-304, :312-387             fpyv_amd.env.DroneBatch  (N drones per object; `Drone(params)`
                                                    takes the same params dict, plus num_envs= / device=;
                                                    calculate_needed_force_orientation is DESIGN 3.9,
                                                    point_and_shoot(pixel, action, ref_frame, mode) DESIGN 3.11)
    PID     :15-54                                  fpyv_amd.pid.PID         (N controllers per object)
    Ground  :646-683, Cylinder :685-729,            fpyv_amd.objects         (reference constructor signatures;
    Target  :753-778, Gate :780-831, Trail :631-644                           distance + normal only, Gate/Trail inert)

`Racer` (/root/reference/tests/racer_drone_test.py:68-103) maps to fpyv_amd.env.RacerBatch.
`Camera` (:449-629) maps to fpyv_amd.camera.Camera: the reference's constructor signature on the batched depth camera (DESIGN 3.8;
its rendering of point clouds is out of scope).
"""
from .camera import Camera  # noqa: F401
from .env import DroneBatch as Drone, RacerBatch as Racer, FpvVecEnv  # noqa: F401
from .objects import Cylinder, Gate, Ground, Target, Trail  # noqa: F401
from .pid import PID  # noqa: F401

__all__ = ["Drone", "Racer", "FpvVecEnv", "Ground", "Cylinder", "Target", "Gate", "Trail", "PID", "Camera"]
