"""The eight airframes of the per-drone physics tests (tests/test_physics_host.py, tests/test_gpu_physics.py): the packaged
defaults, the four other motor blocks of the G14 captures (their mass, thrust cubic, drag and low-pass rates on the base's
uniform parameters - dt, max_rates and the geometry are not per drone), and three with mass, drag and the lags moved."""
import numpy as np

from conftest import load_golden, params_for_golden
from fpyv_amd import _lib

PER_DRONE = ("mass", "thrust_poly", "drag_coefficients", "rates_transition_rate", "thrust_transition_rate")


def parameter_sets(base):
    sets = [base]
    for k in range(4):
        g = params_for_golden(load_golden(f"g14_drone_type_{k}"))
        sets.append(base.replace(**{f: getattr(g, f) for f in PER_DRONE}))
    sets.append(base.replace(mass=base.mass * 1.3, drag_coefficients=np.array([2.4, 1.1, 0.7])))
    sets.append(base.replace(mass=base.mass * 0.7, rates_transition_rate=0.25, thrust_transition_rate=0.9))
    sets.append(base.replace(drag_coefficients=np.array([0.9, 2.7, 1.9]), rates_transition_rate=0.95, thrust_transition_rate=0.15,
                             thrust_poly=base.thrust_poly * 1.2))
    return sets


def inputs_of(p):
    """[FPV_PHYS_INPUTS] float64: the parameter set of DroneParams `p` as fpv_physics_derive reads it"""
    return np.array([p.mass, *p.thrust_poly, *p.drag_coefficients, p.rates_transition_rate, p.thrust_transition_rate], dtype=np.float64)


def dealt(sets, n):
    """(set index of every drone - round-robin -, [n, FPV_PHYS_INPUTS] inputs)"""
    which = np.arange(n) % len(sets)
    return which, np.stack([inputs_of(sets[k]) for k in which])


assert len(PER_DRONE) == 5 and _lib.FPV_PHYS_INPUTS == 10
