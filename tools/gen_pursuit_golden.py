#!/usr/bin/env python3
"""Writes tests/golden/g20_targets.npz: captures of the reference's own Target, CircularPath and generate_targets
(src/utils/components.py:743-774, src/utils/generators.py:21-24), float64, for tests/test_pursuit_host.py.

The reference is IMPORTED (oracle.gen_golden.import_reference: its pure-Python classes with the display modules stubbed) and run;
nothing of it is copied.  Needs the reference checkout oracle/gen_golden.py names; the committed .npz file is what the tests read.

  8 targets whose inputs (centre, radius, path radius) are rounded through float32:
    0..3   the default path (radius 25, resolution 5500), 64 updates each; their centres and radii are what generate_targets makes of
           the `simulator.targets` section of the reference's params.yaml (count 4) after np.random.seed(20)
    4 5 6  resolutions 1, 2 and 7 (path radius 3, 1.5, 40), 2 K + 3 updates each: the wrap-around of the path index is in it
    7      a target without a path: it stands still (no update: the reference has none to make)
  Every update records the position; after every update Target.calculate_distance is recorded for 16 seeded points.  The arrays are
  padded to the longest run (64) with NaN (the points are stored as the float32 they are); `updates` holds each target's count.
  `generated_*` hold generate_targets' raw output, `section_*` the section it was given.
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, REPO)
from oracle.gen_golden import import_reference, ref_params  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SEED = 20
POINTS = 16
DEFAULT_UPDATES = 64
SMALL = [(1, 3.0), (2, 1.5), (7, 40.0)]              # (resolution, path radius)


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def main():
    yaml_helper, _, _, _ = import_reference()
    from utils.components import Target
    from utils.generators import generate_targets
    section = dict(ref_params(yaml_helper, 250)["simulator"]["targets"])
    section["count"] = 4
    np.random.seed(SEED)
    made = generate_targets(**section)
    rng = np.random.default_rng(SEED)
    centre = [f32(t.position) for t in made]
    radius = [float(f32(t.radius)) for t in made]
    path_r = [float(section["path"]["radius"])] * 4
    res = [int(section["path"]["resolution"])] * 4
    updates = [DEFAULT_UPDATES] * 4
    for k, r in SMALL:
        centre.append(f32(rng.uniform(-20, 20, 3))); radius.append(float(f32(rng.uniform(0.2, 1.5))))
        path_r.append(float(f32(r))); res.append(k); updates.append(2 * k + 3)
    centre.append(f32(rng.uniform(-20, 20, 3))); radius.append(float(f32(rng.uniform(0.2, 1.5)))); path_r.append(0.0); res.append(0); updates.append(1)
    n, longest = len(centre), max(updates)
    position = np.full((n, longest, 3), np.nan)
    points = np.full((n, longest, POINTS, 3), np.nan)
    distance = np.full((n, longest, POINTS), np.nan)
    for i in range(n):
        has_path = res[i] > 0
        t = Target(centre[i].copy(), radius[i], 1, path=dict(radius=path_r[i], resolution=res[i]) if has_path else None)
        for k in range(updates[i]):
            if has_path:
                t.update()
            position[i, k] = np.asarray(t.position, dtype=np.float64)
            pts = f32(position[i, k] + rng.normal(size=(POINTS, 3)) * rng.uniform(0.5, 30.0, size=(POINTS, 1)))
            points[i, k] = pts
            distance[i, k] = [t.calculate_distance(p) for p in pts]
    np.savez_compressed(os.path.join(OUT, "g20_targets.npz"), centre=np.array(centre), radius=np.array(radius), path_radius=np.array(path_r),
                        resolution=np.array(res, dtype=np.int64), updates=np.array(updates, dtype=np.int64), position=position,
                        points=points.astype(np.float32), distance=distance, seed=np.int64(SEED),
                        generated_centre=np.array([np.asarray(t.position, dtype=np.float64) for t in made]),
                        generated_radius=np.array([float(t.radius) for t in made]),
                        section_center=np.array(section["center"], dtype=np.float64), section_std=float(section["std"]),
                        section_size=float(section["size"]), section_variation=float(section["variation"]))
    print(f"g20_targets: {n} targets, {sum(updates)} updates, {os.path.getsize(os.path.join(OUT, 'g20_targets.npz'))} bytes")


if __name__ == "__main__":
    main()
