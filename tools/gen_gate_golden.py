"""tests/golden/g18_gates.npz: the reference's own Gate geometry for tests/test_gates_host.py - eight gates, data only.

Six gates as the reference's track factory builds them (generators.generate_track: all three shapes, yawed around the circle) and
two hand-placed ones that are pitched and rolled.  One row per gate: position, rotation_matrix, size, shapes, plane
(calculate_plane_equation), distance (calculate_distance of the 64 seeded `points`); corners holds the closed outlines the
reference draws, one after the other (corner_count rows each).
Runs where the reference is checked out (oracle.gen_golden.import_reference); the fixture is committed, this script only documents
how it was made:  python tools/gen_gate_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)


def main():
    from oracle import gen_golden
    gen_golden.import_reference()
    from utils.components import Gate
    from utils.generators import generate_track
    from utils.helper_functions import euler_angles_to_rotation_matrix
    gates = generate_track(6, 8.0, 2.0, 5)
    shapes = [("rectangle", "circle", "half_circle")[k % 3] for k in range(6)]
    gates.append(Gate(np.array([1.5, -2.0, 6.0]), euler_angles_to_rotation_matrix(0.0, np.deg2rad(20.0), np.deg2rad(35.0)), 1.6,
                      shape="half_circle", resolution=9))
    gates.append(Gate(np.array([-3.0, 0.5, 4.0]), euler_angles_to_rotation_matrix(np.deg2rad(-30.0), np.deg2rad(10.0), 0.0), 2.4,
                      shape="circle", resolution=9))
    shapes += ["half_circle", "circle"]
    rng = np.random.default_rng(18)
    points = rng.uniform(-10.0, 10.0, (64, 3))
    out = {"points": points, "shapes": np.array(shapes),
           "position": np.array([g.position for g in gates], dtype=np.float64),
           "rotation_matrix": np.array([g.rotation_matrix for g in gates], dtype=np.float64),
           "size": np.array([g.size for g in gates], dtype=np.float64),
           "corners": np.concatenate([g.corners for g in gates]).astype(np.float64),          # gate k's rows: corner_count[:k].sum() ...
           "corner_count": np.array([len(g.corners) for g in gates], dtype=np.int64),
           "plane": np.array([g.calculate_plane_equation() for g in gates], dtype=np.float64),
           "distance": np.array([[g.calculate_distance(p) for p in points] for g in gates], dtype=np.float64)}
    path = os.path.join(REPO, "tests", "golden", "g18_gates.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
