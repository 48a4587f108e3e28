"""Gate courses on the host (include/fpv_abi.h "Gate courses") - no GPU needed: the descriptor rows against the
reference's own Gate geometry (tests/golden/g18_gates.npz), the kernels' gate function (fpv_gate_eval) against a float64 NumPy
restatement over a lane-model trajectory, the laps / start-gate / reset / bonus rules on hand-made segments, and the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gate_course as gc
from conftest import REPO, load_golden
from fpyv_amd import _lib
from fpyv_amd import gates as G
from fpyv_amd.objects import Gate

PASS, MISS, FINISH = _lib.GATE_EVENT_PASS, _lib.GATE_EVENT_MISS, _lib.GATE_EVENT_FINISH


def _golden_gates():
    g = load_golden("g18_gates")
    ends = np.cumsum(g["corner_count"])
    out = []
    for k in range(len(g["size"])):
        gate = Gate(g["position"][k], g["rotation_matrix"][k], float(g["size"][k]), str(g["shapes"][k]))
        out.append((gate, g["corners"][ends[k] - g["corner_count"][k]:ends[k]], g["plane"][k], g["distance"][k]))
    return g, out


def _aperture(row, points):
    """the aperture test of fpv_abi.h on world points [m, 3], in float64 on the fp32 descriptor row"""
    row = row.astype(np.float64)
    x = points - row[0:3]
    y, z = x @ row[6:9], x @ row[9:12]
    return (np.abs(y) <= row[12]) & (np.abs(z) <= row[13]) & (y * y + (z - row[14]) ** 2 <= row[15])


# ---- T1: geometry against the reference ---------------------------------------------------------------------------------------
def test_descriptor_rows_reproduce_the_reference_gates():
    g, gates = _golden_gates()
    assert len(gates) == 8 and {"rectangle", "circle", "half_circle"} == set(g["shapes"].tolist())
    rows = G.derive([gate for gate, *_ in gates])
    assert rows.shape == (8, _lib.FPV_GATE_FLOATS) and rows.dtype == np.float32
    pts = g["points"]
    for (gate, corners, plane, dist), row in zip(gates, rows):
        r64 = row.astype(np.float64)
        # the plane: n.(p - c) of the fp32 row against the recorded calculate_distance, 1e-6 = the fp32 narrowing of metre-scale values
        assert np.abs((pts - r64[0:3]) @ r64[3:6] - dist).max() <= 1e-6
        assert np.abs(r64[3:6] - plane[:3]).max() <= 1e-7 and abs(-r64[3:6] @ r64[0:3] - plane[3]) <= 1e-6
        # every recorded corner lies on the aperture's boundary: just inside it is in, just outside it is out
        c = np.asarray(gate.position, np.float64)
        assert _aperture(row, c + (corners - c) * (1 - 1e-4)).all(), gate.shape
        assert not _aperture(row, c + (corners - c) * (1 + 1e-4)).any(), gate.shape
        assert np.abs((corners - r64[0:3]) @ r64[3:6]).max() <= 1e-6              # ... and in the gate's plane
        # objects.Gate keeps the reference's plane functions
        assert np.abs(gate.calculate_distance(pts) - dist).max() <= 1e-12
        assert abs(gate.calculate_distance(pts[0]) - dist[0]) <= 1e-12
        assert np.abs(gate.calculate_plane_equation() - plane).max() <= 1e-12 and np.array_equal(gate.normal, plane[:3])
        assert gate.collides is False


def test_derive_refuses_what_is_not_a_gate_and_names_it():
    ok = Gate(np.zeros(3), np.eye(3), 1.0)
    for bad, what in ((Gate(np.zeros(3), np.eye(3), 0.0), "size"), (Gate(np.zeros(3), np.eye(3), -1.0), "size"),
                      (Gate(np.zeros(3), np.eye(3) * (1 + 1e-5), 1.0), "orthonormal"),
                      (Gate(np.zeros(3), np.array([[1, 1e-5, 0], [0, 1, 0], [0, 0, 1.0]]), 1.0), "orthonormal")):
        with pytest.raises(_lib.FpvError, match=f"gate 2: .*{what}") as e:
            G.derive([ok, ok, bad])
        assert e.value.name == "FPV_EPARAM"
    arr = (_lib.FpvGate * 1)()
    arr[0].rotation[:] = np.eye(3).reshape(9).tolist()
    arr[0].size, arr[0].shape = 1.0, 7
    out = np.zeros(16, np.float32)
    L = _lib.lib()
    assert L.fpv_gates_derive(1, C.addressof(arr), out.ctypes.data) == -5 and b"gate 0" in L.fpv_last_error() and b"shape" in L.fpv_last_error()
    for count in (0, 65):
        with pytest.raises(_lib.FpvError, match="1..64"):
            G.derive([ok] * count)
    assert G.derive([ok] * 64).shape == (64, 16)
    with pytest.raises(NotImplementedError):
        Gate(np.zeros(3), np.eye(3), 1.0, shape="triangle").shape_code()
    # a rotation within 1e-6 of orthonormal is a gate
    assert G.derive([Gate(np.zeros(3), np.eye(3) * (1 + 2e-7), 1.0)]).shape == (1, 16)


def test_circular_track_is_a_closed_round_course():
    tr = G.circular_track(9, 12.0, 2.0, height=3.0)
    rows = G.derive(tr).astype(np.float64)
    assert [g.shape for g in tr[:4]] == ["rectangle", "circle", "half_circle", "rectangle"]
    c, n = rows[:, 0:3], rows[:, 3:6]
    assert np.allclose(np.hypot(c[:, 0], c[:, 1]), 12.0) and np.allclose(c[:, 2], 3.0)
    assert np.abs(np.einsum("ij,ij->i", n, c - [0, 0, 3.0])).max() < 1e-5          # normals are tangent to the circle ...
    nxt = np.roll(c, -1, axis=0) - c
    assert (np.einsum("ij,ij->i", n, nxt) > 0).all()                                 # ... and point at the next gate
    with pytest.raises(ValueError):
        G.circular_track(65, 10.0, 1.0)


# ---- T2: fpv_gate_eval against the float64 restatement ------------------------------------------------------------------------
def test_gate_eval_matches_the_float64_race_over_a_lane_model_trajectory():
    """Worst case seen: progress reward 3.4 ulp of the larger distance, observation 3.1 ulp of |c_h - p|."""
    _, _, snaps, pdone = gc.trajectory()
    ref = gc.race64()
    rows = ref["rows"]
    # what the float64 logic gives on this course: the floors make an eventless run fail
    assert not pdone.any()
    assert (ref["passes"] > 0).sum() >= 100 and (ref["misses"] > 0).sum() >= 100 and (ref["backward"] > 0).sum() >= 30
    assert gc.assert_event_floors(ref["words"])[2] >= 3
    keep = ~ref["excluded"]
    assert ref["excluded"].mean() <= 0.05
    word = np.zeros(gc.N, np.uint32)
    worst_r = worst_o = 0.0
    for t in range(gc.STEPS):
        po, pn, qn = snaps[t, 0:3].T, snaps[t + 1, 0:3].T, snaps[t + 1, 6:10].T
        word, rew, done, obs = G.evaluate(rows, po, pn, qn, pdone[t], word, gate_rewards=gc.REWARDS_PROGRESS_ONLY)
        bad = np.flatnonzero((word != ref["words"][t]) & keep)
        assert bad.size == 0, f"step {t}: words differ for drones {bad[:5]}: {word[bad[:5]]} != {ref['words'][t][bad[:5]]}"
        assert not done.any()
        err = np.abs(rew - ref["reward"][t])[keep] / (gc.EPS32 * ref["dist"][t][keep])
        worst_r = max(worst_r, float(err.max()))
        want, scale = gc.obs64(rows, word, qn, pn)
        eo = np.abs(obs - want)[keep]
        worst_o = max(worst_o, float((eo[:, :3] / (gc.EPS32 * scale[keep, None])).max()), float((eo[:, 3:] / gc.EPS32).max()))
    print(f"gate_eval vs float64: worst progress reward {worst_r:.2f} ulp of the larger distance, worst obs {worst_o:.2f} ulp of |c_h - p|")
    assert worst_r <= 16 and worst_o <= 16


# ---- T3: laps, start gates, reset and bonuses on hand-made segments -----------------------------------------------------------
def _two_gates():
    return G.derive([Gate(np.array([1.0, 0, 5.0]), np.eye(3), 1.0, "rectangle"), Gate(np.array([2.0, 0, 5.0]), np.eye(3), 1.0, "circle")])


def _seg(rows, x0, x1, word=0, y=0.0, done=False, **kw):
    w, r, d, o = G.evaluate(rows, [[x0, y, 5.0]], [[x1, y, 5.0]], [[1, 0, 0, 0]], [done], [word], **kw)
    return int(w[0]), float(r[0]), bool(d[0]), o[0]


def _fields(w):
    return w & 0xFF, (w >> 8) & 3, w >> 10


def test_laps_finish_wrap_and_reset():
    rows = _two_gates()
    zero = dict(gate_rewards=dict(progress=0.0, passed=0.0, finish=0.0, missed=0.0, crash=0.0))
    w = 0
    seen = []
    for lap in range(2):                 # laps = 2 on two gates: FINISH at exactly the fourth pass
        for x in (1.0, 2.0):
            w, _, d, _ = _seg(rows, x - 0.1, x + 0.1, w, laps=2, **zero)
            seen.append((_fields(w), d))
    assert seen == [((1, PASS, 1), False), ((0, PASS, 2), False), ((1, PASS, 3), False), ((0, FINISH, 4), True)]
    # laps = 0 never finishes, and a step without a crossing clears the event
    w, _, d, _ = _seg(rows, 0.9, 1.1, seen[-1][0][0] | (4 << 10), **zero)
    assert _fields(w) == (1, PASS, 5) and not d
    w, _, d, _ = _seg(rows, 1.1, 1.2, w, **zero)
    assert _fields(w) == (1, 0, 5) and not d
    # only the next gate is tested: crossing gate 0's plane while gate 1 is next is no event
    assert _fields(_seg(rows, 0.9, 1.1, 1, **zero)[0]) == (1, 0, 0)
    # a reset (auto_reset and done): passed = 0, next = gate_start[i], the event still describes the step; obs points at the new gate
    w, _, d, o = _seg(rows, 1.9, 2.1, 1 | (3 << 10), laps=2, auto_reset=True, gate_start=[1], p_after=[[0.0, 0, 5.0]], q_after=[[1, 0, 0, 0]], **zero)
    assert d and _fields(w) == (1, FINISH, 0) and np.allclose(o, [2.0, 0, 0, 1, 0, 0])
    w, _, d, o = _seg(rows, 1.9, 2.1, 1 | (3 << 10), laps=2, auto_reset=True, **zero)
    assert d and _fields(w) == (0, FINISH, 0) and np.allclose(o, [1.0 - 2.1, 0, 0, 1, 0, 0])       # no start table: gate 0, seen from p_new
    w, _, d, _ = _seg(rows, 1.9, 2.1, 1 | (3 << 10), laps=2, auto_reset=False, gate_start=[1], **zero)
    assert d and _fields(w) == (0, FINISH, 4)                                                      # no auto-reset: the word runs on
    assert _fields(_seg(rows, 1.9, 2.1, 1, auto_reset=True, gate_start=[9], miss_is_done=True, y=3.0, **zero)[0]) == (0, MISS, 0)   # a start gate past the course: gate 0
    # physics done resets too
    assert _fields(_seg(rows, 1.1, 1.2, 1 | (7 << 10), done=True, auto_reset=True, gate_start=[1], **zero)[0]) == (1, 0, 0)


def test_miss_backward_and_the_plane_itself():
    rows = _two_gates()
    zero = dict(gate_rewards=dict(progress=0.0, passed=0.0, finish=0.0, missed=0.0, crash=0.0))
    w, _, d, _ = _seg(rows, 0.9, 1.1, 0, y=0.6, **zero)                 # outside the 1 m rectangle
    assert _fields(w) == (0, MISS, 0) and not d
    w, _, d, _ = _seg(rows, 0.9, 1.1, 0, y=0.6, miss_is_done=True, **zero)
    assert _fields(w) == (0, MISS, 0) and d
    w, _, d, _ = _seg(rows, 1.9, 2.1, 1, y=0.45, **zero)                # inside the circle (r = 0.5)
    assert _fields(w)[1] == PASS
    z = G.evaluate(rows, [[1.9, 0.4, 5.4]], [[2.1, 0.4, 5.4]], [[1, 0, 0, 0]], [0], [1], **zero)[0][0]
    assert _fields(int(z)) == (1, MISS, 0)                               # the corner of the square is outside the circle
    # a backward crossing through the aperture is no event
    w, _, d, _ = _seg(rows, 1.1, 0.9, 0, **zero)
    assert _fields(w) == (0, 0, 0) and not d
    # s1 == 0 counts as a forward crossing; s0 == 0 does not
    assert _fields(_seg(rows, 0.9, 1.0, 0, **zero)[0]) == (1, PASS, 1)
    assert _fields(_seg(rows, 1.0, 1.1, 0, **zero)[0]) == (0, 0, 0)
    assert _fields(_seg(rows, 1.0, 1.0, 0, **zero)[0]) == (0, 0, 0)


def test_each_reward_term_alone():
    rows = _two_gates()
    keys = ("progress", "passed", "finish", "missed", "crash")
    only = lambda k, v: dict(gate_rewards={q: (v if q == k else 0.0) for q in keys})  # noqa: E731
    # progress: the distance to the NEXT gate's centre before the step minus after it, here 0.25 - 0.125 along x
    assert _seg(rows, 0.75, 0.875, 0, **only("progress", 2.0))[1] == 2.0 * (0.25 - 0.125)
    assert _seg(rows, 0.875, 0.75, 0, **only("progress", 2.0))[1] == -2.0 * (0.25 - 0.125)
    # the pass bonus on PASS and on FINISH, the finish bonus on FINISH only
    assert _seg(rows, 0.9, 1.1, 0, **only("passed", 3.0))[1] == 3.0
    assert _seg(rows, 1.9, 2.1, 1 | (1 << 10), laps=1, **only("passed", 3.0))[1] == 3.0
    assert _seg(rows, 0.9, 1.1, 0, **only("finish", 7.0))[1] == 0.0
    assert _seg(rows, 1.9, 2.1, 1 | (1 << 10), laps=1, **only("finish", 7.0))[1] == 7.0
    # the miss penalty on MISS only, the crash penalty on physics done only
    assert _seg(rows, 0.9, 1.1, 0, y=0.6, **only("missed", 4.0))[1] == -4.0
    assert _seg(rows, 0.9, 1.1, 0, **only("missed", 4.0))[1] == 0.0
    assert _seg(rows, 0.7, 0.8, 0, done=True, **only("crash", 9.0))[1:3] == (-9.0, True)
    assert _seg(rows, 0.7, 0.8, 0, **only("crash", 9.0))[1:3] == (0.0, False)
    # all together on a finishing step that also crashes
    r = _seg(rows, 1.875, 2.125, 1 | (1 << 10), laps=1, done=True, gate_rewards=dict(progress=1.0, passed=3.0, finish=7.0, missed=4.0, crash=9.0))[1]
    assert r == (0.125 - 0.125) + 3.0 + 7.0 - 9.0
    with pytest.raises(ValueError, match="gate_rewards"):
        _lib.pack_course(2, gate_rewards=dict(bonus=1.0))


# ---- T4: exports and the ABI are what they were -------------------------------------------------------------------------------
def test_exports_sizes_and_null_handle():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "fpv_abi.h"), encoding="utf-8").read()
    for name in ("fpv_gates_derive", "fpv_set_gates", "fpv_gate_eval"):
        assert name in _lib.EXPORTS and hasattr(L, name) and f"int {name}(" in hdr
    assert L.fpv_abi_version() == 9 and "#define FPV_ABI_VERSION 9" in hdr
    assert L.fpv_sizeof(0) == C.sizeof(_lib.FpvParams) == 688 and L.fpv_sizeof(1) == C.sizeof(_lib.FpvBuffers) == 200
    assert L.fpv_sizeof(5) == C.sizeof(_lib.FpvGateCourse) and L.fpv_sizeof(9) < 0
    c = _lib.pack_course(2)
    assert L.fpv_set_gates(None, C.byref(c)) == -1 and b"null handle" in L.fpv_last_error()
    assert L.fpv_set_gates(None, None) == -1 and b"null handle" in L.fpv_last_error()
    # the constants of a course are checked before anything else of it is read
    rows = _two_gates()
    for kw, what in ((dict(laps=-1), "laps"), (dict(laps=1 << 21), "laps"), (dict(gate_rewards=dict(progress=float("inf"))), "finite")):
        with pytest.raises(_lib.FpvError, match=what):
            G.evaluate(rows, [[0, 0, 0]], [[0, 0, 0]], [[1, 0, 0, 0]], [0], [0], **kw)


def test_fpv_hip_alone_says_gate_courses_are_not_in_this_build(tmp_path):
    """fpv_hip.hip alone still links, exports the three new names, refuses a bind with a message that says why, and derives the
    same descriptor rows (the host arithmetic lives in fpv_hip.hip and its headers)."""
    import torch  # noqa: F401  (the HIP runtime torch ships, as fpyv_amd._lib loads it)
    from __graft_entry__ import HIPCC_FLAGS, HIP_SRC
    out = str(tmp_path / "libfpv_alone.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIPCC_FLAGS + ["-o", out, HIP_SRC], check=True, capture_output=True)
    A = C.CDLL(out, mode=C.RTLD_LOCAL)
    for name in _lib.EXPORTS:
        assert hasattr(A, name), name
    A.fpv_last_error.restype = C.c_char_p
    A.fpv_set_gates.argtypes = [C.c_void_p, C.c_void_p]
    c = _lib.pack_course(2)
    assert A.fpv_set_gates(None, C.byref(c)) == -1 and b"not in this build" in A.fpv_last_error()
    assert A.fpv_set_gates(None, None) == -1 and b"null handle" in A.fpv_last_error()        # unbinding needs no kernel
    course = gc.course()
    arr = G._rows_of(course)
    rows = np.zeros((len(course), 16), np.float32)
    A.fpv_gates_derive.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    assert A.fpv_gates_derive(len(course), C.addressof(arr), rows.ctypes.data) == 0
    assert np.array_equal(rows.view(np.uint32), G.derive(course).view(np.uint32))
