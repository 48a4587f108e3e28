"""The edge-lane set (tests/edge_lanes.py) on the host - no GPU needed: the host functions of the five law and sensor kernels on
every lane.  What tests/test_gpu_edge_lanes.py relies on is pinned here, so that the set cannot silently lose a branch: every class
reaches the branch it was built for; the rules the headers state hold as rules on every lane; a NaN that leaves a function is the
one constant word, except in the five pursuit channels that carry arithmetic; and on the finite degenerate classes the fp32 host
functions agree with the float64 restatements within the bounds the units' own host modules assert.

Prints, per class, the lane count and the share a restatement leaves out by its own margin: of the lanes for the laws and the pursuit
task, of the lane-ray and lane-pixel pairs for the range scan and the depth camera."""
import functools

import numpy as np
import pytest

import depth_scene as DS
import edge_lanes as E
import pursuit_task as PT
import range_scene as RS
from chase_law import Law
from fpyv_amd import _lib
from fpyv_amd.camera import DepthCamera, gate_rows
from fpyv_amd import rays as RY
from fpyv_amd.chase import ChaseGuidance
from fpyv_amd.pns import PointAndShoot
from pns_law import PnsLaw
from test_chase_host import FP32_TOL_FORCE as CHASE_TOL_FORCE
from test_chase_host import FP32_TOL_MATRIX as CHASE_TOL_MATRIX
from test_depth_host import ULP_BOUND as DEPTH_ULP_BOUND
from test_pns_host import FP32_TOL_FORCE as PNS_TOL_FORCE
from test_pns_host import FP32_TOL_MATRIX as PNS_TOL_MATRIX
from test_range_host import ULP_BOUND as RANGE_ULP_BOUND

QNAN = 0x7FC00000
EYE9 = np.eye(3, dtype=np.float32).reshape(9)
LEFT_OUT_MAX = 0.10


def only_the_constant_nan(*arrays):
    for a in arrays:
        a = np.ascontiguousarray(E.f32(a))
        if not np.all(a.view(np.uint32)[np.isnan(a)] == QNAN):
            return False
    return True


def orthonormal(rot9, tol=1e-5):
    R = rot9.reshape(-1, 3, 3).astype(np.float64)
    return np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).reshape(len(R), -1).max(1) <= tol


def report(title, S, left_out, unit="lanes"):
    """print, per class of `left_out` ({class: (left out, all)} in `unit`), the lane count and the share; every share is at most 10 %"""
    for cls, (out, total) in sorted(left_out.items()):
        print(f"{title}: class {cls}: {len(S.of(cls))} lanes, {out} of {total} {unit} = {100.0 * out / max(total, 1):.1f} % left out of the "
              f"restatement comparison")
        assert out <= LEFT_OUT_MAX * total, (title, cls, out, total)


# ---- the set -------------------------------------------------------------------------------------------------------------------------
def test_the_set_is_small_ragged_and_every_class_holds_two_lanes():
    S = E.lanes()
    counts = S.counts()
    for cls, c in sorted(counts.items()):
        print(f"class {cls}: {c} lanes")
    assert S.n < 512 and S.n % 64 != 0 and min(counts.values()) >= 2 and counts["base"] >= 32
    assert set(E.POSE_CLASSES) <= set(counts) and set(E.FINITE_DEGENERATE) <= set(counts)
    # the coordinates the classes were built for are there
    nf = S.of("nonfinite")
    assert all(np.sum(~np.isfinite(np.concatenate([S.p[i], S.v[i], S.q[i]]))) == 1 for i in nf)
    assert sum(np.isnan(S.p[i]).any() for i in nf) == 3 and sum(np.isinf(S.q[i]).any() for i in nf) == 8
    tiny = S.of("tiny")
    assert any(0 < np.abs(S.v[i]).max() < 1.2e-38 for i in tiny) and any(np.signbit(S.p[i]).any() and (S.p[i] == 0).any() for i in tiny)
    assert any(np.abs(S.v[i]).max() == E.FLUSH for i in tiny) and any(np.abs(S.v[i]).max() == E.down(E.FLUSH) for i in tiny)
    assert any(not S.q[i].any() for i in S.of("quat"))
    words = S.tgt.view(np.uint32)
    for w in (0x0000FFFF, 0xFFFF0000, 0xFFFFFFFF):
        assert (words[_lib.TGT_SPAWNS] == w).sum() == 4
    assert (words[_lib.TGT_COUNT] & 0x1FFFF == E.K_PATH - 1).sum() >= 2 and (words[_lib.TGT_COUNT] & 0x1FFFF >= E.K_PATH).sum() >= 4


# ---- the target chase ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chase(frame, mode, given, tweak=None):
    S = E.lanes()
    G = ChaseGuidance(E.params(), ref_frame=frame, mode=mode, max_depth=E.MAX_DEPTH)
    return E.chase_host(G, S.p, S.v, S.q, S.pid, S.pixel if given else None, tweak)


def law_rules(S, o, pid_before, prev_before=None, prev_after=None, restarted=None):
    """the rules fpv_chase.h 1. and 4. / fpv_pns.h 1. state, on every lane"""
    guided = np.isfinite(o["thrust"])
    assert np.all(np.isnan(o["thrust"][~guided])), "a thrust is finite or NaN"
    assert np.isfinite(o["rotation"]).all()                                  # no finite or other state gives a NaN matrix
    assert orthonormal(o["rotation"][guided]).all()
    assert np.all(o["rotation"][~guided] == EYE9)
    keep = ~guided if restarted is None else ~guided & ~restarted
    assert np.array_equal(E.bits(o["pid"][:, keep]), E.bits(pid_before[:, keep]))
    if prev_before is not None:
        assert np.array_equal(E.bits(prev_after[:, keep]), E.bits(prev_before[:, keep]))
    return guided


@pytest.mark.parametrize("frame,mode", E.PAIRS)
def test_chase_rules_branches_and_nan_words(frame, mode):
    S = E.lanes()
    for given in (False, True):
        o = chase(frame, mode, given)
        guided = law_rules(S, o, S.pid)
        seen = o["visible"].astype(bool)
        assert only_the_constant_nan(o["rotation"], o["thrust"], o["pixel"], o["pid"])
        assert (guided & seen).sum() >= 32 and (~seen).sum() >= 2
        overflow = seen & ~guided                                            # seen, and the result is not finite: not guided
        assert overflow.sum() >= 2 and set(S.cls[overflow]) <= {"overflow", "nonfinite", "pixel", "rows"}, set(S.cls[overflow])
        assert np.all(np.isnan(o["pixel"][~seen])) and np.all(np.isfinite(o["pixel"][seen & guided]) | given)
        if not given:
            # the classes that were placed by construction: seen or not as built
            for i in S.of("border"):
                assert seen[i] == ("seen = True" in S.note[i]), S.note[i]
            assert not seen[S.of("behind", "origin")].any()
            # ... and for the reason they were built for: czp is exactly 0 in the host function's own operations - 0 / 0 with the
            # centre on the origin, (f cxp) / 0 with it in the camera's plane, seen from either side.  The zero is +0 in every lane:
            # an fp32 sum of products is -0 only when every product is, which no rotation's entries give (edge_lanes.py's header)
            cxp, cyp, czp = E.camera_frame(S.p, S.q)
            at = S.of("origin")
            assert np.all(czp[at] == 0.0) and ((cxp[at] == 0.0) & (cyp[at] == 0.0)).sum() >= 2
            assert (cxp[at] > 0.0).sum() >= 2 and (cxp[at] < 0.0).sum() >= 2
            assert not np.signbit(czp[czp == 0.0]).any()
            with np.errstate(all="ignore"):
                assert np.array_equal(seen, (czp > 0) & (czp <= np.float32(E.MAX_DEPTH)) & np.isfinite(o["pixel"]).all(1))    # the restated czp is the host's
            assert seen[S.of("still", "tof", "command", "rows", "word")].all()
            assert seen[S.of("base")].sum() >= 24 and (~seen[S.of("base")]).sum() >= 8
        # |v| = 0 and |v| below the flush: no drag, a finite frame
        still = [i for i in S.of("tiny") if np.abs(S.v[i]).max() <= E.down(E.FLUSH)]
        assert len(still) >= 4 and (guided[still] | ~seen[still]).all()
    # F = 0: the identity and no thrust, guided (the PID advanced)
    z = chase(frame, mode, False, E.fzero)
    still = S.of("still")
    assert np.all(z["thrust"][still] == 0.0) and np.all(z["rotation"][still] == EYE9) and np.all(z["pid"][3, still] == 0.0)


def test_rows_given_in_column_major_order_are_read_as_rows():
    """`pid_state=rows[:, idx]` - NumPy lays a fancy-indexed [4, n] out column-major; the evaluate methods read it as the rows it shows"""
    S = E.lanes()
    P = E.params()
    idx = np.arange(S.n)[::-1].copy()
    fancy_pid, fancy_prev = S.pid[:, idx], S.prev[:, idx]
    assert not fancy_pid.flags["C_CONTIGUOUS"]
    c_pid, c_prev = np.ascontiguousarray(fancy_pid), np.ascontiguousarray(fancy_prev)
    p, v, q = S.p[idx], S.v[idx], S.q[idx]
    one = ChaseGuidance(P, max_depth=E.MAX_DEPTH).evaluate(p, v, q, (E.CENTRE, E.RADIUS), fancy_pid)
    two = ChaseGuidance(P, max_depth=E.MAX_DEPTH).evaluate(p, v, q, (E.CENTRE, E.RADIUS), c_pid)
    assert all(np.array_equal(E.bits(E.f32(a)), E.bits(E.f32(b))) for a, b in zip(one, two)) and np.isfinite(one[1]).sum() >= 32
    G = PointAndShoot(P, max_depth=E.MAX_DEPTH)
    one = G.evaluate(p, v, q, target=E.CENTRE, action=S.action[idx], pid_state=fancy_pid, prev_pixel=fancy_prev)
    two = G.evaluate(p, v, q, target=E.CENTRE, action=S.action[idx], pid_state=c_pid, prev_pixel=c_prev)
    assert all(np.array_equal(one[k], two[k], equal_nan=True) for k in one)
    task = E.pursuit_task(("world", "level"))
    one = task.evaluate(p, v, q, S.tgt[:, idx], PT.DT, done=S.done[idx], params=P, pid_state=fancy_pid)
    two = task.evaluate(p, v, q, np.ascontiguousarray(S.tgt[:, idx]), PT.DT, done=S.done[idx], params=P, pid_state=c_pid)
    assert all(np.array_equal(E.canonical(one[k]) if one[k].dtype == np.float32 else one[k], E.canonical(two[k]) if two[k].dtype == np.float32 else two[k])
               for k in one)


def y_column(rot9):
    return rot9.reshape(-1, 3, 3)[:, :, 1]


@pytest.mark.parametrize("law", ["chase", "pns"])
def test_both_fallback_axes_are_taken_and_told_apart_from_the_pose_off_the_parallel(law):
    """fpv_chase.h 4.: the y column is F x (1, 0, 0) normalised on the first fallback axis (no x component) and F x (0, 1, 0) on the
    second (no y component, F along x); the same lane with its pixel moved by 8 pixels is off the parallel and has the column of F x b"""
    S = E.lanes()
    P = E.params()
    cases = (("fallback1", "world", "level", "level:"), ("fallback1", "world", "frontarget", "frontarget:"), ("fallback2", "drone", "level", "drone"),
             ("fallback2", "drone", "frontarget", "drone"))
    for cls, frame, mode, tag in cases:
        idx = np.array([i for i in S.of(cls) if S.note[i].startswith(tag)])
        assert len(idx) >= 2
        nudged = S.pixel[idx] + np.float32(8.0)
        if law == "chase":
            G = ChaseGuidance(P, ref_frame=frame, mode=mode, max_depth=E.MAX_DEPTH)
            on = E.chase_host(G, S.p[idx], S.v[idx], S.q[idx], S.pid[:, idx], S.pixel[idx])
            off = E.chase_host(G, S.p[idx], S.v[idx], S.q[idx], S.pid[:, idx], nudged)
        else:
            G = PointAndShoot(P, ref_frame=frame, mode=mode, max_depth=E.MAX_DEPTH)
            zero = np.zeros((len(idx), 4), np.float32)
            on = E.pns_host(G, S.p[idx], S.v[idx], S.q[idx], S.pid[:, idx], S.prev[:, idx], "pixel", None, S.pixel[idx], zero)
            off = E.pns_host(G, S.p[idx], S.v[idx], S.q[idx], S.pid[:, idx], S.prev[:, idx], "pixel", None, nudged, zero)
        assert np.isfinite(on["thrust"]).all() and np.isfinite(off["thrust"]).all() and orthonormal(on["rotation"]).all()
        y, F = y_column(on["rotation"]), on["rotation"].reshape(-1, 3, 3)[:, :, 2]
        if cls == "fallback1":
            assert np.all(np.abs(y[:, 0]) <= 1e-6) and np.all(np.abs(F[:, 2]) >= 1 - 1e-6), (law, frame, mode, y, F)     # y = F x e_x, F vertical
        else:
            assert np.all(np.abs(y[:, 1]) <= 1e-6) and np.all(np.abs(F[:, 0]) >= 1 - 1e-6), (law, frame, mode, y, F)     # y = F x e_y, F along x
        # off the parallel the column is that of F x b: a different one
        assert np.all(np.abs(y - y_column(off["rotation"])).max(1) >= 1e-3), (law, frame, mode)


# ---- point and shoot ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pns(frame, mode, source, tweak=None):
    """two calls in a row, the restart bytes on the second: (first, second)"""
    S = E.lanes()
    G = PointAndShoot(E.params(), ref_frame=frame, mode=mode, max_depth=E.MAX_DEPTH)
    one = E.pns_host(G, S.p, S.v, S.q, S.pid, S.prev, source, S.own, S.pixel, S.action, None, tweak)
    two = E.pns_host(G, S.p, S.v, S.q, one["pid"], one["prev"], source, S.own, S.pixel, S.action, S.restart, tweak)
    return one, two


@pytest.mark.parametrize("frame,mode", E.PAIRS)
def test_pns_rules_branches_and_nan_words(frame, mode):
    S = E.lanes()
    fmax = np.float32(E.params().max_throttle_in_force)
    for source in ("shared", "rows", "pixel"):
        one, two = pns(frame, mode, source)
        for o, before_pid, before_prev, restarted in ((one, S.pid, S.prev, None), (two, one["pid"], one["prev"], S.restart != 0)):
            guided = law_rules(S, o, before_pid, before_prev, o["prev"], restarted)
            assert only_the_constant_nan(o["rotation"], o["thrust"], o["throttle"], o["velocity"], o["pid"], o["prev"])
            assert np.all(o["visible"][guided] == 1) and np.all(o["limited"][~guided] == 0)
            assert np.all(np.isnan(o["throttle"][~guided])) and np.all(np.isnan(o["velocity"][~guided]))
            assert np.all(np.abs(o["throttle"][guided]) <= 1.0)
            assert guided.sum() >= 32 and (~guided).sum() >= 2
        guided = np.isfinite(one["thrust"])
        # a command that is not finite: not guided, whatever the pixel
        for i in S.of("command"):
            a = S.action[i]
            if not np.isfinite(a).all():
                assert not guided[i] and one["visible"][i] == 0, S.note[i]
        huge = [i for i in S.of("command") if np.isfinite(S.action[i]).all() and np.abs(S.action[i]).max() >= 1e30]
        assert len(huge) >= 8
        if source == "pixel":
            lim = one["limited"]
            assert (lim[guided] == 0).sum() >= 32 and (lim == 1).sum() >= 2 and (lim == 2).sum() >= 2, np.bincount(lim)
            assert np.all(one["thrust"][lim == 2] == fmax)                   # bit-exact where the header says so (fpv_pns.h 5.)
            if (frame, mode) == ("world", "level"):                          # the pair the limit lanes were searched in
                solved = [i for i in S.of("limit") if "solved" in S.note[i] and "change" not in S.note[i]]
                clipped = [i for i in S.of("limit") if "clipped at max_output" in S.note[i]]
                assert len(solved) >= 2 and np.all(one["thrust"][solved] == fmax) and np.all(lim[solved] == 1)
                assert len(clipped) >= 2 and np.all((one["thrust"][clipped] < fmax) & (lim[clipped] == 1))
                # which end the root met, and the discriminant's sign, from the float64 terms (they are no output of the host function)
                terms = {i: E._Law().limit_terms(S.p[i], S.v[i], np.eye(3), S.pixel[i]) for i in S.of("limit") if "about" not in S.note[i]}
                assert all(terms[i][0] > 0 and terms[i][1] > terms[i][3] for i in clipped)
                low = [i for i in S.of("limit") if "clipped at min_output" in S.note[i]]
                assert len(low) >= 2 and all(terms[i][0] > 0 and terms[i][1] < terms[i][2] for i in low) and np.all(lim[low] == 2)
                negative = [i for i in S.of("limit") if "negative discriminant" in S.note[i]]
                assert len(negative) >= 2 and all(terms[i][0] < 0 for i in negative) and np.all(lim[negative] == 2)
                assert np.float64(fmax) ** 2 != np.float64(np.float32(np.float64(fmax) ** 2))     # Fmax^2 is no fp32 value (edge_lanes.py's header)
                edge = [i for i in S.of("limit") if "about Fmax" in S.note[i]]
                assert sorted(lim[edge] > 0) == [False, True]                 # the two speeds either side of |F| = Fmax
                change = [i for i in S.of("limit") if "change" in S.note[i]]
                assert len(change) >= 2 and set(lim[change]) == {1, 2}
            # the second call of a restarted lane is its first call again
            again = (S.restart != 0) & np.isfinite(two["thrust"])
            assert again.sum() >= 1 and np.all(two["velocity"][again] == 0.0) and np.all(two["pid"][1, again] == 0.0)
            idle = (S.restart != 0) & ~np.isfinite(two["thrust"])            # restarted and then not guided: the reset rows are stored
            assert idle.sum() >= 1 and np.all(two["pid"][3, idle] == 1.0) and np.all(np.isnan(two["prev"][:, idle]))
            # the truncation toward zero of (H / 2)(1 + a1): the PID's error row holds pixel.y - trunc(..)
            for i in S.of("command"):
                if "about -0.5" in S.note[i] and guided[i]:
                    assert one["pid"][2, i] == np.float32(np.float32(S.pixel[i, 1]) - np.float32(0.0)), S.note[i]
    z, _ = pns(frame, mode, "shared", E.fzero)
    still = S.of("still")
    assert np.all(z["thrust"][still] == 0.0) and np.all(z["rotation"][still] == EYE9) and np.all(z["limited"][still] == 0)


# ---- the laws against their float64 restatements on the finite degenerate classes ------------------------------------------------------
def test_laws_agree_with_the_float64_restatements_on_the_finite_degenerate_classes():
    S = E.lanes()
    P = E.params()
    idx = S.of(*LAW_CLASSES)
    R64 = RS.rot64(S.q)
    fresh = np.array([0.0, 0.0, 0.0, 1.0])
    for frame, mode in E.PAIRS:
        left = {c: [0, 0] for c in LAW_CLASSES}
        law, plaw = Law.from_params(P, E.MAX_DEPTH), PnsLaw.from_params(P, E.MAX_DEPTH)
        c_found, c_given = chase(frame, mode, False), chase(frame, mode, True)
        p_given, _ = pns(frame, mode, "pixel")
        for i in idx:
            left[S.cls[i]][1] += 1
            out = False                                                       # is any comparison of this lane left out?
            p, v, R = S.p[i].astype(np.float64), S.v[i].astype(np.float64), R64[i]
            # (a speed below the flush has no drag by the header and a drag of 1e-30 N in the restatement: within every bound)
            for o, pixel in ((c_found, None), (c_given, S.pixel[i].astype(np.float64))):
                rot, force, _, seen, _ = law(p, v, R, CENTRE64, E.RADIUS, fresh, pixel=pixel, frame=frame, mode=mode)
                guided = np.isfinite(o["thrust"][i])
                if pixel is None and abs(margin_of_sight(law, p, R)) < 1e-4:
                    out = True                                                # the restatement's own margin: the centre on a border
                    continue
                assert bool(seen) == guided, (S.cls[i], S.note[i], frame, mode)
                if guided and fallback_lane(S, i) and (not same_axis(o["rotation"][i].reshape(3, 3), rot)
                                                       or ill_conditioned(law, rot, p, R, pixel, frame, mode, CHASE_TOL_MATRIX)):
                    out = True                                                # its own margin: F is parallel for one of the two only
                elif guided:
                    assert np.abs(o["rotation"][i].reshape(3, 3) - rot).max() <= CHASE_TOL_MATRIX, (S.cls[i], S.note[i], frame, mode)
                    assert abs(o["thrust"][i] - force) <= CHASE_TOL_FORCE * max(force, 1.0), (S.cls[i], S.note[i])
            w = plaw(p, v, R, S.action[i].astype(np.float64), fresh, np.full(2, np.nan), pixel=S.pixel[i].astype(np.float64), frame=frame, mode=mode)
            guided = np.isfinite(p_given["thrust"][i])
            steered = S.pixel[i].astype(np.float64) + S.action[i, 2:].astype(np.float64) * [plaw.w / 2, plaw.h / 2]     # the pixel the law aims at
            assert w["guided"] == guided, (S.cls[i], S.note[i], frame, mode)
            if guided and fallback_lane(S, i) and (not same_axis(p_given["rotation"][i].reshape(3, 3), w["rot"])
                                                   or ill_conditioned(plaw, w["rot"], p, R, steered, frame, mode, PNS_TOL_MATRIX)):
                out = True
            elif guided and "about" in S.note[i] and w["limited"] != p_given["limited"][i]:
                out = True                                                    # an ulp from a threshold of the limit: float64 is on its other side
            elif guided:
                assert w["limited"] == p_given["limited"][i], (S.cls[i], S.note[i], frame, mode)
                assert np.abs(p_given["rotation"][i].reshape(3, 3) - w["rot"]).max() <= PNS_TOL_MATRIX, (S.cls[i], S.note[i], frame, mode)
                assert abs(p_given["thrust"][i] - w["thrust"]) <= PNS_TOL_FORCE * max(w["thrust"], 1.0), (S.cls[i], S.note[i])
            left[S.cls[i]][0] += out
        report(f"laws {frame}/{mode}", S, {c: tuple(x) for c, x in left.items() if x[1]})


CENTRE64 = E.CENTRE.astype(np.float64)


def margin_of_sight(law, p, R):
    """how far (pixels, metres) the centre is from the nearest edge of `seen` in float64"""
    pix, depth, _ = law.project(p, R, CENTRE64)
    with np.errstate(invalid="ignore"):
        m = np.nanmin(np.abs([pix[0], pix[0] - law.w, pix[1], pix[1] - law.h, depth, depth - law.max_depth]))
    return m


LAW_CLASSES = ("tiny", "turn", "fallback1", "fallback2", "still", "limit", "tof")         # the finite degenerate classes that are about the laws


def fallback_lane(S, i):
    """the restatement takes a fallback axis when ITS F is parallel: on these lanes fp32 and float64 may decide differently"""
    return S.cls[i] in ("fallback1", "fallback2")


def ill_conditioned(law, rot, p, R, pixel, frame, mode, tol):
    """Is the restated F (rot's third column) off the parallel to the cross product's operand b, but by a sine so small that the
    fp32 rounding of F alone, 2^-24 of its length, turns y = F x b by more than `tol`?  sine < 2^-24 / tol.  From float64 values only."""
    if mode == "level":
        b = law.g if frame == "world" else R @ law.g
    else:
        pix = law.project(p, R, CENTRE64)[0] if pixel is None else pixel
        b = R @ (law.rr @ np.array([(pix[0] - law.w / 2) / law.f, (pix[1] - law.h / 2) / law.f, 1.0]))
    sine = np.linalg.norm(np.cross(rot[:, 2], b)) / np.linalg.norm(b)
    return bool(rot[0, 1] != 0.0 and rot[1, 1] != 0.0 and sine < 2.0 ** -24 / tol)


def same_axis(rot32, rot64):
    """did fp32 and float64 take the same axis?  The y column of the first fallback, F x (1, 0, 0), has an x component of exactly 0 and
    that of the second, F x (0, 1, 0), a y component of exactly 0; off the parallel neither is"""
    return np.array_equal(rot32[:2, 1] == 0.0, rot64[:2, 1] == 0.0)


# ---- range scan and depth camera ---------------------------------------------------------------------------------------------------------
def ulps(got, ref, scale):
    return np.abs(got.astype(np.float64) - ref) / np.spacing(np.maximum(scale, 1e-3).astype(np.float32)).astype(np.float64)


def without(world, k):
    return [ob for j, ob in enumerate(world) if j != k]


def test_every_range_is_finite_and_within_reach_on_every_lane_and_agrees_with_the_restatement():
    S = E.lanes()
    rays = E.ray_set()
    for count in (0, 8):
        world = RS.world(count)
        got = RY.evaluate(rays, RS.MAX_RANGE, S.p, S.q, world)
        assert np.isfinite(got).all() and (got >= 0).all() and (got <= np.float32(RS.MAX_RANGE)).all()       # every lane, every ray
        if count == 0:
            assert np.all(got == np.float32(RS.MAX_RANGE))
            continue
        # a pose that is not finite, or absurd: a NaN or infinite position is near nothing (every cull test is false) and reports
        # max_range; a quaternion that is not finite turns every ray into NaN, which meets nothing
        absurd = S.of("nonfinite", "overflow")
        ground = RY.evaluate(rays, RS.MAX_RANGE, S.p[absurd], S.q[absurd], RS.world(1))
        for k, i in enumerate(absurd):
            if np.isnan(S.q[i]).any():
                assert np.all(got[:, i] == np.float32(RS.MAX_RANGE)), S.note[i]
            elif not np.array_equal(S.p[i], S.p[absurd[-1]]):               # the position is the absurd coordinate: only the ground is near
                assert np.array_equal(got[:, i], ground[:, k]), S.note[i]
                if not np.isfinite(S.p[i, 2]) or abs(S.p[i, 2]) >= 1e19:
                    assert np.all(got[:, i] == (0.0 if S.p[i, 2] < 0 else np.float32(RS.MAX_RANGE))), S.note[i]
        assert (got == 0).sum() >= 2 * rays.shape[0] and (got == np.float32(RS.MAX_RANGE)).sum() >= 100
        assert ((got > 0) & (got < np.float32(RS.MAX_RANGE))).sum() >= 100
        assert np.all(got[:, S.of("inside")] == 0.0)
        base_hits = got[:, S.of("base")] < np.float32(RS.MAX_RANGE)
        assert base_hits.any(0).sum() >= 32                                  # the controls hit things
        for i in S.of("graze"):
            assert (got[E.GRAZE_RAY, i] < RS.MAX_RANGE) == ("hit = True" in S.note[i])
        # the finite degenerate classes against the float64 restatement
        # the float64 restatement has no parallel rule: a direction component below fpv_range.h's 1e-12 "never changes its answer" by
        # the header, so the reference takes the two rays of the axis list that hold 1e-13 with a 0 there (what an exact turn leaves
        # of them; under any other attitude the component is far below an ulp of the others)
        rays_ref = np.where(np.abs(rays) < 1e-12, np.float32(0.0), rays)
        left = {}
        for cls in ("tiny", "turn", "surface", "inside", "graze", "cull", "reach"):
            idx = S.of(cls)
            idx = idx[np.abs(S.q[idx]).max(1) > 0.5]                         # (a quaternion holding a denormal is still unit)
            ref, which, keep, scale = RS.restate(S.p[idx], S.q[idx], rays_ref, world)
            err = ulps(got[:, idx], ref, scale)
            # An origin ON the surface of object k (S.on) and a ray that the definition has touch or enter k right there (t_out or
            # t_in is 0: range 0): the fp32 t_out is 0 or an ulp of |oc| below it, and below it the ray has left k at once - it
            # reports 0 or what the world without k gives, nothing else
            for k in np.unique(S.on[idx][S.on[idx] >= 0]):
                at = np.flatnonzero(S.on[idx] == k)
                alt, _, alt_keep, alt_scale = RS.restate(S.p[idx[at]], S.q[idx[at]], rays_ref, without(world, k))
                touching = (ref[:, at] == 0.0) & (which[:, at] == k)
                err[:, at] = np.where(touching, np.minimum(err[:, at], ulps(got[:, idx[at]], alt, alt_scale)), err[:, at])
                keep[:, at] &= alt_keep | ~touching
            assert err[keep].max() <= RANGE_ULP_BOUND, (cls, err[keep].max())
            left[cls] = (int((~keep).sum()), keep.size)
            print(f"range: class {cls}: worst {err[keep].max():.1f} ulp over {int(keep.sum())} of {keep.size} pairs")
        report("range", S, left, "lane-ray pairs")


@pytest.mark.parametrize("res", [(8, 8), (12, 8)])
def test_every_depth_is_finite_and_within_reach_on_every_lane_and_agrees_with_the_restatement(res):
    S = E.lanes()
    course = DS.course(64)
    world = DS.world(8)
    cam = DepthCamera(resolution=res, max_depth=DS.MAX_DEPTH)
    got = cam.evaluate(S.p, S.q, world, course)
    byte = DepthCamera(resolution=res, max_depth=DS.MAX_DEPTH, encoding="u8").evaluate(S.p, S.q, world, course)
    assert got.dtype == np.float32 and np.isfinite(got).all() and (got >= 0).all() and (got <= np.float32(DS.MAX_DEPTH)).all()
    assert byte.dtype == np.uint8 and (byte == 0).any() and (byte == 255).any() and ((byte > 0) & (byte < 255)).any()
    assert np.all(byte[got == np.float32(DS.MAX_DEPTH)] == 0) and np.all(byte[got == 0.0] == 255)
    absurd = S.of("nonfinite", "overflow")
    ground = cam.evaluate(S.p[absurd], S.q[absurd], DS.world(1))
    for k, i in enumerate(absurd):
        if np.isnan(S.q[i]).any():                                           # every ray is NaN and meets nothing
            assert np.all(got[i] == np.float32(DS.MAX_DEPTH)), S.note[i]
        elif not np.array_equal(S.p[i], S.p[absurd[-1]]):                   # the position is the absurd coordinate: only the ground is near
            assert np.array_equal(got[i], ground[k]), S.note[i]
            if not np.isfinite(S.p[i, 2]) or abs(S.p[i, 2]) >= 1e19:
                assert np.all(got[i] == (0.0 if S.p[i, 2] < 0 else np.float32(DS.MAX_DEPTH))), S.note[i]
    assert (got == 0).sum() >= 2 * res[0] * res[1] and ((got > 0) & (got < np.float32(DS.MAX_DEPTH))).sum() >= 100
    levels = [int(byte[i, 7, 3]) for i in S.of("byte") if S.note[i].startswith(str(res))]
    assert sorted(levels) == [100, 101], levels                              # 255 (1 - d / max_depth) either side of the integer 101
    plain = cam.evaluate(S.p, S.q, world)
    assert (got != plain).reshape(S.n, -1).any(1).sum() >= 8                 # gate frames are in the picture of some lanes
    left = {}
    rows = np.asarray(gate_rows(course))
    for cls in ("tiny", "turn", "surface", "inside", "graze", "reach"):
        idx = S.of(cls)
        idx = idx[np.abs(S.q[idx]).max(1) > 0.5]
        ref, which, keep, scale, _ = DS.restate(S.p[idx], S.q[idx], cam, world, rows)
        err = ulps(got[idx], ref, scale)
        # The CAMERA's origin on the surface of object k in fp32 (S.camera_on; p + rel is rounded there, in float64 it is 1e-8 m to
        # one side): every ray goes into k or away from it at the origin - depth 0, or what the world without k gives
        for j in np.flatnonzero(S.camera_on[idx] >= 0):
            alt, _, alt_keep, alt_scale, _ = DS.restate(S.p[idx[j:j + 1]], S.q[idx[j:j + 1]], cam, without(world, S.camera_on[idx[j]]), rows)
            err[j] = np.minimum(np.where(got[idx[j]] == 0.0, 0.0, err[j]), ulps(got[idx[j:j + 1]], alt, alt_scale)[0])
            keep[j] &= alt_keep[0]
        assert err[keep].max() <= DEPTH_ULP_BOUND, (cls, err[keep].max())
        left[cls] = (int((~keep).sum()), keep.size)
        print(f"depth {res}: class {cls}: worst {err[keep].max():.1f} ulp over {int(keep.sum())} of {keep.size} pixels")
    report(f"depth {res}", S, left, "lane-pixel pairs")


# ---- the pursuit task ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pursuit(guide, advance, reset=False):
    S = E.lanes()
    task = E.pursuit_task(guide)
    reward = (np.arange(S.n) * 0.01).astype(np.float32)
    return task, task.evaluate(S.p, S.v, S.q, S.tgt, PT.DT, done=S.done, reward=reward, reset=reset, advance=advance, params=E.params(),
                               pid_state=S.pid if guide else None)


@pytest.mark.parametrize("advance", [True, False])
@pytest.mark.parametrize("guide", [None, ("world", "level"), ("drone", "frontarget")])
def test_pursuit_words_captures_and_nan_discipline(guide, advance):
    S = E.lanes()
    task, o = pursuit(guide, advance)
    words_in, words = S.tgt.view(np.uint32), o["rows"][:, :S.n].view(np.uint32)
    done = S.done.astype(bool)
    event = o["event"].astype(bool)
    assert event.sum() >= 2 and done.sum() >= 10 and not (event & done).any()
    for i in S.of("capture"):
        assert event[i] == ("captured = True" in S.note[i]), S.note[i]
    respawned = event | done
    assert np.all(words[_lib.TGT_COUNT, respawned] & _lib.FPV_TGT_FRESH)
    # the counters: 16 bits each, wrapping; a rebase clears the captures
    sp_in, sp = words_in[_lib.TGT_SPAWNS], words[_lib.TGT_SPAWNS]
    assert np.array_equal(sp & 0xFFFF, (sp_in + respawned) & 0xFFFF)
    assert np.array_equal(sp >> 16, np.where(done, 0, ((sp_in >> 16) + event) & 0xFFFF))
    wrapped = (sp_in == 0xFFFFFFFF) & event
    assert wrapped.sum() >= 2 and np.all(sp[wrapped] == 0)                    # 0xFFFFFFFF wraps to 0 on a capture
    low, high = (sp_in == 0x0000FFFF) & event, (sp_in == 0xFFFF0000) & event   # each half wraps by itself
    assert low.sum() >= 2 and np.all(sp[low] == 0x00010000) and high.sum() >= 2 and np.all(sp[high] == 0x00000001)
    rebased = np.isin(sp_in, (0x0000FFFF, 0xFFFFFFFF)) & done
    assert rebased.sum() >= 2 and np.all(sp[rebased] == 0)                    # a rebase: the respawns wrap, the captures are cleared
    # the path index: K - 1 wraps to 0, a cell that was never set reads index 0
    quiet = ~respawned
    j_in = words_in[_lib.TGT_COUNT] & 0x1FFFF
    j_in = np.where(j_in < E.K_PATH, j_in, 0)
    if advance:
        assert np.array_equal(words[_lib.TGT_COUNT, quiet] & 0x1FFFF, ((j_in + 1) % E.K_PATH)[quiet])
    assert ((j_in == E.K_PATH - 1) & quiet).sum() >= 2 and ((words_in[_lib.TGT_COUNT] & 0x1FFFF >= E.K_PATH) & quiet).sum() >= 4
    if advance:
        assert not (words[_lib.TGT_COUNT, quiet] & _lib.FPV_TGT_FRESH).any()
    else:
        assert np.array_equal(words[_lib.TGT_COUNT, quiet], words_in[_lib.TGT_COUNT, quiet])
    # NaN discipline: outside the five channels every NaN is the constant; inside them another NaN only on a nonfinite / overflow
    # pose or on a PREV_DIST that was seeded non-finite
    assert only_the_constant_nan(o["position"], o["rows"][:5, :S.n])
    if guide:
        assert only_the_constant_nan(o["rotation"], o["thrust"], o["pixel"], o["pid_state"])
        guided = law_rules(S, dict(thrust=o["thrust"], rotation=o["rotation"].reshape(-1, 9), pid=o["pid_state"]), S.pid, restarted=done)
        assert guided.sum() >= 32 and (~guided).sum() >= 2
    may = np.isin(S.cls, ("nonfinite", "overflow")) | ~np.isfinite(S.tgt[_lib.TGT_PREV_DIST])
    for a in (o["obs"], o["paid"], o["reward"], o["rows"][_lib.TGT_PREV_DIST, :S.n]):
        a = np.atleast_2d(a)
        odd = (np.isnan(a) & (np.ascontiguousarray(a).view(np.uint32) != QNAN)).any(0)
        assert not (odd & ~may).any(), (S.cls[odd & ~may], [S.note[i] for i in np.flatnonzero(odd & ~may)])
    # the float64 restatement on the finite lanes whose words it defines (an index below K)
    fin = np.isfinite(S.p).all(1) & np.isfinite(S.v).all(1) & np.isfinite(S.q).all(1) & (np.abs(S.p).max(1) < 1e6) & (np.abs(S.v).max(1) < 1e6)
    fin &= np.isfinite(S.tgt[_lib.TGT_PREV_DIST]) & (words_in[_lib.TGT_COUNT] & 0x1FFFF < E.K_PATH)      # (what is compared does not read q)
    idx = np.flatnonzero(fin)
    R = PT.Restated(task, S.tgt[:, idx], len(idx), PT.DT, 0)
    dist, tol = R.measure(S.p[idx], advance)
    clear = np.abs(dist - task.capture_distance) > 4 * tol                   # the restatement's own margin at the capture threshold
    sel = idx[clear]
    # per class, over every lane of the classes whose inputs the restatement defines (finite, moderate, a path index below K): the classes built on an input that it does not define - nonfinite, overflow, prevdist - are not its to judge, nor
    # is `capture`, two lanes an ulp either side of the threshold that the loop above holds to the fp32 rule itself
    judged = sorted(set(S.cls) - {"nonfinite", "overflow", "prevdist", "capture"})
    cut = {c: (int(len(S.of(c)) - np.isin(S.of(c), sel).sum()), len(S.of(c))) for c in judged}
    # (the garbage COUNT words, index >= K, are compared by the word rules above: they are no lanes of the restatement's)
    cut["word"] = (cut["word"][0] - int(((words_in[_lib.TGT_COUNT] & 0x1FFFF) >= E.K_PATH).sum()), cut["word"][1])
    report(f"pursuit guide={guide} advance={advance}", S, cut)
    assert np.array_equal(o["event"][sel], (~done[sel] & (dist[clear] <= task.capture_distance)).astype(np.uint8))
    unspawned = sel[~respawned[sel]]
    d64 = dict(zip(idx.tolist(), dist.tolist()))
    t64 = dict(zip(idx.tolist(), tol.tolist()))
    for i in unspawned:
        assert abs(float(o["obs"][6, i]) - d64[i]) <= t64[i], (S.cls[i], S.note[i])
        paid = task.progress * (float(S.tgt[_lib.TGT_PREV_DIST, i]) - d64[i])
        assert abs(float(o["paid"][i]) - paid) <= abs(task.progress) * 2 * t64[i] + 4 * PT.EPS * abs(paid), (S.cls[i], S.note[i])


def test_pursuit_reset_call_rebases_the_masked_lanes_only():
    S = E.lanes()
    _, o = pursuit(("world", "level"), True, True)
    mask = S.done.astype(bool)
    rows_in, rows = S.tgt.view(np.uint32), o["rows"][:, :S.n].view(np.uint32)
    assert np.array_equal(rows[:, ~mask], rows_in[:, ~mask]) and not o["paid"].any() and not o["event"].any()
    assert np.all(rows[_lib.TGT_SPAWNS, mask] >> 16 == 0) and np.all(o["pid_state"][3, mask & ~np.isfinite(o["thrust"])] == 1.0)


# ---- the gate step's set -------------------------------------------------------------------------------------------------------------
def test_the_gate_scene_reaches_its_branches_on_the_host():
    p, init, acts, course, words, states, pdone = E.gate_scene()
    rows, out = E.gate_expectation(1)
    kinds = E.gate_kinds()
    w, r, d, o = out[0]
    ev = (w >> 8) & 3
    P0, P1 = states[0, 0:3].T, states[1, 0:3].T
    for k in range(64):
        c, nrm = rows[k, 0:3], rows[k, 3:6]
        s0, s1 = np.float32(nrm @ (P0[k] - c)), np.float32(nrm @ (P1[k] - c))
        if kinds[k] in ("through", "edge", "edge_z", "outside"):
            assert s1 == 0.0 and s0 < 0.0, (k, kinds[k], s0, s1)        # the plane at the post-step position: s1 == 0 exactly
            assert ev[k] in ((1, 3) if kinds[k] != "outside" else (2,)), (k, kinds[k], ev[k])
        elif kinds[k] == "start_on_plane":
            assert s0 == 0.0 and ev[k] == 0, (k, s0, ev[k])
        else:
            assert np.array_equal(P0[k, :2], P1[k, :2]) and s0 == 0.0 and s1 == 0.0 and ev[k] == 0, (k, P0[k], P1[k])
    through = [k for k in range(64) if kinds[k] == "through"]
    top = E.GATE_MAX_PASSED
    assert (w[through[1]] >> 10) == top and (w[through[2]] >> 10) == top          # MAX - 1 counts once more, MAX saturates
    assert ev[through[3]] == 3 and d[through[3]] and ev[through[0]] == 1          # passed = finish_at - 1 on a lane that passes: FINISH
    assert np.all((w[64:80] & 0xFF) < 64)                                         # a garbage word reads gate 0 and leaves with a valid index
