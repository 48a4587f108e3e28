"""The law and sensor kernels on the inputs no flight visits (tests/edge_lanes.py): range scan, depth camera, target chase, point and
shoot, pursuit task and the gate race inside the step, each launched on the whole edge-lane set and once more with the lanes in
reversed order (other wave neighbours for the range cull's and the gate crossing's wave-level branch and for the depth cull's
ballots), and compared with the host function of the same call on the poses read back from the batch: bit for bit, NaN words
included.  Only the pursuit task's five arithmetic channels (obs, paid, the reward and the episode return it is added to, PREV_DIST)
are compared after mapping every NaN to one word: there a NaN is the result of an operation (inf - inf, 0 x inf), whose sign and
payload are the processor's.  Guard words stand behind every output and in the row padding; every optional output is present in one
call and absent in another.  tests/test_edge_lanes_host.py pins, without a GPU, that the set reaches the branches it was built for."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_scene as DS
import edge_lanes as E
import pursuit_task as PT
import range_scene as RS
from fpyv_amd import _lib
from fpyv_amd import rays as RY
from fpyv_amd.camera import DepthCamera
from fpyv_amd.chase import ChaseGuidance
from fpyv_amd.env import DroneBatch
from fpyv_amd.pns import PointAndShoot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1.0e30
ORDERS = ["forward", "reversed"]
bits = E.bits


def order_of(S, order):
    idx = np.arange(S.n)
    return idx if order == "forward" else idx[::-1].copy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def posed(idx, **kw):
    """a batch whose drones stand on the lanes `idx` of the set - written straight into the state rows: a quaternion off the unit
    sphere cannot come out of reset - and the poses read back from it"""
    S = E.lanes()
    n = len(idx)
    b = DroneBatch(E.params(), n, device=DEV, **kw)
    b.reset()
    b.state[:10, :n] = dev(np.concatenate([S.p[idx].T, S.v[idx].T, S.q[idx].T]))
    torch.cuda.synchronize()
    s = b.state[:10, :n].cpu().numpy()
    p, v, q = s[0:3].T.copy(), s[3:6].T.copy(), s[6:10].T.copy()
    assert np.array_equal(bits(p), bits(S.p[idx])) and np.array_equal(bits(q), bits(S.q[idx]))      # the rows hold the lanes' bits
    return b, p, v, q


def guarded(count, dtype=torch.float32, pad=16):
    return torch.full((count + pad,), GUARD if dtype == torch.float32 else 0x5A, dtype=dtype, device=DEV)


def rows(fill, n, ld):
    """[rows, ld] device rows: `fill` [rows, n] in the drones' columns, guard words in the padding"""
    fill = np.atleast_2d(fill)
    t = torch.full((fill.shape[0], ld), GUARD, dtype=torch.float32, device=DEV)
    t[:, :n] = dev(fill.astype(np.float32))
    return t


def same(device_tensor, host, what):
    got = device_tensor.cpu().numpy() if torch.is_tensor(device_tensor) else device_tensor
    g, w = bits(got).reshape(-1), bits(np.asarray(host)).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:6]}: device {g[bad[:6]]} host {w[bad[:6]]}"


# ---- range scan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_range_scan_on_the_edge_lanes(order):
    S = E.lanes()
    idx = order_of(S, order)
    n = S.n
    level = RY.derive(E.level_rays(slice(None)))
    assert (np.abs(level[:, 2]) < np.float32(1e-12)).sum() >= 2 and (np.abs(level[:, 2]) >= np.float32(1e-12)).sum() >= 2
    for ray_set in (E.ray_set(), level):
        b, p, _, q = posed(idx, range_rays=ray_set, range_max=RS.MAX_RANGE)
        ld = (n + 3) // 4 * 4 + 8
        for count in (0, 8):
            world = RS.world(count)
            b._scan_world(world)
            out = torch.full((ray_set.shape[0] + 1, ld), GUARD, dtype=torch.float32, device=DEV)      # a guard row behind the last ray's
            s = _lib.FpvRangeScan.from_buffer_copy(b._scan)
            s.ranges, s.ranges_ld = out.data_ptr(), ld
            b._range_scan_raw(s)
            torch.cuda.synchronize()
            same(out[:-1, :n], RY.evaluate(ray_set, RS.MAX_RANGE, p, q, world), f"ranges, {count} objects, {order}")
            assert bool((out[:, n:] == GUARD).all()) and bool((out[-1] == GUARD).all())


# ---- depth camera ----------------------------------------------------------------------------------------------------------------------
def render(b, cam, p, q, world, course, what):
    n, px = b.n, cam.resolution[0] * cam.resolution[1]
    b._render_world(world)
    fill = 7
    wide = torch.full((n + 1, px + 8), fill, dtype=b.depth.dtype, device=DEV)                        # padding behind every image, a guard image
    r = _lib.FpvDepthRender.from_buffer_copy(b._render)
    r.image, r.image_stride = wide.data_ptr(), px + 8
    b._depth_render_raw(r)
    torch.cuda.synchronize()
    want = cam.evaluate(p, q, world, course)
    got = wide.cpu().numpy()
    same(got[:n, :px].reshape(want.shape), want, what)
    assert (got[:n, px:] == fill).all() and (got[n] == fill).all(), what
    return want


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("res", [(8, 8), (12, 8), (4, 4)])
def test_depth_render_on_the_edge_lanes(res, order):
    S = E.lanes()
    idx = order_of(S, order)
    if res == (4, 4):                                           # 64 lanes of every sensor class: lanes 16..63 of the cull are no live pixels
        pick = np.concatenate([S.of(c)[:k] for c, k in (("base", 8), ("nonfinite", 10), ("overflow", 10), ("tiny", 6), ("quat", 4), ("turn", 8),
                                                        ("surface", 8), ("inside", 4), ("graze", 2), ("cull", 4))])
        assert len(pick) == 64
        idx = pick if order == "forward" else pick[::-1].copy()
    course = DS.course(64)
    for enc in ("metres", "u8"):
        cam = DepthCamera(resolution=res, max_depth=DS.MAX_DEPTH, encoding=enc)
        plain, p, _, q = posed(idx, depth_camera=cam)
        gated, p2, _, q2 = posed(idx, depth_camera=cam, gates=course)
        for count in (0, 8):
            render(plain, cam, p, q, DS.world(count), (), f"depth {res} {enc} {count} objects, {order}")
            with_gates = render(gated, cam, p2, q2, DS.world(count), course, f"depth {res} {enc} {count} objects 64 gates, {order}")
        if enc == "metres":
            assert (with_gates != cam.evaluate(p, q, DS.world(8))).any()        # gate frames are in the picture


# ---- target chase ----------------------------------------------------------------------------------------------------------------------
def chase_call(b, G, n, ld, pid, pixel, optional, tweak=None):
    """one fpv_chase_guide launch on caller-owned, guarded buffers: dict of what the device holds afterwards"""
    rot, thrust, pix, vis = guarded(9 * n), guarded(n), guarded(2 * n), guarded(n, torch.uint8)
    s = G.derive((E.CENTRE, E.RADIUS))
    if tweak:
        tweak(s)
    s.pid_state, s.pid_ld, s.rotation, s.thrust = pid.data_ptr(), ld, rot.data_ptr(), thrust.data_ptr()
    if optional:
        s.pixel_out, s.visible = pix.data_ptr(), vis.data_ptr()
    if pixel is not None:
        s.pixel = pixel.data_ptr()
    b._sensor_raw(b._L.fpv_chase_guide, s, None)
    torch.cuda.synchronize()
    return dict(rot=rot, thrust=thrust, pix=pix, vis=vis)


def check_chase(d, w, n, pid, optional, what):
    same(d["rot"][:9 * n], w["rotation"].reshape(-1), what + ": rotation")
    same(d["thrust"][:n], w["thrust"], what + ": thrust")
    same(pid[:, :n], w["pid"], what + ": PID rows")
    if optional:
        same(d["pix"][:2 * n], w["pixel"].reshape(-1), what + ": pixel")
        same(d["vis"][:n], w["visible"], what + ": visible")
    used = (2 * n, n) if optional else (0, 0)
    assert bool((d["rot"][9 * n:] == GUARD).all()) and bool((d["thrust"][n:] == GUARD).all()) and bool((d["pix"][used[0]:] == GUARD).all()), what
    assert bool((d["vis"][used[1]:] == 0x5A).all()) and bool((pid[:, n:] == GUARD).all()), what


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("frame,mode", E.PAIRS)
def test_chase_on_the_edge_lanes(frame, mode, order):
    S = E.lanes()
    idx = order_of(S, order)
    n, ld = S.n, S.n + 12
    b, p, v, q = posed(idx)
    G = ChaseGuidance(E.params(), ref_frame=frame, mode=mode, max_depth=E.MAX_DEPTH)
    for given in (False, True):
        pid = rows(S.pid[:, idx], n, ld)                         # the rows the caller filled: NaN, inf, denormals, IS_FIRST = 2, -0, NaN
        host_pid = S.pid[:, idx]
        pixel = dev(S.pixel[idx]) if given else None
        for call in range(2):                                   # the PID's first-call branch, then its steady branch
            optional = call == 0
            d = chase_call(b, G, n, ld, pid, pixel, optional)
            w = E.chase_host(G, p, v, q, host_pid, S.pixel[idx] if given else None)
            check_chase(d, w, n, pid, optional, f"chase {frame}/{mode} given={given} call {call} {order}")
            host_pid = w["pid"]
    # F = 0: the mass at 1e-30 kg and the multiplier pinned to 0
    pid = rows(S.pid[:, idx], n, ld)
    d = chase_call(b, G, n, ld, pid, None, True, E.fzero)
    w = E.chase_host(G, p, v, q, S.pid[:, idx], None, E.fzero)
    assert (w["thrust"] == 0.0).sum() >= 3
    check_chase(d, w, n, pid, True, f"chase {frame}/{mode} F = 0 {order}")


# ---- point and shoot -------------------------------------------------------------------------------------------------------------------
# (pixel source, commands given, every optional output, struct change: the last pass is the F = 0 one)
PNS_VARIANTS = [("shared", True, True, None), ("rows", True, False, None), ("pixel", True, True, None), ("pixel", False, False, None),
                ("shared", True, True, E.fzero)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("frame,mode", E.PAIRS)
def test_pns_on_the_edge_lanes(frame, mode, order):
    S = E.lanes()
    idx = order_of(S, order)
    n, ld = S.n, S.n + 12
    b, p, v, q = posed(idx)
    G = PointAndShoot(E.params(), ref_frame=frame, mode=mode, max_depth=E.MAX_DEPTH)
    own, pixel, action, restart = S.own[idx], S.pixel[idx], S.action[idx], S.restart[idx]
    dev_pixel, dev_action, dev_restart = dev(pixel), dev(action), dev(restart)
    for source, commands, optional, tweak in PNS_VARIANTS:
        pid, prev, tgt_rows = rows(S.pid[:, idx], n, ld), rows(S.prev[:, idx], n, ld), rows(own.T, n, ld)
        host_pid, host_prev = S.pid[:, idx], S.prev[:, idx]
        for call in range(2):                                   # two calls in a row: the second sees the first's rows, and the restart bytes
            rot, thrust = guarded(9 * n), guarded(n)
            vel, lim, vis, thr = guarded(2 * n), guarded(n, torch.uint8), guarded(n, torch.uint8), guarded(n)
            s = G.derive()
            if tweak:
                tweak(s)
            s.pid_state, s.pid_ld, s.prev_pixel, s.prev_pixel_ld = pid.data_ptr(), ld, prev.data_ptr(), ld
            s.rotation, s.thrust = rot.data_ptr(), thrust.data_ptr()
            if optional:
                s.pixel_velocity, s.limited, s.visible, s.throttle = vel.data_ptr(), lim.data_ptr(), vis.data_ptr(), thr.data_ptr()
            if source == "shared":
                s.target = E.CENTRE.ctypes.data
            elif source == "rows":
                s.target_rows, s.target_ld = tgt_rows.data_ptr(), ld
            else:
                s.pixel = dev_pixel.data_ptr()
            if commands:
                s.action = dev_action.data_ptr()
            if call == 1:
                s.restart = dev_restart.data_ptr()
            b._sensor_raw(b._L.fpv_pns_guide, s, None)
            torch.cuda.synchronize()
            w = E.pns_host(G, p, v, q, host_pid, host_prev, source, own, pixel, action if commands else None, restart if call == 1 else None, tweak)
            host_pid, host_prev = w["pid"], w["prev"]
            what = f"pns {frame}/{mode} {source} commands={commands} optional={optional} F0={tweak is not None} call {call} {order}"
            same(rot[:9 * n], w["rotation"].reshape(-1), what + ": rotation")
            same(thrust[:n], w["thrust"], what + ": thrust")
            same(pid[:, :n], host_pid, what + ": PID rows")
            same(prev[:, :n], host_prev, what + ": prev_pixel")
            same(tgt_rows[:, :n], own.T, what + ": target rows (read only)")
            used = dict(vel=2 * n, b=n) if optional else dict(vel=0, b=0)
            if optional:
                same(vel[:2 * n], w["velocity"].reshape(-1), what + ": pixel velocity")
                same(thr[:n], w["throttle"], what + ": throttle")
                same(lim[:n], w["limited"], what + ": limited")
                same(vis[:n], w["visible"], what + ": visible")
            for t, k in ((rot, 9 * n), (thrust, n), (vel, used["vel"]), (thr, used["b"])):
                assert bool((t[k:] == GUARD).all()), what
            assert bool((lim[used["b"]:] == 0x5A).all()) and bool((vis[used["b"]:] == 0x5A).all()), what
            for t in (pid, prev, tgt_rows):
                assert bool((t[:, n:] == GUARD).all()), what
        if tweak:
            assert (w["thrust"] == 0.0).sum() >= 3


# ---- pursuit task ----------------------------------------------------------------------------------------------------------------------
class Rig:
    """the batch and caller-owned, guard-filled buffers for everything a pursuit call reads and writes (tests/test_gpu_pursuit.py's)"""

    def __init__(self, idx, guide, advance, optional=True):
        S = E.lanes()
        n = self.n = len(idx)
        ld = self.ld = n + 12
        self.idx, self.optional = idx, optional
        self.task = E.pursuit_task(guide)
        self.b, self.p, self.v, self.q = posed(idx)
        f = lambda shape: torch.full(shape, GUARD, dtype=torch.float32, device=DEV)  # noqa: E731
        u = lambda count: torch.full((count,), 0x5A, dtype=torch.uint8, device=DEV)  # noqa: E731
        self.rows, self.obs, self.pos = f((8, ld)), f((7, ld)), f((3, ld))
        self.rows.view(torch.int32)[:, :n] = dev(S.tgt[:, idx].view(np.int32))
        self.event, self.done = u(n + 16), u(n + 16)
        self.paid, self.reward, self.ep = f((n + 16,)), f((n + 16,)), f((n + 16,))
        self.circle = dev(self.task.circle)
        s = self.s = self.task.derive(PT.DT, advance)
        s.targets, s.targets_ld, s.circle = self.rows.data_ptr(), ld, self.circle.data_ptr()
        if optional:
            s.obs, s.obs_ld, s.position, s.position_ld = self.obs.data_ptr(), ld, self.pos.data_ptr(), ld
            s.event, s.reward_out = self.event.data_ptr(), self.paid.data_ptr()
        self.pid = self.rot = self.thrust = self.pix = self.vis = None
        if guide:
            self.pid, self.rot, self.thrust, self.pix, self.vis = f((4, ld)), f((9 * n + 16,)), f((n + 16,)), f((2 * n + 16,)), u(n + 16)
            self.pid[:, :n] = dev(S.pid[:, idx])
            g = self.g = self.task.chase(E.params())
            g.pid_state, g.pid_ld, g.rotation, g.thrust = self.pid.data_ptr(), ld, self.rot.data_ptr(), self.thrust.data_ptr()
            if optional:
                g.pixel_out, g.visible = self.pix.data_ptr(), self.vis.data_ptr()
            s.guide = C.pointer(g)
        self.buf = _lib.FpvBuffers.from_buffer_copy(self.b._buf)
        self.buf.reward, self.buf.done, self.buf.ep_return = self.reward.data_ptr(), self.done.data_ptr(), self.ep.data_ptr()

    def call(self, flags, step_reward, ep_return, reset):
        n, b = self.n, self.b
        self.reward[:n], self.ep[:n] = dev(step_reward), dev(ep_return)
        if reset:
            mask = None if flags is None else dev(flags.astype(np.uint8))
            rc = b._L.fpv_pursuit_reset(b._handle, C.byref(self.buf), C.byref(self.s), mask.data_ptr() if mask is not None else None, b._stream())
        else:
            self.done[:n] = dev(flags.astype(np.uint8))
            rc = b._L.fpv_pursuit_step(b._handle, C.byref(self.buf), C.byref(self.s), b._stream())
        _lib.check(rc)
        torch.cuda.synchronize()

    def guards_hold(self):
        n, ok = self.n, True
        for t in (self.rows, self.obs, self.pos) + ((self.pid,) if self.pid is not None else ()):
            ok &= bool((t[:, n:] == GUARD).all())
        for t, used in ((self.paid, n), (self.reward, n), (self.ep, n)) + (((self.rot, 9 * n), (self.thrust, n), (self.pix, 2 * n)) if self.rot is not None else ()):
            ok &= bool((t[used:] == GUARD).all())
        for t in (self.event, self.done) + ((self.vis,) if self.vis is not None else ()):
            ok &= bool((t[n:] == 0x5A).all())
        if not self.optional:                                   # an output that was not given holds nothing but guard words
            ok &= bool((self.obs == GUARD).all()) and bool((self.pos == GUARD).all()) and bool((self.paid == GUARD).all()) and bool((self.event == 0x5A).all())
            if self.pix is not None:
                ok &= bool((self.pix == GUARD).all()) and bool((self.vis == 0x5A).all())
        return ok


def same_arithmetic(device_tensor, host, what):
    """a channel that carries arithmetic: bit for bit after mapping every NaN to one word"""
    got = device_tensor.cpu().numpy()
    g, w = E.canonical(got).reshape(-1), E.canonical(host).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:6]}: device {g[bad[:6]]} host {w[bad[:6]]}"


def check_pursuit(rig, want, live, ep_before, rebased, what):
    """the device's rows and outputs against the host's: the five arithmetic channels NaN-canonicalised, everything else bit for bit;
    `live`: the lanes the call touched (a reset call's mask)"""
    n = rig.n
    host_rows = want["rows"][:, :n]
    dist_row = _lib.TGT_PREV_DIST
    others = [r for r in range(8) if r != dist_row]
    same(rig.rows[others][:, :n], host_rows[others], what + ": target rows (words)")
    same_arithmetic(rig.rows[dist_row, :n], host_rows[dist_row], what + ": PREV_DIST")
    same_arithmetic(rig.reward[:n], want["reward"], what + ": reward")
    same_arithmetic(rig.ep[:n], np.where(rebased, ep_before, ep_before + want["paid"]).astype(np.float32), what + ": episode return")
    lv = torch.from_numpy(np.flatnonzero(live)).to(DEV)
    if rig.optional:
        same_arithmetic(rig.obs[:, :n][:, lv], want["obs"][:, live], what + ": obs")
        same_arithmetic(rig.paid[:n][lv], want["paid"][live], what + ": paid")
        same(rig.pos[:, :n][:, lv], want["position"][:, live], what + ": position")
        same(rig.event[:n][lv], want["event"][live], what + ": event")
    if rig.pid is not None:
        same(rig.pid[:, :n], want["pid_state"], what + ": PID rows")
        same(rig.rot[:9 * n].reshape(n, 9)[lv], want["rotation"].reshape(n, 9)[live], what + ": rotation")
        same(rig.thrust[:n][lv], want["thrust"][live], what + ": thrust")
        if rig.optional:
            same(rig.pix[:2 * n].reshape(n, 2)[lv], want["pixel"][live], what + ": pixel")
            same(rig.vis[:n][lv], want["visible"].astype(np.uint8)[live], what + ": visible")
    assert rig.guards_hold(), what


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("advance", [True, False])
@pytest.mark.parametrize("guide", [None, ("world", "level"), ("drone", "frontarget")])
def test_pursuit_on_the_edge_lanes(guide, advance, order):
    S = E.lanes()
    idx = order_of(S, order)
    n = S.n
    done = S.done[idx]
    step_reward, ep = (np.arange(n) * np.float32(0.01)).astype(np.float32), np.linspace(-2, 2, n).astype(np.float32)
    for optional in (True, False):
        rig = Rig(idx, guide, advance, optional)
        host_rows, host_pid = S.tgt[:, idx], (S.pid[:, idx] if guide else None)
        kw = dict(advance=advance, params=E.params())
        # the step call, done bytes on a third of the pose lanes; the word lanes capture, rebase or do neither as they were built
        rig.call(done, step_reward, ep, False)
        want = rig.task.evaluate(rig.p, rig.v, rig.q, host_rows, PT.DT, done=done, reward=step_reward, pid_state=host_pid, **kw)
        check_pursuit(rig, want, np.ones(n, bool), ep, done.astype(bool), f"pursuit step guide={guide} advance={advance} optional={optional} {order}")
        if optional:
            assert want["event"].sum() >= 2
        # a second step on the rows the first one left (respawned targets, advanced counters)
        host_rows, host_pid = want["rows"], want.get("pid_state")
        none = np.zeros(n, np.uint8)
        rig.call(none, step_reward, ep, False)
        want = rig.task.evaluate(rig.p, rig.v, rig.q, host_rows, PT.DT, done=none, reward=step_reward, pid_state=host_pid, **kw)
        check_pursuit(rig, want, np.ones(n, bool), ep, none.astype(bool), f"pursuit step 2 guide={guide} advance={advance} optional={optional} {order}")
        # the reset call with a mask, then with a null mask
        for mask in ((np.arange(n) % 3 == 1), None):
            host_rows, host_pid = want["rows"], want.get("pid_state")
            before = dict(obs=rig.obs.clone(), paid=rig.paid.clone(), rot=None if rig.rot is None else rig.rot.clone())
            rig.call(mask, step_reward, ep, True)
            want = rig.task.evaluate(rig.p, rig.v, rig.q, host_rows, PT.DT, done=mask, reward=step_reward, reset=True, pid_state=host_pid, **kw)
            live = np.ones(n, bool) if mask is None else mask
            what = f"pursuit reset mask={'null' if mask is None else 'every third'} guide={guide} advance={advance} optional={optional} {order}"
            check_pursuit(rig, want, live, ep, np.ones(n, bool), what)
            assert not want["paid"].any() and np.array_equal(want["reward"], step_reward)         # a reset call pays nothing, anywhere
            if mask is not None:                                # outside the mask: every bit as it was
                out = torch.from_numpy(np.flatnonzero(~mask)).to(DEV)
                assert torch.equal(rig.obs[:, out].view(torch.int32), before["obs"][:, out].view(torch.int32)), what
                assert torch.equal(rig.paid[out].view(torch.int32), before["paid"][out].view(torch.int32)), what
                if rig.rot is not None:
                    assert torch.equal(rig.rot[:9 * n].reshape(n, 9)[out].view(torch.int32), before["rot"][:9 * n].reshape(n, 9)[out].view(torch.int32)), what


# ---- the gate race inside the step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_gate_step_on_the_edge_lanes(order):
    p, init, acts, course, words, states, pdone = E.gate_scene()
    n = E.GATE_N
    idx = np.arange(n) if order == "forward" else np.arange(n)[::-1].copy()      # (the words carry the gate's index: lane k keeps ITS gate)
    rows, out = E.gate_expectation(3)
    a = dev(acts[:, idx])
    for steps in (1, 3):
        b = DroneBatch(p, n, device=DEV, gates=course, laps=1)
        b.reset()
        b.state[:, :n] = dev(init[:, :n][:, idx])
        b.gate_word.copy_(dev(words[idx].view(np.int32)))
        if steps == 1:
            b.step(a[0], return_imu=False)
            torch.cuda.synchronize()
            w, r, d, o = out[0]
            same(b.reward, r[idx], f"gate step {order}: reward")
            assert np.array_equal(b.done.cpu().numpy(), d[idx]), f"gate step {order}: done"
        else:
            rew, don = torch.zeros((3, n), device=DEV), torch.zeros((3, n), dtype=torch.bool, device=DEV)
            b.rollout(a, rewards=rew, dones=don)                # one fpv_step_n launch
            torch.cuda.synchronize()
            for t in range(3):
                same(rew[t], out[t][1][idx], f"gate step_n {order}: reward of step {t}")
                assert np.array_equal(don[t].cpu().numpy(), out[t][2][idx]), f"gate step_n {order}: done of step {t}"
            w, r, d, o = out[2]
        same(b.state[:, :n], states[steps][:, idx], f"gate {steps} step(s) {order}: state")
        same(b.gate_word.cpu().numpy().view(np.uint32), w[idx], f"gate {steps} step(s) {order}: word")
        same(b.gate_obs.contiguous(), o[idx], f"gate {steps} step(s) {order}: obs")
