"""What a batch carries besides its drones - the pursuit task, the range sensor, the depth camera, the box detector and the point-cloud
camera, in launch order (`_Batch.attachments`) -, each an `Attachment`: its output tensors, the ctypes struct of its launch with every
pointer that runs over the drones declared once (`_output`), the world it binds before a launch and what it adds to an env's `info`.
A partition launches it with a struct for its own columns: `columns` is the one place where a pointer is moved by a first drone."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional

import torch

from . import _lib, rays as _rays
from .clouds import PointCloud
from .objects import to_rows


def need(attachment: Optional["Attachment"], whose: str, option: str) -> "Attachment":
    if attachment is None:
        raise ValueError(f"this {whose} was built without {option}=")
    return attachment


def columns(struct: C.Structure, steps: Dict[str, int], lo: int, into: Optional[C.Structure] = None) -> C.Structure:
    """`struct` for the drones from column `lo` on: a copy (or `into`, a struct of the same type that keeps its other fields) whose
    pointer fields `steps` - field -> bytes per drone - are `struct`'s moved by `lo` drones.  A pointer that is None stays None."""
    c = type(struct).from_buffer_copy(struct) if into is None else into
    for field, step in steps.items():
        at = getattr(struct, field)
        setattr(c, field, at + lo * step if at else None)
    return c


class Attachment:
    """`struct` what `launch` (a call of the library: handle, buffers, struct, stream) reads; `steps` the pointer fields of `struct`
    that run over the drones (`columns`).  An env launches it after every `every`-th step of a stepper since the last reset (0 = only
    when asked; `option` names the env's argument that sets it, None = every step) and - `after_reset` - after a reset."""
    every, after_reset, option = 1, True, None

    def __init__(self, struct: C.Structure, launch: Any = None):
        self.struct, self.launch, self.steps, self.key = struct, launch, {}, None

    def _output(self, field: str, tensor: torch.Tensor, per_drone: int = 1) -> torch.Tensor:
        """`tensor`, `per_drone` elements for every drone, as what `struct.field` points at"""
        setattr(self.struct, field, tensor.data_ptr())
        self.steps[field] = per_drone * tensor.element_size()
        return tensor

    def columns(self, lo: int) -> C.Structure:                # the struct of a partition that starts at drone `lo`
        return columns(self.struct, self.steps, lo)

    def world_changed(self) -> None:
        """the gates of the batch's course are others than they were: what `bind` cached under `key` is stale"""
        self.key = None

    def bind(self, batch: Any, world: Any, struct: C.Structure) -> None:
        """`world` (what the public call of the batch takes) and the batch's course into `struct`: this attachment's, or a partition's"""

    def _objects(self, batch: Any, object_list: Any) -> Optional[int]:
        """Where the object list of the next scan or render is: given, it is packed into the sensor's own `table` (nothing is bound to the
        steps: a Racer can see a world it does not collide with); None takes what `set_objects` or the last `step` bound."""
        return batch._buf.objects if object_list is None else self.table.address(object_list)

    def run(self, batch: Any, world: Any = None, stepper: Any = None, struct: Optional[C.Structure] = None, stream: Any = None) -> None:
        """One launch for the drones of `stepper` (None: the batch's, with its own struct) on `stream` (None: torch's current one)"""
        struct = self.struct if struct is None else struct
        self.bind(batch, world, struct)
        (batch if stepper is None else stepper)._sensor_raw(self.launch, struct, stream)

    def info(self, batch: Any, lo: int, hi: int) -> Dict[str, torch.Tensor]:
        """what an env's `info` shows of the drones [lo, hi)"""
        return {}


class Pursuit(Attachment):
    """fpv_pursuit_step (fpyv_amd.pursuit.PursuitTask): `rows` [8, ld] a target per drone (read and written by the call after every step
    and reset), `obs_rows` [7, ld], `position_rows` [3, ld], `event` [n] and `reward` [n] its outputs; with guide= `pid_rows` [4, ld] and
    `guidance` = (rotation_matrix [n, 3, 3], thrust_force [n]) of the last call, in the layout the step's override reads.  The call
    after a reset is the batch's own (`_Batch._reset_raw`, with the lanes' mask).  A checkpoint carries what the next call or step
    reads - `rows`, `pid_rows`, `guidance` -, not the outputs."""
    after_reset = False

    def __init__(self, batch: Any, task: Any):
        super().__init__(task.derive(batch.params.dt), batch._L.fpv_pursuit_step)
        n, ld, s, f32 = batch.n, batch.ld, self.struct, dict(dtype=torch.float32, device=batch.device)
        self.rows = self._output("targets", torch.from_numpy(task.rows(n, ld)).to(batch.device))
        self.circle = torch.from_numpy(task.circle).to(batch.device)
        self.position_rows = self._output("position", torch.zeros((3, ld), **f32))
        self.event = self._output("event", torch.zeros(n, dtype=torch.uint8, device=batch.device))
        self.reward = self._output("reward_out", torch.zeros(n, **f32))
        s.targets_ld, s.position_ld, s.circle = ld, ld, self.circle.data_ptr()
        self.obs_rows = self.pid_rows = self.guidance = self.guide = None
        if task.obs:
            self.obs_rows, s.obs_ld = self._output("obs", torch.zeros((_lib.FPV_PURSUIT_OBS, ld), **f32)), ld
        g = task.chase(batch.params)
        if g is not None:
            self.guide = Attachment(g)
            self.pid_rows, g.pid_ld = self.guide._output("pid_state", torch.zeros((_lib.FPV_PID_ROWS, ld), **f32)), ld
            self.pid_rows[_lib.FPV_PID_ROWS - 1] = 1.0                  # is_first: a freshly reset PID
            self.guidance = (self.guide._output("rotation", torch.zeros((n, 3, 3), **f32), 9),
                             self.guide._output("thrust", torch.full((n,), float("nan"), **f32)))
            s.guide = C.pointer(g)
        # set_targets: the same call without a move and without a respawn - it only restarts the distance of the lanes it is given
        self.rebase = _lib.FpvPursuit.from_buffer_copy(s)
        self.rebase.advance = self.rebase.respawn_on_done = 0

    def columns(self, lo: int) -> C.Structure:
        t = super().columns(lo)
        if self.guide is not None:
            t._guide = self.guide.columns(lo)       # (kept alive by the struct that points at it)
            t.guide = C.pointer(t._guide)
        return t

    def info(self, batch: Any, lo: int, hi: int) -> Dict[str, torch.Tensor]:
        return {**({} if self.obs_rows is None else {"target_obs": self.obs_rows[:, lo:hi].t()}), "target_event": self.event[lo:hi],
                "captures": (self.rows[_lib.TGT_SPAWNS, lo:hi].view(torch.int32) >> 16) & 0xFFFF}


class RangeSensor(Attachment):
    """fpv_range_scan: `rays` [R, 3] unit body-frame directions (fpyv_amd.rays.derive of what was given), `rows` [R, ld] the rows a scan
    writes - an output: checkpoints do not carry them"""

    def __init__(self, batch: Any, rays: Any, max_range: float):
        self.rays = _rays.derive(rays)
        super().__init__(_lib.pack_range_scan(self.rays, max_range), batch._L.fpv_range_scan)
        self.rows = self._output("ranges", torch.zeros((self.rays.shape[0], batch.ld), dtype=torch.float32, device=batch.device))
        self.struct.ranges_ld, self.table = batch.ld, _lib.ObjectTable()

    def bind(self, batch: Any, world: Any, struct: C.Structure) -> None:
        struct.objects = self._objects(batch, world)

    def info(self, batch: Any, lo: int, hi: int) -> Dict[str, torch.Tensor]:
        return {"ranges": self.rows[:, lo:hi]}                    # [R, columns] after this step's scan


class DepthSensor(Attachment):
    """fpv_depth_render: `camera` a fpyv_amd.camera.DepthCamera, `image` [num_envs, H, W] float32 or uint8 the images a render writes -
    caller-visible, zero-copy, an output: checkpoints do not carry them"""
    option = "depth_every"

    def __init__(self, batch: Any, camera: Any):
        super().__init__(camera.derive(), batch._L.fpv_depth_render)
        (w, h), u8 = camera.resolution, camera.encoding == "u8"
        self.image = self._output("image", torch.zeros((batch.n, h, w), dtype=torch.uint8 if u8 else torch.float32, device=batch.device), w * h)
        self.struct.image_stride, self.table = w * h, _lib.ObjectTable()

    def bind(self, batch: Any, world: Any, struct: C.Structure) -> None:
        """The object list and the gates of the next render.  A batch with a bound course passes its own descriptor table: gates that
        `set_gates` moved are seen where they are."""
        course = batch._course
        struct.gate_count, struct.gate_descriptors = (int(course.count), batch.gate_desc.data_ptr()) if course is not None else (0, None)
        struct.objects = self._objects(batch, world)

    def info(self, batch: Any, lo: int, hi: int) -> Dict[str, torch.Tensor]:
        return {"depth": self.image[lo:hi]}                       # [columns, H, W] after the last render


class BoxSensor(Attachment):
    """fpv_detect_boxes (fpyv_amd.detect.BoxDetector): `rows` [slots, 4, ld], `depth_rows` [slots, ld] and `visible_rows` [slots, ld]
    bool the rows a detection writes - outputs: checkpoints do not carry them.  `slots` is how many boxes the rows hold: by default the
    most an object list can bring (8), the gates of the course the batch is built with and the own-target slot; how many the last
    detection filled is the batch's `_detect_count`."""
    option = "detect_every"

    def __init__(self, batch: Any, det: Any, slots: Optional[int]):
        own = bool(det.own_target)
        if own and batch._pursuit is None:
            raise ValueError("BoxDetector(own_target=True) needs a batch built with pursuit=: the slot is the drone's own target")
        cap = int(slots) if slots is not None else _lib.FPV_MAX_OBJECTS + len(batch._gate_list or ()) + int(own)
        if not 1 <= cap <= _lib.FPV_MAX_BOXES:
            raise ValueError(f"detect_slots must be 1..{_lib.FPV_MAX_BOXES}")
        super().__init__(det.derive(), batch._L.fpv_detect_boxes)
        ld, f32 = batch.ld, dict(dtype=torch.float32, device=batch.device)
        self.rows = self._output("boxes", torch.zeros((cap, 4, ld), **f32))
        self.depth_rows = self._output("box_depth", torch.zeros((cap, ld), **f32))
        self.visible_rows = self._output("box_visible", torch.zeros((cap, ld), dtype=torch.bool, device=batch.device))   # the kernel writes exactly 0 or 1
        self.struct.ld = ld
        if own:
            self._output("target_rows", batch.target_position_rows)
            self._output("target_radius", batch.target_rows[_lib.TGT_RADIUS])
            self.struct.target_ld = ld
        self.det, self.slots, self.list, self.table = det, cap, [], None

    def bind(self, batch: Any, world: Any, struct: C.Structure) -> None:
        """The box table of the next detection: the collidable entries of `world` (None: the list of the last detection), then the
        gates of the course as `set_gates` last left them.  A world that did not move is not boxed again."""
        if world is not None:
            self.list = list(world)
        if batch._course is not None and batch._gate_list is None:
            raise ValueError("the gate course came from a checkpoint whose gates this batch was not given: call set_gates(gates) before "
                             "detect() (a checkpoint holds the descriptor rows, which do not say what a detection boxes)")
        gates = (batch._gate_list or []) if batch._course is not None else []
        key = (to_rows(self.list), tuple(float(getattr(o, "size", 0.0) or 0.0) for o in self.list), len(gates))
        if key != self.key:
            self.table, self.key = self.det.table(self.list, gates), key
        m = int(self.table.count) + int(self.det.own_target)
        if m > self.slots:
            raise ValueError(f"{m} boxes do not fit the {self.slots} slots of this batch: build it with detect_slots={m}")
        batch._detect_count = m
        struct.table = C.addressof(self.table)

    def info(self, batch: Any, lo: int, hi: int) -> Dict[str, torch.Tensor]:
        m = slice(batch._detect_count)                                     # [M, 4 | -, columns] after the last detection
        return {"boxes": self.rows[m, :, lo:hi], "box_depth": self.depth_rows[m, lo:hi], "box_visible": self.visible_rows[m, lo:hi]}


class CloudSensor(Attachment):
    """fpv_splat_render (fpyv_amd.splat.PointCloudCamera): `image` [num_envs, H, W] uint8 or float32 and - PointCloudCamera(centroid=True)
    - `centroid` [num_envs, 2], `lit` [num_envs]: outputs, not in checkpoints.  The PointCloud of the last render and its points on the
    device are the batch's `_cloud` and `_cloud_dev`."""
    option = "cloud_every"

    def __init__(self, batch: Any, cam: Any):
        super().__init__(cam.derive(), batch._L.fpv_splat_render)
        (w, h), n, dtype = cam.resolution, batch.n, torch.float32 if cam.encoding == "metres" else torch.uint8
        self.image = self._output("image", torch.zeros((n, h, w), dtype=dtype, device=batch.device), w * h)
        self.struct.image_ld, self.centroid, self.lit = w * h, None, None
        if cam.centroid:
            self.centroid = self._output("centroid", torch.zeros((n, 2), dtype=torch.float32, device=batch.device), 2)
            self.lit = self._output("lit", torch.zeros((n,), dtype=torch.int32, device=batch.device))
        self.held = self.cloud_dev_of = None

    def bind(self, batch: Any, world: Any, struct: C.Structure) -> None:
        """The cloud of the next render.  `world` a PointCloud: taken as it is.  An object list: its clouds in list order
        (PointCloud.from_world), then the points of the course's gates as `set_gates` last left them; a list of the same objects as
        last time is not flattened or uploaded again - only the Targets' offsets are read anew (an object whose points changed in place
        needs a new list or a PointCloud).  None: the world of the last render, the empty one if there was none."""
        if isinstance(world, PointCloud):
            batch._cloud, self.key = world, None
        elif world is not None or batch._cloud is None:
            objs = list(world or ())
            gates = (batch._gate_list or []) if batch._course is not None else []
            key = tuple(id(o) for o in objs) + (len(gates),)
            if key != self.key:
                batch._cloud, self.key, self.held = PointCloud.from_world(objs, gates), key, objs
        cloud = batch._cloud
        cloud.refresh()
        if self.cloud_dev_of is not cloud:
            # a new tensor every time: a render in flight on another stream keeps reading the one it was given
            batch._cloud_dev, self.cloud_dev_of = torch.from_numpy(cloud.points).to(batch.device), cloud
        cloud.fill(struct)
        struct.points = batch._cloud_dev.data_ptr()

    def info(self, batch: Any, lo: int, hi: int) -> Dict[str, torch.Tensor]:
        shown = {"points_image": self.image, "points_centroid": self.centroid}         # [columns, H, W | 2] after the last render
        return {key: t[lo:hi] for key, t in shown.items() if t is not None}
