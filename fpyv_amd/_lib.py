"""ctypes binding of libfpv_hip.so (include/fpv_abi.h).

There is exactly one compute path: the HIP library.  If it is missing or does not load, importing
this module's `lib()` raises - there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional


_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfpv_hip.so")

FPV_ABI_VERSION = 9
FPV_OK = 0
FPV_MODE_DRONE, FPV_MODE_RACER = 0, 1
FPV_DRONE_ROWS, FPV_RACER_ROWS = 14, 29
FPV_FLAG_AUTO_RESET = 1
FPV_FLAG_GROUND = 2
FPV_FLAG_FP16_STATE = 4
FPV_FLAG_STICK_NOISE = 8
FPV_FLAG_RESET_JITTER = 16
RESET_POSE_ROWS = 10          # fpv_buffers_t.reset_pose: [10][ld] = p3 v3 q4 (wxyz), the state's row order
FPV_PHYS_ROWS = 13            # fpv_set_physics: [13][ld] derived constants per drone (fpv_abi.h FPV_PHYS_*)
FPV_PHYS_INPUTS = 10          # a parameter set: mass, c3 c2 c1 c0, Cd x y z, rates_transition_rate, thrust_transition_rate
PHYS_IN_MASS, PHYS_IN_C3, PHYS_IN_CD_X, PHYS_IN_RATES_LAG, PHYS_IN_THRUST_LAG = 0, 1, 5, 8, 9
FPV_MAX_GATES = 64            # fpv_set_gates: a course has 1..64 gates
FPV_GATE_FLOATS = 16          # a descriptor row: c3 n3 u3 w3 a hz zc r2 (fpv_abi.h "Gate courses")
GATE_SHAPES = {"rectangle": 0, "circle": 1, "half_circle": 2}
GATE_EVENT_NONE, GATE_EVENT_PASS, GATE_EVENT_MISS, GATE_EVENT_FINISH = 0, 1, 2, 3
GATE_OBS_ROWS = 6
FPV_MAX_RAYS = 32             # fpv_range_scan: a ray set has 1..32 body-frame directions (fpv_abi.h "Range scan")
FPV_DEPTH_MAX_SIDE = 128      # fpv_depth_render: an image is 4..128 pixels wide and high (fpv_abi.h "Depth camera")
DEPTH_ENCODINGS = {"metres": 0, "u8": 1}
FPV_CHASE_MAX_SIDE = 16384    # fpv_chase_guide: no image is written, the camera may be 1..16384 pixels wide and high ("Target chase")
CHASE_FRAMES = {"world": 0, "drone": 1}
CHASE_MODES = {"level": 0, "frontarget": 1}
FPV_TGT_ROWS = 8              # fpv_pursuit_step: targets[8][ld] (fpv_abi.h "Pursuit task")
TGT_CX, TGT_CY, TGT_CZ, TGT_PATH_R, TGT_RADIUS, TGT_PREV_DIST, TGT_COUNT, TGT_SPAWNS = range(8)
FPV_TGT_FRESH = 0x80000000    # bit 31 of the COUNT word: not advanced since it was set or respawned
FPV_PURSUIT_OBS = 7           # rows of the target observation: R^T (t - p), R^T (v_target - v), dist
FPV_PURSUIT_MAX_RESOLUTION = 65536
FPV_HALF_PAIR_ROWS = 5
FPV_HALF_HALVES = 11          # binary16 values per drone in state_h (5 pair rows + 1 half row)
FPV_OBS_AOS_DIM = 16

# state rows (fpv_abi.h)
PX, PY, PZ, VX, VY, VZ, QW, QX, QY, QZ, RX, RY, RZ, THRUST = range(14)
R_OMEGA, R_IERR, R_LERR, R_FIRST, R_OMEGA_LO, R_IERR_LO, R_DFILT = 10, 13, 16, 19, 20, 23, 26

# every symbol include/fpv_abi.h declares
EXPORTS = ("fpv_abi_version", "fpv_sizeof", "fpv_state_rows", "fpv_algorithmic_bytes", "fpv_handle_algorithmic_bytes", "fpv_create", "fpv_destroy",
           "fpv_reset", "fpv_step", "fpv_rollout", "fpv_step_n", "fpv_rollout_graph", "fpv_return_triple", "fpv_widen_state", "fpv_set_params", "fpv_set_step_counter", "fpv_get_step_counter", "fpv_set_rotation", "fpv_get_rotation", "fpv_recommended_ld",
           "fpv_recommended_ld_device", "fpv_check_cache_model", "fpv_device_cache_model", "fpv_get_cache_model",
           "fpv_diag_stream_copy", "fpv_diag_stream_copy_wide", "fpv_diag_busy", "fpv_diag_xcd_map", "fpv_pid_reset", "fpv_pid_call", "fpv_comm_unique_id", "fpv_comm_create", "fpv_comm_destroy", "fpv_comm_info",
           "fpv_allgather_done", "fpv_allgather_f32", "fpv_last_error",
           "fpv_error_name", "fpv_encoding_id", "fpv_reset_pose_sample",
           "fpv_physics_rows", "fpv_physics_derive", "fpv_physics_sample", "fpv_set_physics", "fpv_get_physics",
           "fpv_gates_derive", "fpv_set_gates", "fpv_gate_eval",
           "fpv_rays_derive", "fpv_range_scan", "fpv_range_eval",
           "fpv_camera_derive", "fpv_depth_render", "fpv_depth_eval",
           "fpv_chase_derive", "fpv_chase_guide", "fpv_chase_eval",
           "fpv_pursuit_derive", "fpv_pursuit_sample", "fpv_pursuit_step", "fpv_pursuit_reset", "fpv_pursuit_eval",
           "fpv_pns_derive", "fpv_pns_guide", "fpv_pns_eval",
           "fpv_boxes_derive", "fpv_detect_derive", "fpv_detect_boxes", "fpv_detect_eval",
           "fpv_splat_derive", "fpv_cloud_derive", "fpv_splat_render", "fpv_splat_eval")


class FpvParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32), ("racer_omega_dt", C.c_uint32),
        ("dt", C.c_double), ("gravity", C.c_double), ("mass", C.c_double), ("max_rates", C.c_double),
        ("rates_transition_rate", C.c_double), ("thrust_transition_rate", C.c_double),
        ("thrust_poly", C.c_double * 4),
        ("drag_coefficients", C.c_double * 3), ("cross_section_areas", C.c_double * 3),
        ("air_density", C.c_double),
        ("motor_xy", (C.c_double * 2) * 4),
        ("init_position", C.c_double * 3), ("init_velocity", C.c_double * 3), ("init_quat", C.c_double * 4),
        ("ceiling", C.c_double), ("goal", C.c_double * 3),
        ("racer_mass", C.c_double), ("racer_inertia", C.c_double * 3), ("racer_pid", (C.c_double * 3) * 3),
        ("racer_velocity_damping", C.c_double),
        ("motor_radius", C.c_double), ("ground_spring", C.c_double), ("ground_damping", C.c_double),
        ("noise_transition", C.c_double), ("noise_gain", C.c_double),
        ("noise_seed", C.c_uint64), ("drone_id_offset", C.c_uint64),
        ("racer_pid_variant", C.c_uint32), ("_reserved0", C.c_uint32),
        ("pid_integral_clip", C.c_double), ("pid_min_output", C.c_double), ("pid_max_output", C.c_double),
        ("pid_derivative_transition_rate", C.c_double),
        # ABI 9: FPV_FLAG_RESET_JITTER boxes ([lo row, hi row]) and seed
        ("reset_pos_range", (C.c_double * 3) * 2), ("reset_vel_range", (C.c_double * 3) * 2),
        ("reset_ypr_range_deg", (C.c_double * 3) * 2), ("reset_seed", C.c_uint64),
    ]


FPV_MAX_OBJECTS = 8
OBJ_GROUND, OBJ_CYLINDER, OBJ_SPHERE = 0, 1, 2
FPV_PID_ROWS = 4       # integral, prev_derivative, previous_error, is_first
FPV_COMM_ID_BYTES = 128


class FpvPidParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("_reserved", C.c_uint32), ("kP", C.c_double), ("kI", C.c_double),
                ("kD", C.c_double), ("dt", C.c_double), ("integral_clip", C.c_double), ("min_output", C.c_double),
                ("max_output", C.c_double), ("derivative_transition_rate", C.c_double)]


class FpvObject(C.Structure):
    _fields_ = [("type", C.c_int32), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float),
                ("radius", C.c_float), ("height", C.c_float)]


class FpvObjects(C.Structure):
    _fields_ = [("count", C.c_int32), ("obj", FpvObject * FPV_MAX_OBJECTS)]


def pack_objects(objects) -> FpvObjects:
    """sequence of (type, x, y, z, radius, height) in object_list order -> fpv_objects_t"""
    objs = list(objects)
    if len(objs) > FPV_MAX_OBJECTS:
        raise ValueError(f"at most {FPV_MAX_OBJECTS} collision objects")
    t = FpvObjects()
    t.count = len(objs)
    for k, o in enumerate(objs):
        t.obj[k].type = int(o[0])
        t.obj[k].x, t.obj[k].y, t.obj[k].z = float(o[1]), float(o[2]), float(o[3])
        t.obj[k].radius, t.obj[k].height = float(o[4]), float(o[5])
    return t


class ObjectTable:
    """The fpv_objects_t of an object_list that is given again and again: `address(object_list)` converts the list as `step` does
    (objects.to_rows: `rows`) and packs it only when the rows are not the last call's - a world that did not move is not re-packed."""

    def __init__(self):
        self.rows = self.packed = None

    def address(self, object_list) -> int:
        from .objects import to_rows
        rows = to_rows(object_list)
        if rows != self.rows:
            self.packed, self.rows = pack_objects(rows), rows
        return C.addressof(self.packed)


class FpvBuffers(C.Structure):
    _fields_ = [
        ("state", C.c_void_p), ("ld", C.c_int64), ("action", C.c_void_p), ("reward", C.c_void_p),
        ("done", C.c_void_p), ("done_bits", C.c_void_p), ("accel", C.c_void_p), ("ep_return", C.c_void_p),
        ("ep_length", C.c_void_p), ("last_return", C.c_void_p), ("last_length", C.c_void_p),
        ("wind", C.c_float * 3), ("rounding_seed", C.c_uint32), ("state_h", C.c_void_p),
        ("pos_comp", C.c_void_p), ("noise_state", C.c_void_p), ("action_out", C.c_void_p), ("action_ld", C.c_int64), ("objects", C.c_void_p), ("obs_aos", C.c_void_p),
        ("done_bits_stride", C.c_int64), ("rotation_override", C.c_void_p), ("thrust_override", C.c_void_p),
        ("state_h_thrust", C.c_void_p), ("reset_pose", C.c_void_p),
    ]


def pack_params(p, auto_reset: bool = False, fp16_state: bool = False, stick_noise: bool = False,
                noise_seed: int = 0, drone_id_offset: int = 0) -> FpvParams:
    """DroneParams -> fpv_params_t."""
    s = FpvParams()
    s.struct_size = C.sizeof(FpvParams)
    s.mode = int(p.mode)
    s.flags = ((FPV_FLAG_AUTO_RESET if auto_reset else 0) | (FPV_FLAG_GROUND if getattr(p, "ground", False) else 0)
               | (FPV_FLAG_FP16_STATE if fp16_state else 0) | (FPV_FLAG_STICK_NOISE if stick_noise else 0))
    s.noise_transition = float(getattr(p, "noise_transition", 0.1))
    s.noise_gain = float(getattr(p, "noise_gain", 1.0))
    s.noise_seed, s.drone_id_offset = int(noise_seed) & (2 ** 64 - 1), int(drone_id_offset)
    s.racer_omega_dt = int(bool(p.racer_omega_dt))
    s.dt, s.gravity, s.mass, s.max_rates = float(p.dt), float(p.gravity), float(p.mass), float(p.max_rates)
    s.rates_transition_rate = float(p.rates_transition_rate)
    s.thrust_transition_rate = float(p.thrust_transition_rate)
    s.thrust_poly[:] = [float(x) for x in p.thrust_poly]
    s.drag_coefficients[:] = [float(x) for x in p.drag_coefficients]
    s.cross_section_areas[:] = [float(x) for x in p.cross_section_areas]
    s.air_density = float(p.air_density)
    for m in range(4):
        s.motor_xy[m][0], s.motor_xy[m][1] = float(p.motor_xy[m][0]), float(p.motor_xy[m][1])
    s.init_position[:] = [float(x) for x in p.init_position]
    s.init_velocity[:] = [float(x) for x in p.init_velocity]
    s.init_quat[:] = [float(x) for x in p.init_quat]
    s.ceiling = float(p.ceiling)
    s.goal[:] = [float(x) for x in p.goal]
    s.racer_mass = float(p.racer_mass)
    s.racer_inertia[:] = [float(x) for x in p.racer_inertia]
    for i in range(3):
        for j in range(3):
            s.racer_pid[i][j] = float(p.racer_pid[i][j])
    s.racer_velocity_damping = float(p.racer_velocity_damping)
    s.racer_pid_variant = int(getattr(p, "racer_pid_variant", 0))
    s.pid_integral_clip = float(getattr(p, "pid_integral_clip", 1.0))
    s.pid_min_output = float(getattr(p, "pid_min_output", 0.3))
    s.pid_max_output = float(getattr(p, "pid_max_output", 1.0))
    s.pid_derivative_transition_rate = float(getattr(p, "pid_derivative_transition_rate", 0.5))
    s.motor_radius, s.ground_spring, s.ground_damping = float(p.motor_radius), float(p.ground_spring), float(p.ground_damping)
    # reset jitter (ABI 9): any box that is set turns the flag on; a box left at None is [0, 0]
    boxes = [getattr(p, "reset_position_range", None), getattr(p, "reset_velocity_range", None), getattr(p, "reset_ypr_range_deg", None)]
    if any(b is not None for b in boxes):
        s.flags |= FPV_FLAG_RESET_JITTER
        for dst, box in zip((s.reset_pos_range, s.reset_vel_range, s.reset_ypr_range_deg), boxes):
            if box is not None:
                rows = [[float(x) for x in row] for row in box]
                if len(rows) != 2 or any(len(r) != 3 for r in rows):
                    raise ValueError("a reset range is [2, 3]: a lo row and a hi row of three components")
                for r in range(2):
                    dst[r][:] = rows[r]
    s.reset_seed = int(getattr(p, "reset_seed", 0)) & (2 ** 64 - 1)
    return s


class FpvGate(C.Structure):
    """fpv_gate_t: what fpv_gates_derive reads (the reference's Gate(position, rotation_matrix, size, shape))."""
    _fields_ = [("position", C.c_double * 3), ("rotation", C.c_double * 9), ("size", C.c_double), ("shape", C.c_int32),
                ("_reserved", C.c_int32)]


class FpvGateCourse(C.Structure):
    """fpv_gate_course_t: a course as fpv_set_gates binds it (device pointers) or fpv_gate_eval reads it (host pointers)."""
    _fields_ = [("struct_size", C.c_uint32), ("count", C.c_int32), ("descriptors", C.c_void_p), ("gate_word", C.c_void_p),
                ("gate_obs", C.c_void_p), ("gate_obs_ld", C.c_int64), ("gate_start", C.c_void_p), ("laps", C.c_int32),
                ("miss_is_done", C.c_int32), ("progress_gain", C.c_float), ("pass_bonus", C.c_float), ("finish_bonus", C.c_float),
                ("miss_penalty", C.c_float), ("crash_penalty", C.c_float), ("_reserved", C.c_float)]


GATE_REWARD_DEFAULTS = dict(progress=1.0, passed=10.0, finish=50.0, missed=5.0, crash=10.0)


def pack_course(count: int, laps: int = 0, gate_rewards=None, miss_is_done: bool = False) -> FpvGateCourse:
    """The constants of a course (the pointers are the caller's to fill): gate_rewards = dict(progress=, passed=, finish=,
    missed=, crash=), each defaulting to GATE_REWARD_DEFAULTS."""
    r = dict(GATE_REWARD_DEFAULTS)
    unknown = set(gate_rewards or ()) - set(r)
    if unknown:
        raise ValueError(f"gate_rewards has no {sorted(unknown)}; its keys are {sorted(r)}")
    r.update(gate_rewards or {})
    c = FpvGateCourse()
    c.struct_size, c.count, c.laps, c.miss_is_done = C.sizeof(FpvGateCourse), int(count), int(laps), int(bool(miss_is_done))
    c.progress_gain, c.pass_bonus, c.finish_bonus = float(r["progress"]), float(r["passed"]), float(r["finish"])
    c.miss_penalty, c.crash_penalty = float(r["missed"]), float(r["crash"])
    return c


class FpvRangeScan(C.Structure):
    """fpv_range_scan_t: a ray set, its reach, the rows the ranges go to (device for fpv_range_scan, host for fpv_range_eval) and
    the object list (host memory, read during the call)."""
    _fields_ = [("struct_size", C.c_uint32), ("ray_count", C.c_int32), ("rays", (C.c_float * 3) * FPV_MAX_RAYS), ("max_range", C.c_float),
                ("ranges", C.c_void_p), ("ranges_ld", C.c_int64), ("objects", C.c_void_p)]


def pack_range_scan(rays, max_range: float) -> FpvRangeScan:
    """The constants of a scan (`ranges`, `ranges_ld` and `objects` are the caller's to fill): `rays` [R, 3] float32 as
    fpyv_amd.rays.derive wrote them."""
    rows = [[float(x) for x in r] for r in rays]
    if not 1 <= len(rows) <= FPV_MAX_RAYS or any(len(r) != 3 for r in rows):
        raise ValueError(f"a ray set is [R, 3] with 1 <= R <= {FPV_MAX_RAYS}")
    s = FpvRangeScan()
    s.struct_size, s.ray_count, s.max_range = C.sizeof(FpvRangeScan), len(rows), float(max_range)
    for k, r in enumerate(rows):
        s.rays[k][:] = r
    return s


class FpvCamera(C.Structure):
    """fpv_camera_t: the reference's Camera arguments as fpv_camera_derive reads them."""
    _fields_ = [("pitch_deg", C.c_double), ("relative_position", C.c_double * 3), ("fov_deg", C.c_double), ("width", C.c_int32),
                ("height", C.c_int32)]


class FpvDepthRender(C.Structure):
    """fpv_depth_render_t: what fpv_camera_derive wrote, the reach and the encoding, the images (device for fpv_depth_render, host
    for fpv_depth_eval), the object list (host memory) and the gate table (device / host like the images)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("encoding", C.c_int32),
                ("dir0", C.c_float * 3), ("dir_u", C.c_float * 3), ("dir_v", C.c_float * 3), ("offset", C.c_float * 3),
                ("dir_len_max", C.c_float), ("max_depth", C.c_float), ("gate_frame_width", C.c_float), ("gate_count", C.c_int32),
                ("focal_length", C.c_double), ("relative_rotation", C.c_double * 9), ("image", C.c_void_p), ("image_stride", C.c_int64),
                ("objects", C.c_void_p), ("gate_descriptors", C.c_void_p)]


class FpvChase(C.Structure):
    """fpv_chase_t: the camera numbers fpv_chase_derive wrote, the law's constants, frame and mode, the target, the guidance PID's
    constants and rows, the optional pixels and the outputs (device for fpv_chase_guide, host for fpv_chase_eval)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("ref_frame", C.c_int32), ("mode", C.c_int32),
                ("_reserved", C.c_int32), ("focal_length", C.c_double), ("relative_rotation", C.c_double * 9),
                ("relative_position", C.c_double * 3), ("max_depth", C.c_double), ("mass", C.c_double),
                ("virtual_drag_coefficient", C.c_double), ("virtual_lift_coefficient", C.c_double), ("tof_effective_distance", C.c_double),
                ("keep_distance", C.c_double), ("UWB_sensor_max_range", C.c_double), ("target", C.c_float * 3), ("target_radius", C.c_float),
                ("pid", FpvPidParams), ("pid_state", C.c_void_p), ("pid_ld", C.c_int64), ("pixel", C.c_void_p), ("rotation", C.c_void_p),
                ("thrust", C.c_void_p), ("pixel_out", C.c_void_p), ("visible", C.c_void_p)]


class FpvPns(C.Structure):
    """fpv_pns_t: the camera numbers fpv_chase_derive computes, the law's constants, frame and mode, the thrust limit and the inverse
    thrust polynomial, the guidance PID's constants and rows, the prev_pixel rows, the optional pixels, targets, commands and restart
    bytes, and the outputs (device for fpv_pns_guide, host for fpv_pns_eval; `target` is always host memory)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("ref_frame", C.c_int32), ("mode", C.c_int32),
                ("_reserved", C.c_int32), ("focal_length", C.c_double), ("relative_rotation", C.c_double * 9),
                ("relative_position", C.c_double * 3), ("max_depth", C.c_double), ("mass", C.c_double),
                ("virtual_drag_coefficient", C.c_double), ("virtual_lift_coefficient", C.c_double), ("tof_effective_distance", C.c_double),
                ("max_throttle_in_force", C.c_double), ("thrust2throttle_poly", C.c_double * 4), ("pid", FpvPidParams),
                ("pid_state", C.c_void_p), ("pid_ld", C.c_int64), ("prev_pixel", C.c_void_p), ("prev_pixel_ld", C.c_int64),
                ("pixel", C.c_void_p), ("target", C.c_void_p), ("target_rows", C.c_void_p), ("target_ld", C.c_int64),
                ("action", C.c_void_p), ("restart", C.c_void_p), ("rotation", C.c_void_p), ("thrust", C.c_void_p),
                ("pixel_velocity", C.c_void_p), ("limited", C.c_void_p), ("visible", C.c_void_p), ("throttle", C.c_void_p)]


FPV_MAX_BOXES = FPV_MAX_OBJECTS + FPV_MAX_GATES      # fpv_detect_boxes: the objects of a list, the gates of a course (fpv_abi.h "Object detections")
DETECT_PIXELS = {"int": 0, "float": 1}


class FpvBoxes(C.Structure):
    """fpv_boxes_t: the box table fpv_boxes_derive writes - (min x, y, z, max x, y, z) per slot."""
    _fields_ = [("count", C.c_int32), ("box", (C.c_float * 6) * FPV_MAX_BOXES)]


class FpvDetect(C.Structure):
    """fpv_detect_t: the camera numbers fpv_detect_derive computes, the pixel mode and the clip flag, the box table (host memory),
    the optional per-drone target rows and radii, and the three outputs (device for fpv_detect_boxes, host for fpv_detect_eval)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("pixel_mode", C.c_int32), ("clip", C.c_int32),
                ("_reserved", C.c_int32), ("focal_length", C.c_double), ("relative_rotation", C.c_double * 9),
                ("relative_position", C.c_double * 3), ("table", C.c_void_p), ("target_rows", C.c_void_p), ("target_ld", C.c_int64),
                ("target_radius", C.c_void_p), ("target_radius_all", C.c_float), ("_reserved2", C.c_float), ("boxes", C.c_void_p),
                ("box_depth", C.c_void_p), ("box_visible", C.c_void_p), ("ld", C.c_int64)]


FPV_SPLAT_MAX_POINTS = 1 << 20                      # fpv_splat_t: the points of a cloud (fpv_abi.h "Point-cloud camera")
SPLAT_ENCODINGS = {"metres": 0, "u8": 1, "mask": 2}
CLOUD_GROUND, CLOUD_CYLINDER, CLOUD_GATE = 0, 1, 2


class FpvSplat(C.Structure):
    """fpv_splat_t: the camera numbers fpv_splat_derive computes, max_depth and the encoding, the object tables by value (first,
    offset, box), the SoA points, the image and the optional centroid and lit (device for fpv_splat_render, host for fpv_splat_eval)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("encoding", C.c_int32), ("max_depth", C.c_float),
                ("object_count", C.c_int32), ("focal_length", C.c_double), ("relative_rotation", C.c_double * 9),
                ("relative_position", C.c_double * 3), ("first", C.c_int32 * (FPV_MAX_BOXES + 1)), ("_reserved", C.c_int32),
                ("offset", (C.c_float * 3) * FPV_MAX_BOXES), ("box", (C.c_float * 6) * FPV_MAX_BOXES), ("points", C.c_void_p),
                ("point_ld", C.c_int64), ("image", C.c_void_p), ("image_ld", C.c_int64), ("centroid", C.c_void_p), ("lit", C.c_void_p)]


class FpvPursuit(C.Structure):
    """fpv_pursuit_t: the path table, the rewards, the spawn box and the flags of a pursuit call, the target rows and the optional
    outputs (device for fpv_pursuit_step / _reset, host for fpv_pursuit_eval), and the optional guidance law (a fpv_chase_t)."""
    _fields_ = [("struct_size", C.c_uint32), ("path_resolution", C.c_int32), ("advance", C.c_int32), ("respawn_on_done", C.c_int32),
                ("add_to_reward", C.c_int32), ("_reserved", C.c_int32), ("spawn_seed", C.c_uint64), ("dt", C.c_double),
                ("capture_distance", C.c_double), ("progress", C.c_double), ("capture", C.c_double), ("spawn_lo", C.c_double * 3),
                ("spawn_hi", C.c_double * 3), ("radius_lo", C.c_double), ("radius_hi", C.c_double), ("targets", C.c_void_p),
                ("targets_ld", C.c_int64), ("circle", C.c_void_p), ("obs", C.c_void_p), ("obs_ld", C.c_int64), ("position", C.c_void_p),
                ("position_ld", C.c_int64), ("event", C.c_void_p), ("reward_out", C.c_void_p), ("guide", C.POINTER(FpvChase))]


class FpvCacheModel(C.Structure):
    """fpv_cache_model_t: what a device says about itself, held against the cache model of the rotation / row stride."""
    _fields_ = [("struct_size", C.c_uint32), ("matches", C.c_int32), ("compute_units", C.c_int32), ("xcds", C.c_int32),
                ("l2_bytes_per_xcd", C.c_int64), ("infinity_cache_bytes", C.c_int64), ("arch", C.c_char * 64), ("reason", C.c_char * 256)]

    def as_dict(self):
        return {"matches": bool(self.matches), "arch": self.arch.decode(), "compute_units": int(self.compute_units), "xcds": int(self.xcds),
                "l2_bytes_per_xcd": int(self.l2_bytes_per_xcd), "infinity_cache_bytes": int(self.infinity_cache_bytes),
                "reason": self.reason.decode() or None}


class FpvError(RuntimeError):
    def __init__(self, code: int, name: str, msg: str):
        super().__init__(f"{name} ({code}): {msg}")
        self.code, self.name = code, name


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libfpv_hip.so (once).  torch is imported first so that the HIP runtime torch ships
    (same SONAME, libamdhip64.so.7) is the one both sides use - one runtime, shared streams and
    device pointers."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  fpyv_amd has no CPU fallback.")
    import torch  # noqa: F401  (loads libamdhip64 / libhsa-runtime64 from torch/lib)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)
    vp, i64, pp, pb = C.c_void_p, C.c_int64, C.POINTER(FpvParams), C.POINTER(FpvBuffers)
    L.fpv_abi_version.restype = C.c_int
    L.fpv_state_rows.argtypes = [C.c_int]
    L.fpv_algorithmic_bytes.argtypes = [C.c_int]
    L.fpv_handle_algorithmic_bytes.argtypes = [vp]
    L.fpv_create.argtypes = [pp, i64, C.c_int, C.POINTER(vp)]
    L.fpv_destroy.argtypes = [vp]
    L.fpv_destroy.restype = None
    L.fpv_reset.argtypes = [vp, pb, vp, vp, vp, vp, vp]
    L.fpv_step.argtypes = [vp, pb, vp]
    L.fpv_rollout.argtypes = [vp, pb, C.c_int, i64, i64, vp]
    L.fpv_rollout_graph.argtypes = [vp, pb, C.c_int, i64, i64, vp]
    L.fpv_step_n.argtypes = [vp, pb, C.c_int, i64, i64, vp]
    L.fpv_return_triple.argtypes = [vp, pb, vp, vp, vp, vp]
    L.fpv_widen_state.argtypes = [vp, pb, vp, i64, vp]
    L.fpv_set_params.argtypes = [vp, pp]
    L.fpv_set_step_counter.argtypes = [vp, C.c_uint64]
    L.fpv_get_step_counter.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.fpv_set_rotation.argtypes = [vp, C.c_int64]
    L.fpv_get_rotation.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fpv_recommended_ld.argtypes = [i64]
    L.fpv_recommended_ld.restype = i64
    L.fpv_recommended_ld_device.argtypes = [i64, C.c_int]
    L.fpv_recommended_ld_device.restype = i64
    L.fpv_check_cache_model.argtypes = [C.c_char_p, C.c_int, i64, C.POINTER(FpvCacheModel)]
    L.fpv_device_cache_model.argtypes = [C.c_int, C.POINTER(FpvCacheModel)]
    L.fpv_get_cache_model.argtypes = [vp, C.POINTER(FpvCacheModel)]
    L.fpv_diag_stream_copy.argtypes = [vp, vp, i64, vp]
    L.fpv_diag_stream_copy_wide.argtypes = [vp, vp, i64, vp]
    L.fpv_diag_busy.argtypes = [C.c_double, vp]
    L.fpv_diag_xcd_map.argtypes = [vp, i64, vp]
    L.fpv_comm_unique_id.argtypes = [vp]
    L.fpv_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.fpv_comm_destroy.argtypes = [vp]
    L.fpv_comm_destroy.restype = None
    L.fpv_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fpv_allgather_done.argtypes = [vp, vp, vp, i64, vp]
    L.fpv_allgather_f32.argtypes = [vp, vp, vp, i64, vp]
    L.fpv_pid_reset.argtypes = [vp, i64, i64, vp, C.c_int, vp]
    L.fpv_pid_call.argtypes = [C.POINTER(FpvPidParams), vp, i64, i64, vp, vp, C.c_float, vp, vp, C.c_int, vp]
    L.fpv_last_error.restype = C.c_char_p
    L.fpv_error_name.argtypes = [C.c_int]
    L.fpv_error_name.restype = C.c_char_p
    L.fpv_encoding_id.argtypes = [C.c_int]
    L.fpv_encoding_id.restype = C.c_char_p
    L.fpv_sizeof.argtypes = [C.c_int]
    L.fpv_reset_pose_sample.argtypes = [pp, C.c_uint64, C.c_uint64, C.c_int, vp, vp]
    L.fpv_physics_rows.restype = C.c_int
    L.fpv_physics_derive.argtypes = [pp, i64, vp, vp, i64]
    L.fpv_physics_sample.argtypes = [pp, C.c_uint64, C.c_uint64, i64, vp, vp]
    L.fpv_set_physics.argtypes = [vp, vp, i64]
    L.fpv_get_physics.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.fpv_gates_derive.argtypes = [C.c_int, vp, vp]
    L.fpv_set_gates.argtypes = [vp, C.POINTER(FpvGateCourse)]
    L.fpv_gate_eval.argtypes = [C.POINTER(FpvGateCourse), i64, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.fpv_rays_derive.argtypes = [C.c_int, vp, vp]
    L.fpv_range_scan.argtypes = [vp, pb, C.POINTER(FpvRangeScan), vp]
    L.fpv_range_eval.argtypes = [C.POINTER(FpvRangeScan), i64, vp, vp]
    L.fpv_camera_derive.argtypes = [C.POINTER(FpvCamera), C.POINTER(FpvDepthRender)]
    L.fpv_depth_render.argtypes = [vp, pb, C.POINTER(FpvDepthRender), vp]
    L.fpv_depth_eval.argtypes = [C.POINTER(FpvDepthRender), i64, vp, vp]
    L.fpv_chase_derive.argtypes = [C.POINTER(FpvCamera), C.POINTER(FpvChase)]
    L.fpv_chase_guide.argtypes = [vp, pb, C.POINTER(FpvChase), vp]
    L.fpv_chase_eval.argtypes = [C.POINTER(FpvChase), i64, vp, vp, vp]
    L.fpv_pursuit_derive.argtypes = [C.c_int32, vp]
    L.fpv_pursuit_sample.argtypes = [C.POINTER(FpvPursuit), C.c_uint64, C.c_uint32, vp, C.POINTER(C.c_uint32)]
    L.fpv_pursuit_step.argtypes = [vp, pb, C.POINTER(FpvPursuit), vp]
    L.fpv_pursuit_reset.argtypes = [vp, pb, C.POINTER(FpvPursuit), vp, vp]
    L.fpv_pursuit_eval.argtypes = [C.POINTER(FpvPursuit), i64, C.c_uint64, vp, vp, vp, vp, vp, C.c_int]
    L.fpv_pns_derive.argtypes = [C.POINTER(FpvCamera), C.POINTER(FpvPns)]
    L.fpv_pns_guide.argtypes = [vp, pb, C.POINTER(FpvPns), vp]
    L.fpv_pns_eval.argtypes = [C.POINTER(FpvPns), i64, vp, vp, vp]
    L.fpv_boxes_derive.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(FpvBoxes)]
    L.fpv_detect_derive.argtypes = [C.POINTER(FpvCamera), C.POINTER(FpvDetect)]
    L.fpv_detect_boxes.argtypes = [vp, pb, C.POINTER(FpvDetect), vp]
    L.fpv_detect_eval.argtypes = [C.POINTER(FpvDetect), i64, vp, vp]
    L.fpv_splat_derive.argtypes = [C.POINTER(FpvCamera), C.POINTER(FpvSplat)]
    L.fpv_cloud_derive.argtypes = [C.c_int, vp, vp, vp, i64]
    L.fpv_splat_render.argtypes = [vp, pb, C.POINTER(FpvSplat), vp]
    L.fpv_splat_eval.argtypes = [C.POINTER(FpvSplat), i64, vp, vp]
    if L.fpv_abi_version() != FPV_ABI_VERSION:
        raise ImportError(f"libfpv_hip.so ABI {L.fpv_abi_version()} != binding {FPV_ABI_VERSION} - rebuild the library "
                          "(`python -c 'import __graft_entry__ as g; g.build()'`)")
    for which, struct in ((0, FpvParams), (1, FpvBuffers), (2, FpvObjects), (3, FpvPidParams), (4, FpvCacheModel), (5, FpvGateCourse),
                          (6, FpvRangeScan), (7, FpvDepthRender), (8, FpvChase), (10, FpvPursuit), (12, FpvPns), (14, FpvDetect),
                          (16, FpvBoxes), (18, FpvSplat)):
        if L.fpv_sizeof(which) != C.sizeof(struct):
            raise ImportError(f"{struct.__name__}: ctypes declares {C.sizeof(struct)} bytes, libfpv_hip.so has "
                              f"{L.fpv_sizeof(which)} - _lib.py and include/fpv_abi.h are out of step")
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        L = lib()
        raise FpvError(rc, L.fpv_error_name(rc).decode(), L.fpv_last_error().decode())
    return rc


def state_rows(mode: int) -> int:
    return FPV_DRONE_ROWS if mode == FPV_MODE_DRONE else FPV_RACER_ROWS


def algorithmic_bytes(mode: int) -> int:
    """state read + write, action read, reward + done write (fpv_algorithmic_bytes): the SURVEY 8d
    figures, 133 B for the drone and 181 B for the 20 base rows of the Racer; a live handle reports
    what its kernel variant really moves (fpv_handle_algorithmic_bytes)."""
    return (FPV_DRONE_ROWS if mode == FPV_MODE_DRONE else 20) * 8 + 16 + 4 + 1
