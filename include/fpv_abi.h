/*
 * fpv_abi.h - C ABI of the MI355X batched FPV drone stepper (libfpv_hip.so).
 *
 * The reference has no FFI for this path: its boundary is the Python method pair
 *   Drone.reset(position, velocity, ypr)                 /root/reference/src/utils/components.py:150-169
 *   Drone.step(action, wind_velocity_vector, object_list) /root/reference/src/utils/components.py:220-248
 * (plus Racer.reset/step, /root/reference/tests/racer_drone_test.py:85-103).  The entry points
 * below are what a ctypes binding of that pair calls for N drones at once; each one names the
 * reference lines it replaces.  Plain pointers and sizes only - no torch, no C++ types.
 *
 * Conventions
 *   - every function returns FPV_OK (0) or a negative FPV_E* code; fpv_last_error() gives the
 *     message of the calling thread's last failure.  Nothing throws across the boundary.
 *   - device buffers are owned by the caller (the Python host allocates them as torch tensors);
 *     the library never allocates, frees or copies device state.
 *   - `stream` is a hipStream_t (NULL = default stream).  Calls only enqueue work; asynchronous
 *     kernel faults surface at the caller's next synchronisation.
 *   - a handle is bound to one device and is not thread-safe; use one per GPU / host thread.  Every call makes the
 *     handle's device current for its own launches and restores the caller's current device before returning.
 */
#ifndef FPV_ABI_H
#define FPV_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: 64-bit step counter (fpv_set_step_counter takes uint64_t, fpv_get_step_counter added; the stick-noise stream is
 *    unchanged below 2^32 steps and no longer repeats beyond); fpv_set_tuning removed (2 / 4 drones per lane and
 *    256-thread workgroups lost every measurement); fpv_comm_info added; fpv_step_n reads action rows only. */
/* 5: fpv_diag_busy added (a time-bounded one-wave kernel: lets a host tell whether two streams sit on different
 *    hardware queues - the split-phase API picks its partition streams that way); the in-kernel stick-noise generator
 *    rebuilt for cost (Philox4x32-7, four normals per call from a table-driven inverse CDF - no logarithm): streams differ from ABI <= 4 (the reference's profile is
 *    unseeded, /root/reference/tests/noise_smooth_test.py:6-12: there never was a stream to stay compatible with). */
/* 6: fpv_buffers_t.action_f16 / reserved0 (binary16 stick rows, added late in ABI 5) removed: measured at no time gain
 *    for ten more kernels - a half-precision policy casts its sticks (`.float()`); sizeof(fpv_buffers_t) shrinks by 8.
 *    fp16 state: the stored quaternion fields saturate at +-16383 instead of wrapping (unit quaternions: unchanged bits). */
/* 7: fpv_set_rotation / fpv_get_rotation added: the fp32 drone step kernels walk the population from a start block that moves
 *    back by a cache's worth of drones per launch - the L2s' when the state overflows them (2^20 drones: 11 % less time), the
 *    Infinity Cache's beyond that (2^23 drones: up to 25 % less) - same results; automatic by default. */
/* 8: the cache model behind the rotation and the row stride is CHECKED against the device (hipGetDeviceProperties at fpv_create):
 *    fpv_check_cache_model / fpv_device_cache_model / fpv_get_cache_model / fpv_recommended_ld_device added.  A device that is not
 *    gfx950 with 256 compute units and a 4 MiB L2 per XCD (e.g. a CPX compute partition) gets the plain order and the
 *    conservative stride - same results.  Every single-step kernel rotates (drone fp32 / fp16 state / AoS head / Racer), as ABI 7
 *    already did; its comment said "fp32 drone" only.  fpv_encoding_id added (what a checkpoint's fp16 words / noise stream mean). */
/* 9: reset sources for drone mode - a per-lane reset-pose table (fpv_buffers_t.reset_pose) and a seeded uniform jitter of the
 *    reset pose (FPV_FLAG_RESET_JITTER, fpv_params_t.reset_*_range / reset_seed, appended); fpv_reset_pose_sample added.
 *    Nothing changes for a handle that configures neither (state layout, streams and checkpoints of ABI 5-8 included). */
#define FPV_ABI_VERSION 9

enum {
    FPV_OK = 0,
    FPV_EINVAL = -1,  /* bad argument (null pointer, n <= 0, bad mode, struct_size mismatch) */
    FPV_EHIP = -2,    /* a HIP runtime call failed; message carries hipGetErrorString */
    FPV_ENODEV = -3,  /* no usable GPU / device index out of range */
    FPV_EALIGN = -4,  /* buffer alignment or leading dimension violates the layout rules */
    FPV_EPARAM = -5   /* physically meaningless parameter (dt <= 0, mass <= 0, ...) */
};

enum { FPV_MODE_DRONE = 0, FPV_MODE_RACER = 1 };

/* Rows of the SoA state matrix state[rows][ld] (fp32).  Row r of drone i is state[r*ld + i].
 * FPV_MODE_DRONE: the mutable state of Drone (components.py:151-169) with the attitude held as a
 * unit quaternion (w,x,y,z), body->world, instead of the 3x3 matrix. */
enum {
    FPV_PX = 0, FPV_PY, FPV_PZ,          /* state[0:3]   position, m                     */
    FPV_VX, FPV_VY, FPV_VZ,              /* state[3:6]   velocity, m/s                   */
    FPV_QW, FPV_QX, FPV_QY, FPV_QZ,      /* rotation_matrix as quaternion                */
    FPV_RX, FPV_RY, FPV_RZ,              /* prev_rates, deg/s (components.py:189)        */
    FPV_THRUST,                          /* prev_thrust, N    (components.py:194)        */
    FPV_DRONE_ROWS                       /* = 14 */
};
/* FPV_MODE_RACER: Racer state (racer_drone_test.py:70-83) + its three PID integrators (:13-20). */
enum {
    FPV_R_OMEGA = 10,                    /* rows 10..12 angular_velocity                 */
    FPV_R_IERR = 13,                     /* rows 13..15 PID i_error                      */
    FPV_R_LERR = 16,                     /* rows 16..18 PID last_error                   */
    FPV_R_FIRST = 19,                    /* 1.0 until the first PID step                 */
    FPV_R_OMEGA_LO = 20,                 /* rows 20..22 low words of angular_velocity: Racer.step AS WRITTEN turns by
                                            omega RADIANS per step (racer_drone_test.py:99), so omega is carried as an
                                            fp32 (hi, lo) pair; unused (never read or written) with racer_omega_dt = 1 */
    FPV_R_IERR_LO = 23,                  /* rows 23..25 low words of the PID i_error, same reason                */
    FPV_R_DFILT = 26,                    /* rows 26..28 prev_derivative of components.PID (components.py:50); only
                                            touched with racer_pid_variant = 1                                   */
    FPV_RACER_ROWS = 29
};

enum {
    FPV_FLAG_AUTO_RESET = 1u,   /* re-initialise a lane in-kernel when it reports done */
    FPV_FLAG_GROUND = 2u,       /* ground plane z = 0 in object_list: per-motor spring contact,
                                   Drone.handle_collisions with a Ground object (components.py:198-214) */
    FPV_FLAG_STICK_NOISE = 8u,  /* drone mode, fp32 state: the kernel advances an EMA-smoothed Gaussian stick noise
                                   per drone and channel (the profile of tests/noise_smooth_test.py:6-12, Philox4x32-7 + a table-driven inverse normal CDF,
                                   keyed by seed / global drone id / step) and ADDS gain * noise to the action
                                   (clipped to [-1,1]); fpv_buffers_t.action may then be NULL (pure noise sticks) */
    FPV_FLAG_RESET_JITTER = 16u,/* drone mode: every reset (fpv_reset and the in-kernel auto-reset) adds a uniform jitter to its base
                                   pose (fpv_params_t.reset_*; "Reset sources" below) */
    FPV_FLAG_FP16_STATE = 4u    /* drone mode only: v, q, prev_rates, prev_thrust stored as eleven 16-bit words per drone in
                                   fpv_buffers_t.state_h; fpv_buffers_t.state holds only the 3 position rows in
                                   fp32; arithmetic stays fp32 (BASELINE config 4) */
};
/* state_h under FPV_FLAG_FP16_STATE: FPV_HALF_PAIR_ROWS rows of ld 32-bit word pairs (low 16 bits first):
 * (vx,vy) (vz,v_low) (qa,qb) (qc,rx) (ry,rz), followed by ONE row of ld single halves holding prev_thrust:
 * (FPV_HALF_PAIR_ROWS * 2 + 1) * ld 16-bit words in all, 22 bytes per drone.  Encoding (ABI 5; csrc/fpv_math.h,
 * fpv_pack_half / fpv_unpack_half; fpv_widen_state decodes a whole batch):
 *   vx vy vz rx ry rz thrust   IEEE binary16 (v: round toward zero of the stochastically rounded value; rates / thrust: nearest even)
 *   v_low                      bits 0-4 / 5-9 / 10-14: the next five mantissa bits of vx / vy / vz (v has 15 mantissa bits in all)
 *   qa qb qc                   "smallest three": bits 0-14 = 15-bit two's-complement fixed point, value / 23168, of the three
 *                              quaternion components that are NOT the largest in magnitude, in w x y z order; bit 15 of qa and
 *                              of qb = bits 0 and 1 of the index of the dropped component, which is positive and equals
 *                              sqrt(1 - qa^2 - qb^2 - qc^2); stochastically rounded.
 * The kernel never issues a 2-byte access: the two lanes of an even/odd drone pair share the dword of the thrust row and
 * exchange their halves in registers. */
#define FPV_HALF_PAIR_ROWS 5
#define FPV_HALF_ROWS_TOTAL_HALVES 11    /* halves per drone in state_h */
#define FPV_OBS_AOS_DIM 16

/* Host-side description of one drone type; doubles, narrowed to fp32 by fpv_create.
 * Field sources: components.py:92-100 (dt, gravity, mass, drag, areas), :120-125 (motor_xy),
 * :134-136 (thrust_poly), :185-194 (max_rates, transition rates), kinematics.py:33 (air_density),
 * racer_drone_test.py:8,:70-83,:102 (racer_*). */
typedef struct fpv_params {
    uint32_t struct_size;             /* = sizeof(fpv_params_t) */
    uint32_t mode;                    /* FPV_MODE_* */
    uint32_t flags;                   /* FPV_FLAG_* */
    uint32_t racer_omega_dt;          /* 0: rotate by omega per step as the reference writes it; 1: omega*dt */
    double dt;
    double gravity;
    double mass;                      /* kg */
    double max_rates;                 /* deg/s */
    double rates_transition_rate;
    double thrust_transition_rate;
    double thrust_poly[4];            /* c3,c2,c1,c0 of thrust[N] over throttle percent */
    double drag_coefficients[3];
    double cross_section_areas[3];    /* m^2 */
    double air_density;
    double motor_xy[4][2];            /* body-frame motor positions (z = 0), m */
    double init_position[3];          /* used by fpv_reset defaults and FPV_FLAG_AUTO_RESET */
    double init_velocity[3];
    double init_quat[4];              /* w,x,y,z */
    double ceiling;                   /* auto-reset when |z| > ceiling; +inf disables */
    double goal[3];                   /* reward = -|p - goal| (build-defined; the reference has none) */
    double racer_mass;
    double racer_inertia[3];
    double racer_pid[3][3];           /* [axis][kP,kI,kD] */
    double racer_velocity_damping;
    double motor_radius;              /* contact starts at distance < motor_radius (components.py:121), m */
    double ground_spring;             /* N/m   (handle_collisions default 100, components.py:198) */
    double ground_damping;            /* N s/m (handle_collisions default 0) */
    double noise_transition;          /* FPV_FLAG_STICK_NOISE: x_s <- (1-tau) x_s + tau N(0,1); noise_smooth_test.py:5 uses 0.1 */
    double noise_gain;                /* sticks += noise_gain * x_s */
    uint64_t noise_seed;              /* Philox key */
    uint64_t drone_id_offset;         /* global id of this handle's drone 0 (shard offset): streams are keyed by global id */
    /* FPV_MODE_RACER rate loop semantics.  0: PID.step of tests/racer_drone_test.py:22-32 (error = desired - actual,
     * plain integral, raw derivative); 1: PID.__call__ of src/utils/components.py:43-54 (error = current - target,
     * integral <- clip(0.99*integral + error*dt, +-integral_clip), derivative clipped to +-1 then low-passed with
     * derivative_transition_rate, output clipped to [min_output, max_output]); gains come from racer_pid either way */
    uint32_t racer_pid_variant;
    uint32_t _reserved0;
    double pid_integral_clip;         /* components.py:16 defaults: 1 */
    double pid_min_output;            /*                            0.3 */
    double pid_max_output;            /*                            1 */
    double pid_derivative_transition_rate;   /*                     0.5 */
    /* FPV_FLAG_RESET_JITTER (ABI 9): uniform boxes [lo row, hi row] added to the base pose of every reset (position m,
     * velocity m/s, roll/pitch/yaw deg applied in the body frame); finite with lo <= hi (else FPV_EPARAM), narrowed to fp32 as
     * lo and span = hi - lo (computed in double).  Unused without the flag. */
    double reset_pos_range[2][3];
    double reset_vel_range[2][3];
    double reset_ypr_range_deg[2][3];
    uint64_t reset_seed;              /* Philox key of the jitter */
} fpv_params_t;

/* Analytic collision objects = the reference's object_list (components.py:198-214) in list order.
 * Ground: plane z = 0 (components.py:646-680); Cylinder: axis along +z from (x,y,z), radius, height
 * (:685-729); Sphere: a Target (:753-778) - update x,y,z before each step for a moving target
 * (simulator.py:87).  Gates and the Trail never collide in the reference (:202) and have no entry. */
#ifndef FPV_MAX_OBJECTS
#define FPV_MAX_OBJECTS 8
#endif
enum { FPV_OBJ_GROUND = 0, FPV_OBJ_CYLINDER = 1, FPV_OBJ_SPHERE = 2 };
typedef struct fpv_object { int32_t type; float x, y, z, radius, height; } fpv_object_t;
typedef struct fpv_objects { int32_t count; fpv_object_t obj[FPV_MAX_OBJECTS]; } fpv_objects_t;

/* Device buffers of one batch.  Only `state` is mandatory for fpv_reset; `state` and `action`
 * for fpv_step.  NULL optional pointers skip that output. */
typedef struct fpv_buffers {
    float* state;            /* [rows][ld] SoA, 16-byte aligned */
    int64_t ld;              /* row stride in floats, >= n, multiple of 4 */
    const float* action;     /* [n][4] = roll, pitch, yaw, throttle per drone (components.py:181-186), 16-byte aligned;
                                or, when action_ld > 0, SoA [4][action_ld] */
    float* reward;           /* [n] */
    uint8_t* done;           /* [n] one byte per drone, exactly 0 or 1 (Drone.done, components.py:236-240): a C99 bool /
                                numpy.bool_ / torch.bool array can be passed as it is */
    uint64_t* done_bits;     /* [ceil(n/64)] bit i%64 of word i/64 = done[i]; 8-byte aligned */
    float* accel;            /* [3][ld] R_new @ acc, the third value Drone.step returns (components.py:248) */
    float* ep_return;        /* [n] running episode return (read-modify-write) */
    int32_t* ep_length;      /* [n] running episode length */
    float* last_return;      /* [n] written when a lane reports done */
    int32_t* last_length;    /* [n] */
    float wind[3];           /* wind_velocity_vector of this step (kinematics.py:35: ADDED to v) */
    uint32_t rounding_seed;  /* FPV_FLAG_FP16_STATE: mixed with the handle's 64-bit step counter for the stochastic rounding
                                (step t of the handle rounds with rounding_seed + t, the counter's high word folded in) */
    uint16_t* state_h;       /* FPV_FLAG_FP16_STATE: [FPV_HALF_PAIR_ROWS][ld] word pairs (4 bytes each) + [ld] thrust halves
                                (encoding above), 8-byte aligned; else unused */
    float* pos_comp;         /* [6][ld] Kahan compensation of the p and v accumulations, or NULL (plain fp32 sums).
                                Keeps p, v within ~1 ulp over 10^4+ steps (config 1); +48 B per env-step; drone mode,
                                fp32 state; combines with stick noise and objects, not with obs_aos */
    float* noise_state;      /* FPV_FLAG_STICK_NOISE: [4][ld] EMA stick-noise state (read-modify-write); else unused */
    float* action_out;       /* [n][4] the action actually applied (after noise and clipping), 16-byte aligned, or NULL */
    int64_t action_ld;       /* 0: `action` is [n][4]; > 0: `action` is [4][action_ld] (row stride in floats, >= n)
                                - the layout of a `W[4,D] @ obs[D,n]` GEMM output; fp32 drone kernel */
    const struct fpv_objects* objects; /* HOST pointer, read during the call: the step's object_list, or NULL.
                                Drone mode, fp32 state; combines with stick noise and pos_comp; not with obs_aos or
                                FPV_FLAG_GROUND (put a Ground entry in the list instead) */
    float* obs_aos;          /* [n][FPV_OBS_AOS_DIM] row-major observation per drone, 16-byte aligned, or NULL:
                                p3, v3, q4 (wxyz), prev_rates3, R_new@acc 3 - the values Drone.step returns
                                (components.py:247-248) gathered in one row; drone mode, fp32 state only */
    int64_t done_bits_stride;/* fpv_rollout / fpv_step_n: step t writes its bit mask at done_bits + t*done_bits_stride
                                words (>= ceil(n/64)); 0 = every step overwrites the same mask */
    const float* rotation_override; /* [n][9] row-major body->world rotation matrices, or NULL: the guidance call shape
                                Drone.step(..., rotation_matrix=R, thrust_force=f) (components.py:230-232, simulator.py:110):
                                after action2force has advanced prev_rates / prev_thrust from the sticks, the attitude is
                                REPLACED by R and the thrust becomes f * R[:,2]; drag, motor positions, collisions and the
                                attitude increment of the step start from R.  fpv_step only; drone mode, fp32 state,
                                caller-supplied sticks; combines with objects / FPV_FLAG_GROUND */
    const float* thrust_override;   /* [n] thrust_force [N] of the same call; required with rotation_override.  A NaN entry
                                leaves that drone un-overridden (its own attitude and low-passed thrust) */
    uint16_t* state_h_thrust;/* FPV_FLAG_FP16_STATE: the row of prev_thrust halves when it does NOT follow the pair rows at
                                state_h + 2 * FPV_HALF_PAIR_ROWS * ld - i.e. for a handle that steps a column range [lo, hi) of a
                                larger batch (state_h moved by 2 * lo halves, this pointer = the batch's thrust row + lo halves;
                                4-byte aligned: lo even); NULL = the row follows the pair rows */
    float* reset_pose;       /* ABI 9, drone mode: [10][ld] per-lane reset pose (rows p3 v3 q4 wxyz, the state's row order) or NULL:
                                the base pose of every reset of the lane ("Reset sources" below); 16-byte aligned.  Read only by
                                lanes that reset, written by fpv_reset when it is given position / velocity / ypr_deg */
} fpv_buffers_t;

/* Reset sources (ABI 9, drone mode: fp32 and fp16 state, every step entry point).  Every reset of a lane - fpv_reset or the
 * in-kernel reset of FPV_FLAG_AUTO_RESET - produces
 *   base  = the lane's row of fpv_buffers_t.reset_pose when it is given, else fpv_reset's arguments / init_* (as before)
 *   p = base.p + U[pos], v = base.v + U[vel], q = base.q (x) quat_from_rpy_deg(U[ypr])    (FPV_FLAG_RESET_JITTER only)
 *   prev_rates = 0, prev_thrust = 0; episode counters, noise state and Kahan rows zeroed as before.
 * fpv_reset with a table: position / velocity / ypr_deg, where given, replace the corresponding rows of the table for the
 * masked lanes (the quaternion stored is that of ypr_deg), and the lane then starts from its table row - so a later auto-reset
 * returns each drone to its own start.  A table starts as whatever the caller wrote (fpyv_amd: init_*).
 * Jitter sample = fmaf(span, u, lo), u = (w >> 8) * 2^-24 of a Philox4x32-7 word w: key = reset_seed; counter =
 * (gid lo, gid hi ^ (b << 28) ^ (e << 31), t lo, t hi) with b = 0 position / 1 velocity / 2 angles (words 0..2 = components),
 * gid = drone_id_offset + lane (the stick noise's global id), e = 1 for fpv_reset and 0 in-kernel, t = the step index of the
 * step in which the lane reported done (fpv_reset: the handle's step counter at the call).  The draw depends on (seed, gid, t)
 * only: the same for every shard, partition and single-step / k-step choice.  fpv_reset_pose_sample is the same arithmetic on
 * the host.
 * Routing: a handle with a reset source runs its single-step launches (fpv_step, fpv_rollout) on the k-step kernel with k = 1
 * (bit-identical to the single-step kernel, which stays free of the reset-source code); with obs_aos they keep the AoS kernel;
 * fpv_rollout_graph serves them like FPV_FLAG_STICK_NOISE handles (fpv_step_n; fpv_rollout with obs_aos).
 * Refused (FPV_EINVAL): either source on a Racer handle; either source together with rotation_override. */
/* out = the pose a reset of drone `global_id` in step `step` gives a lane whose base pose is `base` (p3 v3 q4), explicit_reset = 1
 * for fpv_reset, 0 for the in-kernel reset; out = base bit for bit without FPV_FLAG_RESET_JITTER.  Host arithmetic only (no
 * device needed), the kernels' own function; the parameters are checked as fpv_create checks them. */
int fpv_reset_pose_sample(const fpv_params_t* params, uint64_t global_id, uint64_t step, int explicit_reset,
                          const float base[10], float out[10]);

/* Per-drone physics (drone mode, fp32 state; functions only - FPV_ABI_VERSION and both structs are those of ABI 9).
 * A handle may be given a read-only PHYSICS TABLE phys[FPV_PHYS_ROWS][ld]: fp32, the state's row stride and column order, in a
 * device buffer the caller owns and keeps alive.  Column i holds the DERIVED constants of drone i - exactly the fp32 values
 * fpv_create narrows from a parameter set with that drone's mass, thrust cubic, drag coefficients and low-pass rates
 * (csrc/fpv_derive.h fpv_derive_physics_rows: one function fills a handle's constants and a table column), so a drone of a table
 * handle flies bit for bit like a drone of a homogeneous handle with its parameters.  Rows: */
enum {
    FPV_PHYS_RATE_LIM = 0,               /* max_rates * rates_transition_rate (the rate gain is its negation)           */
    FPV_PHYS_OMKR, FPV_PHYS_OMKT,        /* 1 - rates_transition_rate, 1 - thrust_transition_rate                       */
    FPV_PHYS_DK3, FPV_PHYS_DK2, FPV_PHYS_DK1, FPV_PHYS_DK0,   /* thrust cubic in the stick, times thrust_transition_rate  */
    FPV_PHYS_KDRAG_X, FPV_PHYS_KDRAG_Y, FPV_PHYS_KDRAG_Z,     /* 0.5 rho Cd_i A_i / m                                     */
    FPV_PHYS_INV_MASS,                   /* 1 / m                                                                       */
    FPV_PHYS_GROUND_K_M, FPV_PHYS_GROUND_C_M,                 /* ground_spring / m, ground_damping / m: loaded only by launches
                                            that can use them (FPV_FLAG_GROUND or an object list)                      */
    FPV_PHYS_ROWS                        /* = 13 */
};
/* Columns of a parameter set as fpv_physics_derive reads and fpv_physics_sample writes it */
enum {
    FPV_PHYS_IN_MASS = 0,                /* kg */
    FPV_PHYS_IN_C3, FPV_PHYS_IN_C2, FPV_PHYS_IN_C1, FPV_PHYS_IN_C0,      /* thrust_poly */
    FPV_PHYS_IN_CD_X, FPV_PHYS_IN_CD_Y, FPV_PHYS_IN_CD_Z,                /* drag_coefficients */
    FPV_PHYS_IN_RATES_LAG, FPV_PHYS_IN_THRUST_LAG,                       /* rates_transition_rate, thrust_transition_rate */
    FPV_PHYS_INPUTS                      /* = 10 */
};
/* Everything else stays uniform and comes from the handle's parameters: dt, gravity, max_rates, the motor geometry, air density
 * and cross sections, the ground spring and damping (divided by the drone's mass), init pose, noise and flags.  max_rates is
 * deliberately NOT per drone: it selects the wave-uniform form of the sin / cos of a step (angle_mode), and the default at
 * fps = 60 sits on a boundary of that choice.  The rows do not depend on dt: a table outlives fpv_set_params(dt), and
 * fpv_set_params leaves a bound table in force (re-derive it when max_rates, air density, areas or the ground constants move).
 * Kernels (csrc/fpv_phys.hip): fpv_step / fpv_rollout / fpv_rollout_graph run a single-step kernel that loads the table rows
 * with the state rows; fpv_step_n a k-step kernel that loads them once and holds them in registers; stick noise, object lists,
 * FPV_FLAG_GROUND, auto-reset and both reset sources combine with a table (a handle with a reset source runs its single steps
 * on the k-step kernel, k = 1, as without a table).  Refused with FPV_EINVAL: fp16 state, Racer mode (fpv_set_physics), Kahan rows
 * (pos_comp), the guidance override and the AoS head (obs_aos) at the launch that combines them with a table.
 * fpv_handle_algorithmic_bytes of a handle with a table: 133 + 4 * (rows its launches load) = 177, or 185 with the ground rows. */
int fpv_physics_rows(void);              /* FPV_PHYS_ROWS */
/* out_rows[r * out_ld + i] = row r of the parameter set inputs[i * FPV_PHYS_INPUTS ..] on `base` (host arithmetic only, no
 * device; out_rows is HOST memory, out_ld >= n).  A NaN cell means "the base value"; inputs == NULL: all base.  FPV_EPARAM for a
 * mass that is not positive or an infinite cell: fpv_last_error() names the first offending drone ("drone <index>: ..."). */
int fpv_physics_derive(const fpv_params_t* base, int64_t n, const double* inputs /*[n][FPV_PHYS_INPUTS]*/,
                       float* out_rows /*[rows][out_ld]*/, int64_t out_ld);
/* Randomised parameter sets for drones global_id0 .. global_id0 + n - 1: out_inputs[i][c] = base value * (lo + (hi - lo) u),
 * u = (w >> 8) * 2^-24 of a Philox4x32-7 word w; key = seed, counter = (gid lo, gid hi ^ (block << 28), 0x53594850, 0): block 0
 * words 0..3 = mass, motor strength, rates lag, thrust lag, block 1 words 0..2 = Cd x, y, z.  ONE factor scales all four thrust
 * coefficients (its range is the c3 row of `ranges`; the c2 c1 c0 rows are not read), one factor each Cd axis.  Keyed by the
 * global drone id only - the style of the reset jitter -, so a drone's parameters do not depend on its shard or partition.
 * Host arithmetic only.  FPV_EPARAM for a bound that is not finite. */
int fpv_physics_sample(const fpv_params_t* base, uint64_t seed, uint64_t global_id0, int64_t n,
                       const double* ranges /*[FPV_PHYS_INPUTS][2], relative factors lo..hi on the base value*/, double* out_inputs);

typedef struct fpv_env* fpv_handle_t;

int fpv_abi_version(void);
/* sizeof of the ABI structs as this library was compiled (0 fpv_params_t, 1 fpv_buffers_t, 2 fpv_objects_t,
 * 3 fpv_pid_params_t, 4 fpv_cache_model_t, 5 fpv_gate_course_t, 6 fpv_range_scan_t, 7 fpv_depth_render_t, 8 fpv_chase_t,
 * 10 fpv_pursuit_t, 12 fpv_pns_t, 14 fpv_detect_t, 16 fpv_boxes_t, 18 fpv_splat_t):
 * lets a foreign-language binding verify its struct declarations at load time */
int fpv_sizeof(int which);
/* rows of the state matrix for a mode (FPV_DRONE_ROWS / FPV_RACER_ROWS), or FPV_EINVAL */
int fpv_state_rows(int mode);
/* bytes each env-step must move at minimum (state R+W, action R, reward+done W) - roofline bookkeeping */
int fpv_algorithmic_bytes(int mode);
/* same for a live handle: FPV_FLAG_FP16_STATE moves 3*4 + 5*4 + 2 = 34 bytes of state each way = 89 B; the Racer as
 * written adds its six (hi, lo) rows (229 B), components.PID its three derivative rows (+24 B) */
int fpv_handle_algorithmic_bytes(fpv_handle_t h);

/* Replaces Drone.__init__'s physics set-up (components.py:86-142) / Racer.__init__ (:68-83).
 * Validates and narrows the parameters; binds to `device`.  No device allocation.
 * n <= 2^28 drones per handle (32-bit lane byte offsets into 16-byte action rows).
 * A handle need not own whole buffers: created with n = hi - lo and params->drone_id_offset + lo, and given every
 * fpv_buffers_t pointer moved by lo elements (same ld; done_bits by lo / 64 words; lo a multiple of 128; fp16 state:
 * state_h by 2 * lo halves and state_h_thrust = the thrust row + lo halves), it
 * steps the COLUMN RANGE [lo, hi) of a larger batch.  Several such handles on streams of their own are independent
 * kernel chains over one set of tensors - the split-phase layout (fpyv_amd.env.FpvVecEnv(partitions=P),
 * examples/c_host/main.c `split`): bit-identical to the single batch, and the chains hide part of each other's
 * per-launch floor. */
int fpv_create(const fpv_params_t* params, int64_t n, int device, fpv_handle_t* out);
void fpv_destroy(fpv_handle_t h);

/* Replaces Drone.reset (components.py:150-169) / Racer.reset (:85-93) for the lanes whose mask
 * byte is non-zero (mask NULL = all).  position/velocity/ypr_deg are [n][3] device arrays or NULL
 * (= the defaults in fpv_params_t); ypr is consumed as (roll,pitch,yaw) degrees like the reference.
 * Zeroes prev_rates, prev_thrust, PID state and episode counters of the reset lanes. */
int fpv_reset(fpv_handle_t h, const fpv_buffers_t* b, const uint8_t* mask, const float* position,
              const float* velocity, const float* ypr_deg, void* stream);

/* Replaces one Drone.step (components.py:220-248; object_list via fpv_buffers_t.objects, the guidance arguments
 * rotation_matrix= / thrust_force= via rotation_override / thrust_override) / Racer.step (:95-103) per drone. */
int fpv_step(fpv_handle_t h, const fpv_buffers_t* b, void* stream);

/* k consecutive steps, one launch each, with no host work in between: step t reads
 * actions + t*action_stride floats (action_stride = 0 holds b->action) and, when the strides are
 * non-zero, writes reward/done at + t*out_stride elements. */
int fpv_rollout(fpv_handle_t h, const fpv_buffers_t* b, int k, int64_t action_stride,
                int64_t out_stride, void* stream);

/* The same k steps as fpv_rollout - bit for bit - in ONE launch: each lane keeps its drone's state (and
 * noise / Kahan / episode accumulators) in registers for the k steps, streams step t's action from
 * action + t*action_stride while step t-1 computes, and writes reward/done (and done_bits) per step only
 * when the strides are non-zero, otherwise after the last step.  This is the open-loop / in-kernel-noise
 * loop `for i in range(time_steps): drone.step(...)` of src/core/simulator.py:83-156 without the
 * 112-byte state round trip per step: (16 + 5 + 112/k) B per env-step instead of 133 B.
 * Supported: drone mode (fp32 or fp16 state; stick noise, objects, Kahan rows in any combination) and
 * racer mode; obs_aos and SoA sticks (action_ld > 0) are refused: an observation row per step and a policy's
 * [4, n] output are closed-loop needs - use fpv_step (or fpv_rollout). */
int fpv_step_n(fpv_handle_t h, const fpv_buffers_t* b, int k, int64_t action_stride,
               int64_t out_stride, void* stream);

/* Drone.step's RETURN VALUE for every drone (components.py:247-248), after a step: rt [n][3][3] = rotation_matrix.T,
 * gyro [n][3][3] = euler_angles_to_rotation_matrix(*rates) - the low-passed rates in deg/s used as radians, as the
 * reference does -, acc [n][3] = rotation_matrix @ acceleration (copied from fpv_buffers_t.accel, which the step wrote;
 * null = not wanted).  One small kernel instead of a few dozen tensor operations on the host side of the boundary;
 * fp32 drone state only. */
int fpv_return_triple(fpv_handle_t h, const fpv_buffers_t* b, float* rt, float* gyro, float* acc, void* stream);

/* FPV_FLAG_FP16_STATE handles: the whole state as 14 fp32 rows out[14][out_ld] (same row numbering as the fp32 state) -
 * position rows copied, the eleven 16-bit words decoded exactly as the step kernel decodes them (v with its low words, q
 * rebuilt from its three stored components: a unit quaternion).  For a caller that reads the state each step (an
 * observation); one launch. */
int fpv_widen_state(fpv_handle_t h, const fpv_buffers_t* b, float* out, int64_t out_ld, void* stream);

/* The 64-bit step index that keys the stick-noise stream (Philox4x32-7 counter = global drone id, step index; key =
 * noise_seed) and the stochastic rounding counts the steps a handle has launched, from 0: set it to resume / replay a
 * run, read it to checkpoint one.  2^64 steps do not wrap in practice (2^32 took 5.5 h at the k-step kernel's rate,
 * which is why the 32-bit counter of ABI <= 3 was widened); streams below 2^32 steps are those of ABI <= 3 bit for bit.
 * A call that is refused (bad argument, failed launch) leaves the counter where it was; fpv_rollout advances it by the
 * launches that were accepted before the failing one. */
int fpv_set_step_counter(fpv_handle_t h, uint64_t step);
int fpv_get_step_counter(fpv_handle_t h, uint64_t* step);

/* Rotation of the traversal (every single-step kernel - drone fp32, fp16 state, AoS head, Racer -, launched by fpv_step /
 * fpv_rollout / fpv_rollout_graph; the k-step kernels of fpv_step_n keep the drone in registers and have nothing to find again;
 * no reference counterpart - the reference steps one drone).  Every launch of a dependent chain re-reads the state the previous launch wrote.  MI355X keeps the most
 * recently touched 256 MiB in its Infinity Cache; a population whose state is larger than that, walked in the same order every
 * launch, finds nothing of it there (cyclic access).  With rotation the launch starts `drones` BEFORE the drone at which the
 * previous launch started - i.e. on the rows the previous launch wrote last - and wraps around, ascending addresses all the
 * way; the results do not depend on the order (bit-identical).  The same holds one level up: the eight 4 MiB L2s keep the last
 * 32 MiB across a kernel boundary.  drones = -1 (default): automatic - the drones whose WRITTEN bytes (state rows, reward,
 * done and whatever else the call's buffers ask for and re-reads: Kahan rows, noise rows, episode sums ...; the accel rows and the AoS
 * observation head leave with a streaming hint and are not counted) fill 61/64 of the cache level that
 * a launch overflows (2^19 drones for the plain kernel's 61 B beyond the L2s, 2^22 beyond the Infinity Cache; whole rounds of the
 * eight XCDs), 0 when a launch writes less than the L2s hold; 0: plain order; > 0: that many drones (rounded down to whole
 * 128-drone workgroups).  fpv_get_rotation returns the value of the last launch (before the first: the estimate for reward
 * and done only).
 * Two cache tiers, one rule: which tier applies is decided per launch from what that launch writes.  A hipGraph replay
 * (fpv_rollout_graph) carries its own rotation, counted from its first node - a replay begins where the previous replay began
 * (one launch in k starts on cold rows) and neither reads nor moves the start that fpv_step / fpv_rollout keep in the handle:
 * mixing the two APIs on one handle is harmless (same results, each keeps its own order).
 * The automatic rule is a model of ONE device - gfx950 in single-partition mode: 256 compute units = eight XCDs with a 4 MiB L2
 * each behind a 256 MiB Infinity Cache, workgroups handed to the XCDs round-robin.  fpv_create asks the device
 * (hipGetDeviceProperties: architecture, compute units, L2 size); when the answer is anything else the automatic setting is the
 * plain order (fpv_get_rotation then reports 0 and leaves the reason in fpv_last_error(); fpv_get_cache_model has it too).  An
 * explicit request (drones > 0) is honoured on any device. */
int fpv_set_rotation(fpv_handle_t h, int64_t drones);
int fpv_get_rotation(fpv_handle_t h, int64_t* drones);

/* The cache model and what a device says about itself. */
typedef struct fpv_cache_model_t {
    uint32_t struct_size;           /* sizeof(fpv_cache_model_t) of the library that filled it */
    int32_t matches;                /* 1: the device is the one the model was measured on - rotation and L2-aware stride apply */
    int32_t compute_units;          /* hipDeviceProp_t.multiProcessorCount: what this process sees (a compute partition shows fewer) */
    int32_t xcds;                   /* 8 when matches (HIP does not report it: implied by gfx950 with all 256 CUs), else 0 */
    int64_t l2_bytes_per_xcd;       /* hipDeviceProp_t.l2CacheSize (0: not reported by the runtime) */
    int64_t infinity_cache_bytes;   /* 256 MiB when matches (HIP does not report it), else 0 */
    char arch[64];                  /* hipDeviceProp_t.gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    char reason[256];               /* matches == 0: what differs and what the library does instead; else "" */
} fpv_cache_model_t;
/* the rule itself, host arithmetic only (no device needed): would a device with these properties get the model? */
int fpv_check_cache_model(const char* arch, int compute_units, int64_t l2_bytes_per_xcd, fpv_cache_model_t* out);
/* the rule applied to device `device` (FPV_ENODEV without one) / what fpv_create found for this handle */
int fpv_device_cache_model(int device, fpv_cache_model_t* out);
int fpv_get_cache_model(fpv_handle_t h, fpv_cache_model_t* out);

/* Same k steps as fpv_rollout, replayed from a hipGraph cached in the handle: for small, launch-bound
 * batches (a 4096-drone step is ~2 us of kernel behind ~4 us of launch).  The graph is rebuilt only when
 * its SHAPE changes (k, strides, launch geometry, parameters, which optional buffers are present); new
 * buffer addresses alone are patched into the instantiated graph.  Frozen arguments mean no per-launch
 * step index, so handles with FPV_FLAG_STICK_NOISE or FPV_FLAG_FP16_STATE are served by the k-step kernel
 * (fpv_step_n: the same k steps bit for bit, and cheaper than a replay).
 * The same holds for a graph the CALLER captures around fpv_step / fpv_rollout (stream capture records the launches
 * with the step index they had at capture time): fine for plain handles, wrong - a repeating noise stream - for
 * FPV_FLAG_STICK_NOISE / FPV_FLAG_FP16_STATE handles, whose launches must be issued, not replayed. */
int fpv_rollout_graph(fpv_handle_t h, const fpv_buffers_t* b, int k, int64_t action_stride,
                      int64_t out_stride, void* stream);

/* Replace the drone type of a live handle (e.g. domain randomisation between episodes). */
int fpv_set_params(fpv_handle_t h, const fpv_params_t* params);

/* Bind (table != NULL) or unbind (NULL) the physics table of a handle ("Per-drone physics" above): a DEVICE pointer to
 * [FPV_PHYS_ROWS][ld] fp32, 16-byte aligned, ld >= n and a multiple of 4 (FPV_EALIGN otherwise), the caller's to keep alive and
 * free to rewrite between launches.  ld must be the row stride of the state the handle is stepped with (checked at the launch).
 * FPV_EINVAL for an fp16-state or Racer handle, and in a library built without csrc/fpv_phys.hip.  fpv_get_physics reads the
 * binding back (NULL / 0 = none). */
int fpv_set_physics(fpv_handle_t h, const float* table, int64_t ld);
int fpv_get_physics(fpv_handle_t h, const float** table, int64_t* ld);

/* ---- Gate courses (drone mode, fp32 state; functions only - FPV_ABI_VERSION, fpv_params_t and fpv_buffers_t are those of ABI 9)
 * A handle may be given a COURSE: an ordered list of 1..FPV_MAX_GATES gates that every drone flies through in order.  The race
 * costs one 32-bit word per drone (gate_word[n]) that the step kernels read and write with the state; the crossing test runs in
 * the step kernel on the position before and after the update (csrc/fpv_gate.h fpv_gate_step: ONE function, the kernels' and
 * fpv_gate_eval's).  The semantics are this build's (the reference has gates but no race); the geometry is the reference's Gate
 * (components.py:784-830): centre c = position, normal n = rotation_matrix[:,0], in-plane axes u, w = columns 1 and 2.
 *
 * Descriptor row of a gate, FPV_GATE_FLOATS fp32 = four 16-byte groups (fpv_gates_derive writes it):
 *     [0..2] c   [3..5] n   [6..8] u   [9..11] w   [12] a   [13] hz   [14] zc   [15] r2
 * aperture (y = u.x, z = w.x of the crossing point x relative to c):  |y| <= a  and  |z| <= hz  and  y^2 + (z - zc)^2 <= r2
 *     rectangle    a = hz = size/2            zc = 0         r2 = +inf                 (components.py:791)
 *     circle       a = hz = size/2            zc = 0         r2 = (size/2)^2           (:793-798)
 *     half_circle  a = size, hz = size/2      zc = -size/2   r2 = size^2               (:793-800)
 *
 * gate_word:  bits 0..7 the NEXT gate index, bits 8..9 the EVENT of the step just executed, bits 10..31 gates passed this episode.
 * A step, with g = next gate before the step, p_old the position rows as loaded, p_new the position after the update and before
 * any reset:  s0 = n.(p_old - c), s1 = n.(p_new - c); a FORWARD crossing is s0 < 0 && s1 >= 0 (a backward one is ignored); then
 * t = s0 / (s0 - s1), x = (p_old - c) + t (p_new - p_old), and the event is PASS when (u.x, w.x) is in the aperture, else MISS.
 * Only gate g is tested: at most one event per step.  PASS: passed += 1 (saturating at 2^22 - 1), next = (g + 1) mod count, and
 * FINISH instead of PASS when laps > 0 and passed == laps * count.
 *   reward = progress_gain (|p_old - c_g| - |p_new - c_g|) + pass_bonus [PASS or FINISH] + finish_bonus [FINISH]
 *            - miss_penalty [MISS] - crash_penalty [physics done]                       (replaces -|p - goal| on a gate handle)
 *   done   = physics done  or  FINISH  or  (MISS and miss_is_done); every done auto-resets like today's.
 * Any reset of a lane (in-kernel, or fpv_reset for its masked lanes) sets passed = 0 and next = gate_start[i] (when bound and
 * < count, else 0); the event bits still describe the step that ended.
 * gate_obs (optional, [6][gate_obs_ld], write-only, streaming stores): for the gate h that is next AFTER the step (after the
 * reset, if there was one), with the post-step (post-reset) attitude R and position p: rows 0..2 = R^T (c_h - p), 3..5 = R^T n_h.
 * The 14 state rows of a gate handle are bit for bit those of the same handle without a course while no lane resets for a gate
 * reason.  Kernels (csrc/fpv_gate.hip): a single-step kernel with the rotated traversal (the word row counts among the written
 * bytes, the obs rows do not), a k-step kernel that holds the word in a register for all k steps and runs the gate logic on every
 * step (reward and gate_obs only where they are stored), and the word reset that fpv_reset adds on the same stream.  A handle with
 * stick noise, an object list or a reset source runs its single steps on the k-step kernel (k = 1).
 * fpv_handle_algorithmic_bytes: 133 + 8 (word read + write) + 24 with gate_obs.
 * Refused with FPV_EINVAL, by name: fp16 state, Racer mode, a physics table (fpv_set_gates / fpv_set_physics), Kahan rows, the
 * guidance override, the AoS head, and stick noise together with an object list (at the launch that combines them). */
#define FPV_MAX_GATES 64
#define FPV_GATE_FLOATS 16
enum { FPV_GATE_RECTANGLE = 0, FPV_GATE_CIRCLE = 1, FPV_GATE_HALF_CIRCLE = 2 };
enum { FPV_GATE_EVENT_NONE = 0, FPV_GATE_EVENT_PASS = 1, FPV_GATE_EVENT_MISS = 2, FPV_GATE_EVENT_FINISH = 3 };
#define FPV_GATE_WORD_NEXT(w) ((uint32_t)(w) & 0xffu)
#define FPV_GATE_WORD_EVENT(w) (((uint32_t)(w) >> 8) & 3u)
#define FPV_GATE_WORD_PASSED(w) ((uint32_t)(w) >> 10)
#define FPV_GATE_MAX_PASSED 0x3fffffu

typedef struct fpv_gate {            /* what fpv_gates_derive reads: the reference's Gate(position, rotation_matrix, size, shape) */
    double position[3];
    double rotation[9];              /* row-major body -> world; orthonormal to 1e-6 */
    double size;                     /* > 0 */
    int32_t shape;                   /* FPV_GATE_RECTANGLE / _CIRCLE / _HALF_CIRCLE */
    int32_t _reserved;
} fpv_gate_t;

typedef struct fpv_gate_course {
    uint32_t struct_size;            /* sizeof(fpv_gate_course_t) = fpv_sizeof(5) */
    int32_t count;                   /* 1..FPV_MAX_GATES */
    const float* descriptors;        /* [count][FPV_GATE_FLOATS] fp32, 16-byte aligned; DEVICE memory for fpv_set_gates, HOST for fpv_gate_eval */
    uint32_t* gate_word;             /* [n] DEVICE: the race state, read and written by every step                               */
    float* gate_obs;                 /* [6][gate_obs_ld] DEVICE or NULL                                                         */
    int64_t gate_obs_ld;             /* >= n when gate_obs is given                                                             */
    const uint8_t* gate_start;       /* [n] DEVICE (HOST for fpv_gate_eval) or NULL: the gate a lane starts at after a reset     */
    int32_t laps;                    /* 0 = endless; > 0: FINISH at laps * count passes (<= FPV_GATE_MAX_PASSED)                  */
    int32_t miss_is_done;            /* != 0: a MISS ends the episode                                                           */
    float progress_gain, pass_bonus, finish_bonus, miss_penalty, crash_penalty;
    float _reserved;
} fpv_gate_course_t;

/* out_rows[k * FPV_GATE_FLOATS ..] = the descriptor row of gates[k] (host arithmetic only, no device; out_rows is HOST memory).
 * FPV_EPARAM, naming the gate ("gate <index>: ..."), for a size that is not positive, a rotation that is not orthonormal to
 * 1e-6, an unknown shape, or a count outside 1..FPV_MAX_GATES. */
int fpv_gates_derive(int count, const fpv_gate_t* gates, float* out_rows /*[count][FPV_GATE_FLOATS]*/);
/* Bind a course to a handle (the struct is copied; the device buffers stay the caller's, who keeps them alive and may rewrite the
 * descriptors between launches - moving gates), or unbind with NULL: the handle then runs exactly the kernels it ran before.
 * Allocates nothing and never synchronises.  FPV_EINVAL for the refusals above and in a library built without csrc/fpv_gate.hip. */
int fpv_set_gates(fpv_handle_t h, const fpv_gate_course_t* course);
/* The kernels' own gate function on the host (no device): for drone i of n, from p_old[i][3], p_new[i][3], q_new[i][4] (wxyz),
 * physics_done[i] and word_in[i], with a course whose `descriptors` (and `gate_start`) are HOST memory and whose device pointers
 * are not read: word_out[i], reward[i], done[i] and obs[i][6].  auto_reset != 0 resets the word of a done drone like the kernels
 * do; its obs is then taken at p_after[i] / q_after[i] (the pose the lane reappears at; NULL: p_new / q_new). */
int fpv_gate_eval(const fpv_gate_course_t* course, int64_t n, const float* p_old, const float* p_new, const float* q_new,
                  const uint8_t* physics_done, const uint32_t* word_in, int auto_reset, const float* p_after, const float* q_after,
                  uint32_t* word_out, float* reward, uint8_t* done, float* obs);

/* ---- Range scan: body-frame ray distances to the object list (build-defined; the reference's rendering of point clouds is out
 * of scope; the depth camera is "Depth camera" below) ------------------------------------------------------------
 * A ray set is 1..FPV_MAX_RAYS unit directions d_b in the body frame.  The ray r of drone i starts at its position p_i and runs
 * along d = R(q_i) d_b (body -> world, not renormalised); a range is the parameter t along d.  Every object of the list is a
 * convex solid in the geometry the collisions use - Ground the half-space z <= 0, Cylinder (x-ob.x)^2 + (y-ob.y)^2 <= radius^2
 * with ob.z <= z <= ob.z + height, Target (sphere) the ball of `radius` - met by a ray in one interval [t_in, t_out]; it is hit
 * when t_in <= t_out and t_out >= 0, at range max(t_in, 0) (0 from inside).  ranges[r][i] = min(max_range, nearest hit); a ray
 * that hits nothing, an empty or NULL list: max_range.  Rays parallel to a constraint (|d_z| < 1e-12 for the ground and a
 * cylinder's caps, d_x^2 + d_y^2 < 1e-24 for its wall) satisfy it always or never; no input gives a NaN.  Gates and trails are
 * not seen by the scan (the depth camera sees gates).  ONE definition (csrc/fpv_range.h fpv_range_lane) is run by the kernel (csrc/fpv_range.hip) and by fpv_range_eval on
 * the host: the same bits.  The scan is a kernel of its own: it serves every fp32 handle (drone or Racer; a physics table, a gate
 * course, stick noise, reset sources, partitions), leaves the state, the step counter and the rotation of the traversal alone,
 * and moves 28 + 4 ray_count bytes per drone. */
#define FPV_MAX_RAYS 32
typedef struct fpv_range_scan {
    uint32_t struct_size;               /* sizeof(fpv_range_scan_t) = fpv_sizeof(6) */
    int32_t  ray_count;                 /* 1..FPV_MAX_RAYS */
    float    rays[FPV_MAX_RAYS][3];     /* body-frame directions as fpv_rays_derive wrote them (unit to 1e-4) */
    float    max_range;                 /* finite, > 0 */
    float*   ranges;                    /* [ray_count][ranges_ld] fp32, write-only; DEVICE for fpv_range_scan, HOST for fpv_range_eval */
    int64_t  ranges_ld;                 /* >= n, multiple of 4 */
    const fpv_objects_t* objects;       /* host memory, read during the call (as fpv_buffers_t.objects); NULL or count 0: nothing to hit */
} fpv_range_scan_t;

/* out[k] = dirs[k] / |dirs[k]|, normalised in double and narrowed once (host arithmetic only).  FPV_EPARAM, naming the ray
 * ("ray <index>: ..."), for a zero or non-finite direction or a count outside 1..FPV_MAX_RAYS. */
int fpv_rays_derive(int count, const double* dirs /*[count][3]*/, float* out /*[count][3]*/);
/* One scan of the handle's n drones at b->state / b->ld on `stream`, under the handle's device: allocates nothing, never
 * synchronises, does not advance the step index and does not touch the rotation.  FPV_EINVAL / FPV_EALIGN, by name: fp16 state
 * (the packed quaternion has no reader here - the named follow-up), a wrong struct_size, ray_count out of range, rays that are
 * not unit, max_range not finite or not positive, null ranges, ranges_ld < n or not a multiple of 4, more than FPV_MAX_OBJECTS
 * objects or an unknown object type; and in a library built without csrc/fpv_range.hip. */
int fpv_range_scan(fpv_handle_t h, const fpv_buffers_t* b, const fpv_range_scan_t* s, void* stream);
/* The kernel's own lane function on the host (no handle, no device): drone i of n at p[i][3] with attitude q[i][4] (wxyz);
 * s->ranges is HOST memory. */
int fpv_range_eval(const fpv_range_scan_t* s, int64_t n, const float* p /*[n][3]*/, const float* q /*[n][4] wxyz*/);

/* ---- Depth camera: one depth image per drone of the object list and the gates (the reference's Camera, components.py:449-629) ----
 * The camera is the reference's Camera(camera_pitch_angle, position_relative_to_frame, [W, H], fov): f = W / (2 tan(fov / 2)),
 * cx = W / 2, cy = H / 2, rel_rot = WORLD2CAM^T euler_angles_to_rotation_matrix(deg2rad(pitch), 0, 0) (the pitch goes in as the roll:
 * a rotation about x after the axis swap - reproduced as computed), origin o = p + R(q) rel_pos, rotation C = R(q) rel_rot.  Pixel
 * (i, j) = column i, row j looks along d = R(q) rel_rot ((i + 1/2 - cx) / f, (j + 1/2 - cy) / f, 1) - not normalised: its
 * camera-frame z is 1, so the ray parameter IS the reference's depth (the third row of projection_matrix @ point, a z-depth).
 * image[drone][j][i] = min(max_depth, nearest hit); nothing hit: max_depth.  Where the reference splats point clouds the
 * semantics are this build's: objects are exactly the range scan's solids and hit rule (0 from inside), and GATES ARE SEEN - a gate
 * is a zero-thickness plate in its plane, seen from both faces: the region inside the aperture grown by gate_frame_width and
 * outside the aperture itself (descriptor rows of fpv_gates_derive; csrc/fpv_depth.h has the exact tests).  No input gives a NaN.
 * ONE definition (csrc/fpv_depth.h fpv_depth_pixel) is run by the kernel (csrc/fpv_depth.hip: a lane is a pixel, a wave 64
 * consecutive pixels of one drone) and by fpv_depth_eval on the host: the same bits.  Like the range scan the render is a kernel
 * of its own that reads p and q only: it serves every fp32 handle and leaves the state, the step counter and the rotation alone. */
#define FPV_DEPTH_MAX_SIDE 128
enum { FPV_DEPTH_METRES = 0,   /* fp32 metres */
       FPV_DEPTH_U8 = 1 };     /* the reference's image byte (uint8)(255 (1 - depth / max_depth)), truncated, computed in fp32 */
typedef struct fpv_camera {          /* what fpv_camera_derive reads: the reference's Camera arguments */
    double pitch_deg;                /* camera_pitch_angle */
    double relative_position[3];     /* position_relative_to_frame, body frame, m */
    double fov_deg;                  /* in (0, 180) */
    int32_t width, height;           /* resolution [W, H]: 4..FPV_DEPTH_MAX_SIDE each, W a multiple of 4 */
} fpv_camera_t;
typedef struct fpv_depth_render {
    uint32_t struct_size;            /* sizeof(fpv_depth_render_t) = fpv_sizeof(7) */
    int32_t  width, height;          /* written by fpv_camera_derive */
    int32_t  encoding;               /* FPV_DEPTH_METRES / FPV_DEPTH_U8 */
    float    dir0[3], dir_u[3], dir_v[3];   /* body-frame direction of pixel (i, j) = dir0 + i dir_u + j dir_v (fpv_camera_derive) */
    float    offset[3];              /* the camera's position in the body frame (fpv_camera_derive) */
    float    dir_len_max;            /* sqrt(1 + (W / 2f)^2 + (H / 2f)^2), rounded up: no pixel's direction is longer (fpv_camera_derive) */
    float    max_depth;              /* finite, > 0 */
    float    gate_frame_width;       /* finite, > 0 (read only with gates) */
    int32_t  gate_count;             /* 0..FPV_MAX_GATES */
    double   focal_length;           /* informational, written by fpv_camera_derive: the reference's focal_length ...       */
    double   relative_rotation[9];   /* ... and relative_rotation_matrix, row-major, in double                              */
    void*    image;                  /* [n][image_stride] elements (fp32 or bytes), row-major [H][W] inside; write-only; DEVICE for
                                        fpv_depth_render, HOST for fpv_depth_eval; 4-byte aligned */
    int64_t  image_stride;           /* elements per drone: >= W * H, multiple of 4; the padding is not written */
    const fpv_objects_t* objects;    /* host memory, read during the call; NULL or count 0: no objects */
    const float* gate_descriptors;   /* [gate_count][FPV_GATE_FLOATS] as fpv_gates_derive wrote them, 16-byte aligned: DEVICE for
                                        fpv_depth_render (the table fpv_set_gates binds: moving gates are seen where they are), HOST
                                        for fpv_depth_eval; not read with gate_count 0 */
} fpv_depth_render_t;
/* Fills width, height, dir0, dir_u, dir_v, offset, dir_len_max, focal_length and relative_rotation of *out (host arithmetic only;
 * every other field is left alone).  FPV_EPARAM, by name: width or height outside 4..128, width not a multiple of 4, fov outside
 * (0, 180), a pitch or a relative position that is not finite. */
int fpv_camera_derive(const fpv_camera_t* camera, fpv_depth_render_t* out);
/* One image per drone of the handle at b->state / b->ld on `stream`, under the handle's device: allocates nothing, never
 * synchronises, does not advance the step index and does not touch the rotation.  FPV_EINVAL / FPV_EALIGN, by name: fp16 state
 * (the packed quaternion has no reader here - the follow-up the range scan names), a wrong struct_size, width or height outside
 * 4..128 or width not a multiple of 4, an unknown encoding, direction vectors that are not finite, image_stride < W * H or not a
 * multiple of 4, max_depth (or, with gates, gate_frame_width) not finite or not positive, a null or misaligned image, more than
 * FPV_MAX_OBJECTS objects or an unknown object type, gate_count outside 0..FPV_MAX_GATES, gates without descriptors, more than
 * 2^31 waves in all; and in a library built without csrc/fpv_depth.hip. */
int fpv_depth_render(fpv_handle_t h, const fpv_buffers_t* b, const fpv_depth_render_t* s, void* stream);
/* The kernel's own pixel function on the host (no handle, no device): drone i of n at p[i][3] with attitude q[i][4] (wxyz);
 * s->image and s->gate_descriptors are HOST memory. */
int fpv_depth_eval(const fpv_depth_render_t* s, int64_t n, const float* p /*[n][3]*/, const float* q /*[n][4] wxyz*/);

/* Row stride (in floats) to allocate for n drones.  Up to 2^18 drones: n rounded up to 64, padded so that the stride in
 * bytes is at least 1 KiB past a multiple of 8 KiB (strides at or near a multiple of 8 KiB put all 14
 * rows on the same HBM channel/bank set).  Beyond: the smallest ld >= n that is 256 mod 512 floats (1 KiB past a multiple of
 * 2 KiB: the best class of stride at every measured population), moved by multiples of 64 floats where - up to 2^21 drones - that
 * stride would make the rows of a drone block share their sets in an XCD's L2 (2^19 drones: n + 320 instead of n + 256 floats,
 * 10.7 against 13.2 us per launch).  Host arithmetic only: no device needed.  Any ld >= n that is a multiple of 4
 * is accepted by fpv_step; results do not depend on ld.
 * fpv_recommended_ld is the rule FOR THE MI355X the model was measured on, whatever device is present (or none);
 * fpv_recommended_ld_device asks `device` first and returns the first, model-free rule (64-float rounding + the 8 KiB pad) for
 * every n when the device is not that one (fpv_device_cache_model; FPV_ENODEV without a device).  Allocate with the latter. */
int64_t fpv_recommended_ld(int64_t n);
int64_t fpv_recommended_ld_device(int64_t n, int device);

/* Diagnostics only: dst[i] = src[i] for n_floats fp32 values with the step kernel's access shape
 * (one dword per lane); a known-byte-count launch for calibrating rocprofv3 byte counters. */
int fpv_diag_stream_copy(float* dst, const float* src, int64_t n_floats, void* stream);
/* the same copy with 16 bytes per lane (n_floats a multiple of 4, 16-byte aligned pointers): the streaming ceiling of
 * the chip on this box - bench.py times it beside the step kernel at 2^23 drones (roofline.beyond_mall.copy_ceiling_GBs) */
int fpv_diag_stream_copy_wide(float* dst, const float* src, int64_t n_floats, void* stream);
/* which XCD runs which workgroup: a launch of `blocks` workgroups of the step kernels' size (128 threads) on `stream` of the
 * current device; workgroup b writes the id (0-7, hardware register XCC_ID) of the XCD it was dispatched to into
 * xcd_of_block[b] (device memory, `blocks` words).  The rotation of the traversal keeps a drone block on "its" XCD from launch
 * to launch only if the dispatcher deals workgroups round-robin over the eight XCDs AND starts every launch of a chain on the
 * same XCD - HIP promises neither; this is the probe that watches both (tools/xcd_map_probe.py, bench.py `roofline.xcd_map`). */
int fpv_diag_xcd_map(uint32_t* xcd_of_block, int64_t blocks, void* stream);
/* one wave that does nothing for about `microseconds` (0 < microseconds <= 1000; bounded by the constant-rate clock AND by
 * an iteration count, so every lane leaves) on `stream` of the current device: a kernel of known duration that occupies one
 * CU.  Two streams whose chains of such kernels take as long together as one chain alone run on different hardware
 * queues (fpyv_amd.streams.overlapping_streams); the runtime shares a queue between streams once it has handed out all
 * it has, and chains on a shared queue do not overlap. */
int fpv_diag_busy(double microseconds, void* stream);

/* ---- multi-GPU: contiguous shards, one process (or thread) per GPU, RCCL over xGMI ---------------------------
 * The physics needs no collective (drones are independent); the only exchange of the path is the all-gather of the
 * done mask (and, on request, per-drone episode returns) for a learner that wants the global view.  These entry
 * points give a non-Python host that exchange: RCCL is opened at run time (dlopen: an already loaded librccl - e.g.
 * the one PyTorch ships - is reused, else librccl.so.1 from the loader path or $FPV_RCCL_PATH), so libfpv_hip.so has
 * no link-time dependency on it.  The Python host uses torch.distributed (backend "nccl" = RCCL) instead. */
#define FPV_COMM_ID_BYTES 128
typedef struct fpv_comm* fpv_comm_t;
/* rank 0: create the rendezvous token (ncclGetUniqueId) and hand its 128 bytes to the other ranks out of band */
int fpv_comm_unique_id(uint8_t id[FPV_COMM_ID_BYTES]);
/* every rank: join the communicator (ncclCommInitRank) on `device`; collective - returns when all ranks joined */
int fpv_comm_create(const uint8_t id[FPV_COMM_ID_BYTES], int world_size, int rank, int device, fpv_comm_t* out);
void fpv_comm_destroy(fpv_comm_t c);
/* what the communicator was created with, and the RCCL version (ncclGetVersion: e.g. 22105) actually loaded - lets a
 * benchmark line certify "RCCL saw N ranks"; any out pointer may be NULL */
int fpv_comm_info(fpv_comm_t c, int* world_size, int* rank, int* rccl_version);
/* all-gather of the bit-packed done masks: every rank contributes words_per_rank 64-bit words (its
 * fpv_buffers_t.done_bits, or a whole [steps][words] bucket of them) and receives world_size * words_per_rank words,
 * rank r's block at recv + r * words_per_rank.  Enqueued on `stream`; equal shard sizes on every rank. */
int fpv_allgather_done(fpv_comm_t c, const uint64_t* send_bits, uint64_t* recv_bits, int64_t words_per_rank, void* stream);
/* same for fp32 values (episode returns: fpv_buffers_t.last_return) */
int fpv_allgather_f32(fpv_comm_t c, const float* send, float* recv, int64_t count_per_rank, void* stream);

/* ---- components.PID for N drones at once (src/utils/components.py:15-54) --------------------------------
 * The reference's guidance PID (Drone.force_multiplier_pid, components.py:145,:288): leaky clipped integral,
 * clipped and low-passed derivative, clipped output.  One lane per drone, state as SoA rows
 * pid_state[FPV_PID_ROWS][ld] (fp32, caller-owned).  The same lane function is the racer_pid_variant = 1 rate
 * loop of FPV_MODE_RACER. */
enum { FPV_PID_INTEGRAL = 0, FPV_PID_PREV_DERIVATIVE, FPV_PID_PREV_ERROR, FPV_PID_IS_FIRST, FPV_PID_ROWS };
typedef struct fpv_pid_params {
    uint32_t struct_size;             /* = sizeof(fpv_pid_params_t) */
    uint32_t _reserved;
    double kP, kI, kD, dt;            /* PID.__init__ (components.py:16-20) */
    double integral_clip;             /* default 1   */
    double min_output;                /* default 0.3 */
    double max_output;                /* default 1   */
    double derivative_transition_rate;/* default 0.5 */
} fpv_pid_params_t;
/* PID.reset (components.py:35-41) for the lanes whose mask byte is non-zero (mask NULL = all) */
int fpv_pid_reset(float* pid_state, int64_t ld, int64_t n, const uint8_t* mask, int device, void* stream);
/* PID.__call__(current, target) (components.py:43-54) per drone: out[i] = clip(kP e + kI I + kD D, min, max) with
 * e = current[i] - target, target = target[i] or, when `target` is NULL, target_scalar.  Also writes, when given,
 * error_out[i] (PID.error).  pid_state rows hold integral, prev_derivative, previous_error, is_first. */
int fpv_pid_call(const fpv_pid_params_t* params, float* pid_state, int64_t ld, int64_t n, const float* current,
                 const float* target, float target_scalar, float* out, float* error_out, int device, void* stream);

/* ---- Target chase: the reference's vision guidance law for N drones (functions and one struct only - FPV_ABI_VERSION, fpv_params_t
 * and fpv_buffers_t are those of ABI 9) -------------------------------------------------------------------------------------------
 * Drone.calculate_needed_force_orientation(pixel, target, ref_frame, mode) (components.py:258-304) fed by the pixel at which the
 * drone's camera sees the target (simulator.py:102-110): one kernel, a lane per drone, reads p, v and q of an fp32 drone handle and
 * the drone's four guidance-PID rows (FPV_PID_*, "components.PID" below), writes rotation[n][9] and thrust[n] in exactly the layout
 * fpv_buffers_t.rotation_override / thrust_override take - the next fpv_step flies them.  The camera is the depth camera's
 * (fpv_camera_t) without an image's size limits.  One shared target (centre, radius).  csrc/fpv_chase.h restates the law as
 * computed and is the ONE definition the kernel (csrc/fpv_chase.hip) and fpv_chase_eval run: the same bits.
 *   pixel: the caller's (x, y) per drone, or - pixel == NULL - the projection of the target's CENTRE (this build's definition of the
 *     reference's centroid of splatted pixels), seen iff depth in (0, max_depth] and 0 <= x < W, 0 <= y < H.  A drone that does not
 *     see the target (or whose given pixel is NaN) is not guided: thrust = NaN (fpv_step: not overridden), rotation = identity,
 *     pixel_out = NaN, visible = 0, PID rows untouched.
 *   defined where the reference gives NaN: |v| = 0 -> no virtual drag; F parallel to the second operand of the first cross
 *     product -> that operand is replaced by the world x axis, then by the world y axis; F = 0 -> identity, thrust 0; a result
 *     that is not finite -> not guided.  No finite state gives a NaN matrix.
 * Like the range scan and the depth camera it is a kernel of its own: the state, the step counter and the rotation of the
 * traversal are left alone.  It moves 112 bytes per drone (10 state floats + 4 PID rows read, 4 PID rows + 10 floats written),
 * 120 with a supplied pixel. */
#define FPV_CHASE_MAX_SIDE 16384
enum { FPV_CHASE_WORLD = 0, FPV_CHASE_DRONE = 1 };            /* ref_frame = 'world' / 'drone' */
enum { FPV_CHASE_LEVEL = 0, FPV_CHASE_FRONTARGET = 1 };       /* mode = 'level' / 'frontarget' */
typedef struct fpv_chase {
    uint32_t struct_size;            /* sizeof(fpv_chase_t) = fpv_sizeof(8) */
    int32_t  width, height;          /* written by fpv_chase_derive: 1..FPV_CHASE_MAX_SIDE */
    int32_t  ref_frame;              /* FPV_CHASE_WORLD / FPV_CHASE_DRONE */
    int32_t  mode;                   /* FPV_CHASE_LEVEL / FPV_CHASE_FRONTARGET */
    int32_t  _reserved;
    double   focal_length;           /* written by fpv_chase_derive, like relative_rotation (row-major) and relative_position */
    double   relative_rotation[9];
    double   relative_position[3];
    double   max_depth;              /* reach of the reference's target-only image (simulator.py:102: 15), finite, > 0 */
    double   mass;                   /* kg: g = (0, 0, -9.81 mass) */
    double   virtual_drag_coefficient, virtual_lift_coefficient, tof_effective_distance;   /* params.yaml point_and_shoot */
    double   keep_distance, UWB_sensor_max_range;                                            /* params.yaml drone */
    float    target[3];              /* the target's centre ... */
    float    target_radius;          /* ... and radius, >= 0 */
    fpv_pid_params_t pid;            /* Drone.force_multiplier_pid (components.py:143-145) */
    float*   pid_state;              /* [FPV_PID_ROWS][pid_ld], read and written; DEVICE for fpv_chase_guide, HOST for fpv_chase_eval (as */
    int64_t  pid_ld;                 /* >= n                                                         every pointer below); 4-byte aligned */
    const float* pixel;              /* [n][2] (x, y) or NULL = find the target; 8-byte aligned */
    float*   rotation;               /* [n][9] row-major body -> world, 4-byte aligned */
    float*   thrust;                 /* [n] newtons; NaN = not guided */
    float*   pixel_out;              /* [n][2] or NULL: the pixel used (NaN, NaN when not seen); 8-byte aligned */
    uint8_t* visible;                /* [n] or NULL: exactly 0 or 1 */
} fpv_chase_t;
/* Fills width, height, focal_length, relative_rotation and relative_position of *out (host arithmetic only; every other field is
 * left alone).  FPV_EPARAM, by name: width or height outside 1..16384, fov outside (0, 180), a pitch or a relative position that is
 * not finite. */
int fpv_chase_derive(const fpv_camera_t* camera, fpv_chase_t* out);
/* One call of the law for the handle's n drones at b->state / b->ld on `stream`, under the handle's device: allocates nothing,
 * never synchronises, does not advance the step index and does not touch the rotation.  FPV_EINVAL / FPV_EALIGN / FPV_EPARAM, by
 * name: fp16 state, a Racer handle, a wrong struct_size, width or height out of range, an unknown ref_frame or mode, camera numbers
 * or constants that are not finite, max_depth or mass not positive, a negative target radius, PID constants fpv_pid_call would
 * refuse, null pid_state / rotation / thrust, pid_ld < n, misaligned pointers; and in a library built without csrc/fpv_chase.hip. */
int fpv_chase_guide(fpv_handle_t h, const fpv_buffers_t* b, const fpv_chase_t* s, void* stream);
/* The kernel's own lane function on the host (no handle, no device): drone i of n at p[i][3] with velocity v[i][3] and attitude
 * q[i][4] (wxyz); every pointer of *s is HOST memory. */
int fpv_chase_eval(const fpv_chase_t* s, int64_t n, const float* p /*[n][3]*/, const float* v /*[n][3]*/, const float* q /*[n][4] wxyz*/);

/* ---- Pursuit task: every drone chases a target of its own (functions and one struct only - FPV_ABI_VERSION, fpv_params_t and
 * fpv_buffers_t are those of ABI 9) -----------------------------------------------------------------------------------------------
 * The reference's simulator (simulator.py:54-110) for N drones: generate_targets once, target.update() every iteration, the guidance
 * law against the drone's target.  targets[FPV_TGT_ROWS][targets_ld] holds a target per drone in the state's column order (4-byte
 * cells, caller-owned): the centre and the radius of its circular path (components.CircularPath; radius 0 = it stands still), the
 * sphere's radius, the distance last measured, the word COUNT (bits 0..16: path index of the next update(), bit 31 FPV_TGT_FRESH: not
 * advanced since it was set or respawned - such a target stands at that index and its first update() leaves it there) and the word
 * SPAWNS (low 16 bits: respawns so far, high 16: captures in the current episode).  The unit circle is one shared table circle[K][2]
 * (fpv_pursuit_derive).  One kernel of its own, a lane per drone, launched AFTER the step (the reference's order: update(), the law on
 * the state the next step starts from, then the step): it advances the target, measures dist = |t - p| - radius, pays
 * progress (previous dist - dist) and, when dist <= capture_distance, `capture` - then the target respawns in the spawn box (a
 * Philox draw keyed by spawn_seed, the drone's global id and its respawn index only) and the jump of the distance is not paid -,
 * observes the target in the body frame and, with `guide`, runs the target chase's law against the drone's own target and writes the
 * next step's override.  A lane whose done byte is set (fpv_pursuit_step) or that is in the mask (fpv_pursuit_reset) REBASES: it pays
 * nothing, clears its episode's captures, respawns when respawn_on_done, restarts its distance and (guide) its PID rows.
 * csrc/fpv_pursuit.h states all of it as computed and is the ONE definition the kernel (csrc/fpv_pursuit.hip) and fpv_pursuit_eval
 * run: the same bits.  The step kernels' object list, the range scan and the depth camera do not see these targets. */
enum { FPV_TGT_CX = 0, FPV_TGT_CY, FPV_TGT_CZ, FPV_TGT_PATH_R, FPV_TGT_RADIUS, FPV_TGT_PREV_DIST, FPV_TGT_COUNT, FPV_TGT_SPAWNS, FPV_TGT_ROWS };
#define FPV_TGT_FRESH 0x80000000u
#define FPV_PURSUIT_OBS 7              /* rows of obs: R^T (t - p) (3), R^T (v_target - v) (3), dist */
#define FPV_PURSUIT_MAX_RESOLUTION 65536
typedef struct fpv_pursuit {
    uint32_t struct_size;            /* sizeof(fpv_pursuit_t) = fpv_sizeof(10) (9 stays "no such struct") */
    int32_t  path_resolution;        /* K: 1..FPV_PURSUIT_MAX_RESOLUTION (the reference's default: 5500) */
    int32_t  advance;                /* 0: the targets are not moved by this call */
    int32_t  respawn_on_done;        /* a rebasing lane draws a new target */
    int32_t  add_to_reward;          /* fpv_pursuit_step adds the payment to b->reward (required then) and b->ep_return (when given) */
    int32_t  _reserved;
    uint64_t spawn_seed;
    double   dt;                     /* > 0: the target's velocity is (t - t_previous) / dt */
    double   capture_distance;       /* >= 0 */
    double   progress, capture;      /* the rewards */
    double   spawn_lo[3], spawn_hi[3];   /* box of a respawned target's centre, lo <= hi */
    double   radius_lo, radius_hi;       /* range of its radius, 0 <= lo <= hi */
    float*   targets;                /* [FPV_TGT_ROWS][targets_ld], 16-byte aligned; DEVICE for fpv_pursuit_step / _reset, HOST for */
    int64_t  targets_ld;             /* >= n                                             fpv_pursuit_eval (as every pointer below) */
    const float* circle;             /* [K][2] (cos, sin), 8-byte aligned: what fpv_pursuit_derive wrote */
    float*   obs;                    /* [FPV_PURSUIT_OBS][obs_ld] or NULL */
    int64_t  obs_ld;
    float*   position;               /* [3][position_ld] or NULL: the target's world position */
    int64_t  position_ld;
    uint8_t* event;                  /* [n] or NULL: 1 = captured in this call */
    float*   reward_out;             /* [n] or NULL: what the task paid in this call */
    const fpv_chase_t* guide;        /* or NULL.  Given: its pid_state, rotation and thrust are required (and pixel_out / visible honoured), */
} fpv_pursuit_t;                     /* its target, target_radius and pixel are ignored - the pixel is found by projection */
/* circle_out_host[resolution][2] = (cos, sin)(2 pi j / resolution) as the reference's linspace takes the angles, computed in double
 * and rounded once (host arithmetic only).  FPV_EPARAM: a resolution outside 1..65536. */
int fpv_pursuit_derive(int32_t resolution, float* circle_out_host);
/* The respawn draw of drone `global_id`'s respawn number `respawn_index` on the host (the kernel's own function): out[0..2] the
 * centre, out[3] the radius, *phase_out the path index in [0, K).  Reads spawn_seed, the box, the radius range and path_resolution
 * of *s. */
int fpv_pursuit_sample(const fpv_pursuit_t* s, uint64_t global_id, uint32_t respawn_index, float out[4], uint32_t* phase_out);
/* One call for the handle's n drones at b->state / b->ld on `stream`, under the handle's device: reads b->done (NULL = no lane
 * rebases), adds to b->reward / b->ep_return when add_to_reward.  Allocates nothing, never synchronises, does not advance the step
 * index and does not touch the rotation.  FPV_EINVAL / FPV_EALIGN / FPV_EPARAM, by name: fp16 state, a Racer handle, a wrong
 * struct_size, path_resolution out of range, constants that are not finite, a box with hi < lo, a negative radius or
 * capture_distance, dt <= 0, null targets / circle, targets_ld (obs_ld, position_ld) < n, misaligned pointers, add_to_reward without
 * b->reward, everything fpv_chase_guide refuses for `guide`; and in a library built without csrc/fpv_pursuit.hip. */
int fpv_pursuit_step(fpv_handle_t h, const fpv_buffers_t* b, const fpv_pursuit_t* s, void* stream);
/* The reset call, after fpv_reset with the same mask: the lanes whose mask byte is non-zero (mask NULL = all) rebase; the others are
 * not touched at all.  Pays nothing and does not read b->done / b->reward. */
int fpv_pursuit_reset(fpv_handle_t h, const fpv_buffers_t* b, const fpv_pursuit_t* s, const uint8_t* mask, void* stream);
/* The kernel's own lane function on the host (no handle, no device): drone i of n at p[i][3] with velocity v[i][3] and attitude
 * q[i][4] (wxyz), global id drone_id_offset + i; done_or_mask [n] or NULL, reward [n] (read and written when add_to_reward, else may
 * be NULL); reset != 0: the reset call.  Every pointer of *s is HOST memory. */
int fpv_pursuit_eval(const fpv_pursuit_t* s, int64_t n, uint64_t drone_id_offset, const float* p /*[n][3]*/, const float* v /*[n][3]*/,
                     const float* q /*[n][4] wxyz*/, const uint8_t* done_or_mask, float* reward, int reset);

/* ---- Point and shoot: the reference's steered guidance law for N drones (functions and one struct only - FPV_ABI_VERSION,
 * fpv_params_t and fpv_buffers_t are those of ABI 9) ---------------------------------------------------------------------------------
 * Drone.point_and_shoot(pixel, action, ref_frame, mode) (components.py:312-381): the target chase's sibling whose four commands
 * steer it - action[1] is where on the image (vertical axis, -1..1) the target is to be held, action[2:] a virtual offset of the
 * target in half-images; action[0] only feeds a yaw angle the reference discards and is not used.  One kernel, a lane per drone,
 * reads p, v and q of an fp32 drone handle, the drone's four guidance-PID rows (the rows the chase uses: the reference has one PID for
 * both laws) and its two prev_pixel rows, writes rotation[n][9] and thrust[n] in the layout fpv_buffers_t.rotation_override /
 * thrust_override take.  csrc/fpv_pns.h restates the law as computed and is the ONE definition the kernel (csrc/fpv_pns.hip) and
 * fpv_pns_eval run: the same bits.
 *   pixel: the caller's (x, y) per drone, or - pixel == NULL - the projection of the centre of `target` (one for all, HOST [3]) or of
 *     target_rows[3][target_ld] (one per drone, the layout fpv_pursuit_t.position writes), seen as the chase sees it.  A drone that
 *     does not see the target, whose given pixel is NaN or whose action is not finite is not guided: thrust = NaN, rotation =
 *     identity, visible = 0, pixel_velocity = throttle = NaN, limited = 0, PID rows and prev_pixel untouched.
 *   thrust limit: the reference's `while |F| > max_throttle_in_force` loop (:358-366) in closed form, no loop: the multiplier becomes
 *     clip(-b + sqrt(b^2 - |B|^2 + Fmax^2), min_output, max_output), b = d . B; where even min_output gives |F| > Fmax (the
 *     reference never returns) the direction of that F with thrust = Fmax.  limited: 0 not limited, 1 limited, 2 out of reach.
 *   prev_pixel[2][prev_pixel_ld]: the law's pixel of the previous call; NaN = the reference's None (the first call: velocity 0).
 *   restart[n]: a lane whose byte is set first resets its PID rows (PID.reset) and its prev_pixel (Drone.reset).
 *   defined where the reference gives NaN as the chase defines it.
 * It moves 156 bytes per drone with per-drone targets and commands (10 state floats, 4 PID and 2 prev_pixel rows, 3 target floats and
 * 4 commands read; 4 PID and 2 prev_pixel rows and 10 floats written), 171 with the restart bytes and every optional output. */
typedef struct fpv_pns {
    uint32_t struct_size;            /* sizeof(fpv_pns_t) = fpv_sizeof(12) (11 stays "no such struct") */
    int32_t  width, height;          /* the camera numbers fpv_chase_derive writes: copy them from its fpv_chase_t (fpv_pns_derive does) */
    int32_t  ref_frame;              /* FPV_CHASE_WORLD / FPV_CHASE_DRONE */
    int32_t  mode;                   /* FPV_CHASE_LEVEL / FPV_CHASE_FRONTARGET */
    int32_t  _reserved;
    double   focal_length;
    double   relative_rotation[9];
    double   relative_position[3];
    double   max_depth;              /* finite, > 0 */
    double   mass;                   /* kg: g = (0, 0, -9.81 mass) */
    double   virtual_drag_coefficient, virtual_lift_coefficient, tof_effective_distance;   /* params.yaml point_and_shoot */
    double   max_throttle_in_force;  /* Fmax > 0, newtons */
    double   thrust2throttle_poly[4];/* throttle percent as a cubic of the thrust, highest power first (components.py:137) */
    fpv_pid_params_t pid;            /* Drone.force_multiplier_pid (components.py:143-145) */
    float*   pid_state;              /* [FPV_PID_ROWS][pid_ld], read and written; DEVICE for fpv_pns_guide, HOST for fpv_pns_eval (as every */
    int64_t  pid_ld;                 /* >= n                                                pointer below but `target`); 4-byte aligned */
    float*   prev_pixel;             /* [2][prev_pixel_ld], read and written */
    int64_t  prev_pixel_ld;          /* >= n */
    const float* pixel;              /* [n][2] (x, y) or NULL = find the target; 8-byte aligned */
    const float* target;             /* HOST [3], read during the call: one target centre for all, or NULL */
    const float* target_rows;        /* [3][target_ld]: a target centre per drone, or NULL.  pixel == NULL needs exactly one of the two */
    int64_t  target_ld;              /* >= n */
    const float* action;             /* [n][4] or NULL = zeros; 16-byte aligned */
    const uint8_t* restart;          /* [n] or NULL */
    float*   rotation;               /* [n][9] row-major body -> world, 4-byte aligned */
    float*   thrust;                 /* [n] newtons; NaN = not guided */
    float*   pixel_velocity;         /* [n][2] or NULL: Drone.pixel_velocity, pixels per second; 8-byte aligned */
    uint8_t* limited;                /* [n] or NULL: 0, 1 or 2 */
    uint8_t* visible;                /* [n] or NULL: exactly 0 or 1 */
    float*   throttle;               /* [n] or NULL: thrust2throttle(thrust) in [-1, 1] */
} fpv_pns_t;
/* Fills width, height, focal_length, relative_rotation and relative_position of *out with what fpv_chase_derive computes for the
 * camera (host arithmetic only; every other field is left alone); refuses what fpv_chase_derive refuses. */
int fpv_pns_derive(const fpv_camera_t* camera, fpv_pns_t* out);
/* One call of the law for the handle's n drones at b->state / b->ld on `stream`, under the handle's device: allocates nothing,
 * never synchronises, does not advance the step index and does not touch the rotation.  FPV_EINVAL / FPV_EALIGN / FPV_EPARAM, by
 * name: everything fpv_chase_guide refuses of the fields the two structs share, max_throttle_in_force not positive, a polynomial
 * that is not finite, null prev_pixel, prev_pixel_ld or target_ld < n, both `target` and `target_rows` given, neither given without
 * a pixel, misaligned pointers; and in a library built without csrc/fpv_pns.hip. */
int fpv_pns_guide(fpv_handle_t h, const fpv_buffers_t* b, const fpv_pns_t* s, void* stream);
/* The kernel's own lane function on the host (no handle, no device): drone i of n at p[i][3] with velocity v[i][3] and attitude
 * q[i][4] (wxyz); every pointer of *s is HOST memory. */
int fpv_pns_eval(const fpv_pns_t* s, int64_t n, const float* p /*[n][3]*/, const float* v /*[n][3]*/, const float* q /*[n][4] wxyz*/);

/* ---- Object detections: the 2-D box of every object and gate in every drone's camera (functions and two structs only -
 * FPV_ABI_VERSION, fpv_params_t, fpv_buffers_t and fpv_objects_t are those of ABI 9) ---------------------------------------------------
 * The reference's Camera.project(attr='bbox3d'), bbox3d_to_bbox2d and pruned_objects_list (components.py:558-600) for N drones: for
 * a drone pose and an axis-aligned world box (min[3], max[3]) the eight corners in the reference's order (helper_functions.py:126-132)
 * are taken into the camera frame, c = Rcam^T (X - pcam) with pcam = p + R(q) rel_pos and Rcam = R(q) rel_rot (Camera.update); a
 * corner is in front when c.z > 0, its pixel is ((f c.x) / c.z + W/2, (f c.y) / c.z + H/2).  The box is the componentwise min and max
 * over the in-front corners, depth the smallest in-front c.z, visible the reference's pruning rule: a corner in front and
 * x_max > 0, y_max > 0, x_min < W, y_min < H.  With no corner in front (the reference's bbox2d raises) the box is (0, 0, 0, 0), depth 0,
 * visible 0.  FPV_DETECT_INT truncates every pixel coordinate toward zero (the reference's astype(int)) and keeps it a float;
 * FPV_DETECT_FLOAT keeps the sub-pixel value.  clip != 0 clamps a VISIBLE box to [0, W] x [0, H] (the reference does not clip).
 * csrc/fpv_detect.h is the ONE definition the kernel (csrc/fpv_detect.hip: a lane is a drone, blockIdx.y a group of 8 slots) and
 * fpv_detect_eval run: the same bits.  Like the range scan it reads p and q only: it serves every fp32 handle and leaves the state,
 * the step counter and the rotation alone; it moves 28 + 21 M bytes per drone for M boxes.
 * Slots: the boxes of `table` in order (fpv_boxes_derive: the collidable objects of the list, then the gates of the course), then -
 * target_rows given - the lane's OWN box, centre +- radius around target_rows[0..2][i] (the layout fpv_pursuit_t.position writes),
 * radius = target_radius[i] or, without that row, target_radius_all. */
#define FPV_MAX_BOXES (FPV_MAX_OBJECTS + FPV_MAX_GATES)
enum { FPV_DETECT_INT = 0, FPV_DETECT_FLOAT = 1 };
typedef struct fpv_boxes { int32_t count; float box[FPV_MAX_BOXES][6]; } fpv_boxes_t;   /* box: min x, y, z, max x, y, z; fpv_sizeof(16) */
typedef struct fpv_detect {
    uint32_t struct_size;            /* sizeof(fpv_detect_t) = fpv_sizeof(14) (13 stays "no such struct") */
    int32_t  width, height;          /* written by fpv_detect_derive, like the three camera fields below */
    int32_t  pixel_mode;             /* FPV_DETECT_INT / FPV_DETECT_FLOAT */
    int32_t  clip;                   /* != 0: clamp visible boxes to the image */
    int32_t  _reserved;
    double   focal_length;
    double   relative_rotation[9];
    double   relative_position[3];
    const fpv_boxes_t* table;        /* HOST memory, read during the call; NULL or count 0: only the own-target slot */
    const float* target_rows;        /* [3][target_ld] or NULL = no own-target slot; DEVICE for fpv_detect_boxes, HOST for fpv_detect_eval */
    int64_t  target_ld;              /* >= n */
    const float* target_radius;      /* [n] a radius per drone, or NULL = target_radius_all (DEVICE / HOST like target_rows) */
    float    target_radius_all;      /* finite, >= 0 */
    float    _reserved2;
    float*   boxes;                  /* [M][4][ld] x_min, y_min, x_max, y_max; write-only; DEVICE / HOST like target_rows; 4-byte aligned */
    float*   box_depth;              /* [M][ld] */
    uint8_t* box_visible;            /* [M][ld] exactly 0 or 1 */
    int64_t  ld;                     /* >= n, multiple of 4; columns n..ld-1 and slots >= M are not written */
} fpv_detect_t;
/* The box table of an object list and a course (host arithmetic only, double, narrowed once): first objects->obj[k] in order -
 * Ground: [-size/2, size/2]^2 x {0} with size = ground_size[k] (the reference's grid cloud); Cylinder: [x +- r, y +- r, z .. z + h]
 * (the reference's cloud when angle_resolution = 1 mod 4); Sphere: centre +- radius (what the box of the reference's icosphere tends
 * to) -, then gates[g] in order: the box of the reference's own corner points (components.py:790-805) at gate_resolution (17 is the
 * reference's) - rectangle, circle and half_circle with its radius `size` and its -size/2 shift.  objects and gates may be NULL with
 * no entries.  FPV_EPARAM, naming the slot ("box <index>: ..."): a Ground without ground_size or with a size that is not positive, a radius or height that makes
 * min > max, a box that is not finite, an unknown type or shape, gate_resolution outside 1..4096, more than FPV_MAX_BOXES boxes. */
int fpv_boxes_derive(const fpv_objects_t* objects, const double* ground_size /*[objects->count] or NULL*/, const fpv_gate_t* gates,
                     int gate_count, int gate_resolution, fpv_boxes_t* out);
/* Fills width, height, focal_length, relative_rotation and relative_position of *out with what fpv_chase_derive computes for the
 * camera (host arithmetic only; the reference's 640 x 480 is accepted; every other field is left alone). */
int fpv_detect_derive(const fpv_camera_t* camera, fpv_detect_t* out);
/* One detection of the handle's n drones at b->state / b->ld on `stream`, under the handle's device: allocates nothing, never
 * synchronises, does not advance the step index and does not touch the rotation.  The struct is checked before the handle is
 * looked at.  FPV_EINVAL / FPV_EALIGN / FPV_EPARAM, by name: null or misaligned outputs, ld < n or not a multiple of 4, a count
 * (table + own slot) outside 1..FPV_MAX_BOXES, a box that is not finite or has min > max, camera numbers that are not
 * fpv_detect_derive's, an unknown pixel mode, fp16 state; FPV_ENODEV for a null handle where there is no device; and in a library
 * built without csrc/fpv_detect.hip. */
int fpv_detect_boxes(fpv_handle_t h, const fpv_buffers_t* b, const fpv_detect_t* s, void* stream);
/* The kernel's own lane function on the host (no handle, no device): drone i of n at p[i][3] with attitude q[i][4] (wxyz); every
 * pointer of *s is HOST memory. */
int fpv_detect_eval(const fpv_detect_t* s, int64_t n, const float* p /*[n][3]*/, const float* q /*[n][4] wxyz*/);

/* ---- Point-cloud camera: the reference's splatted depth image of every drone (functions and one struct only - FPV_ABI_VERSION,
 * fpv_params_t and fpv_buffers_t are those of ABI 9) -------------------------------------------------------------------------------
 * The reference's Camera.render_depth_image and render_image (components.py:602-629) for N drones: the objects whose projected box
 * misses the image are pruned (the rule of "Object detections", pixel mode FPV_DETECT_INT, on box[m] shifted by offset[m]); every
 * point X = point + offset[m] of a kept object goes into the camera frame, c = Rcam^T (X - pcam); it is in front when c.z > 0; its
 * pixel is (trunc((f c.x) / c.z + W/2), trunc((f c.y) / c.z + H/2)) - truncated toward zero like astype(int), so a coordinate in
 * (-1, 0) lands in column or row 0 -, accepted when 0 <= u < W and 0 <= v < H; a pixel keeps the smallest c.z that landed in it.
 * FPV_SPLAT_U8: byte = (uint8)(255 (1 - min(z, max_depth) / max_depth)), a pixel without a point takes max_depth (byte 0);
 * FPV_SPLAT_METRES: that depth as fp32 (max_depth where no point landed, not clipped otherwise); FPV_SPLAT_MASK: the byte 1 where a
 * point landed, else 0 (render_image).  centroid / lit (optional): the pixels whose U8 byte at this max_depth is > 0 are lit; lit[i] is
 * their count, centroid[i] = (sum of their columns / count, sum of their rows / count), NaN NaN with none - the tracker of
 * simulator.py:102-107.  csrc/fpv_splat.h is the ONE definition the kernel (csrc/fpv_splat.hip: a workgroup is a drone, the z-buffer
 * W * H words of LDS) and fpv_splat_eval run: the same bits.  It reads p and q only, serves every fp32 handle and leaves the state,
 * the step counter and the rotation alone. */
#define FPV_SPLAT_MAX_POINTS (1 << 20)
enum { FPV_SPLAT_METRES = 0, FPV_SPLAT_U8 = 1, FPV_SPLAT_MASK = 2 };
enum { FPV_CLOUD_GROUND = 0, FPV_CLOUD_CYLINDER = 1, FPV_CLOUD_GATE = 2 };
typedef struct fpv_splat {
    uint32_t struct_size;            /* sizeof(fpv_splat_t) = fpv_sizeof(18) (17 stays "no such struct") */
    int32_t  width, height;          /* written by fpv_splat_derive, like the three camera fields below: 4..128, W a multiple of 4 */
    int32_t  encoding;               /* FPV_SPLAT_METRES / _U8 / _MASK */
    float    max_depth;              /* finite, > 0 */
    int32_t  object_count;           /* M: 0..FPV_MAX_BOXES */
    double   focal_length;
    double   relative_rotation[9];
    double   relative_position[3];
    int32_t  first[FPV_MAX_BOXES + 1];   /* object m owns the points first[m] .. first[m + 1] - 1; first[0] = 0, non-decreasing, <= 2^20 */
    int32_t  _reserved;
    float    offset[FPV_MAX_BOXES][3];   /* added to every point and to the box of object m (a moving Target: its vertices stay put) */
    float    box[FPV_MAX_BOXES][6];      /* min x, y, z, max x, y, z of object m's points before the offset: finite, min <= max */
    const float* points;             /* [3][point_ld] x row, y row, z row; DEVICE for fpv_splat_render, HOST for fpv_splat_eval; 4-byte
                                        aligned; may be NULL when first[M] = 0; columns at and past first[M] are not read */
    int64_t  point_ld;               /* >= first[M], multiple of 4 */
    void*    image;                  /* [n][image_ld] elements (fp32 for METRES, bytes for U8 and MASK), row-major [H][W] inside;
                                        write-only; DEVICE / HOST like points; 4-byte aligned */
    int64_t  image_ld;               /* elements per drone: >= W * H, multiple of 4; the padding is not written */
    float*   centroid;               /* [n][2] (x, y) or NULL; DEVICE / HOST like points; 4-byte aligned; given together with lit */
    int32_t* lit;                    /* [n] or NULL */
} fpv_splat_t;
/* Fills width, height, focal_length, relative_rotation and relative_position of *out with what fpv_chase_derive computes for the
 * camera, under the depth camera's limits (width and height 4..128, width a multiple of 4); every other field is left alone. */
int fpv_splat_derive(const fpv_camera_t* camera, fpv_splat_t* out);
/* The deterministic clouds of the reference (host arithmetic only, double, narrowed once) as fp32 SoA out_points[3][ld]:
 * FPV_CLOUD_GROUND (components.py:655-664): numbers = {size}, resolutions = {resolution}: the resolution^2 grid at z = 0, x fastest;
 * FPV_CLOUD_CYLINDER (:697-708): numbers = {x, y, z, radius, height}, resolutions = {angle_resolution, height_resolution}: the mesh,
 * angle fastest, plus the position; FPV_CLOUD_GATE (:790-805): numbers = {position[3], rotation_matrix[9] row-major, size},
 * resolutions = {shape (FPV_GATE_*), resolution}: the corner points and the first one again.  Returns the number of points (with
 * out_points NULL nothing is written: a query), or FPV_EINVAL / FPV_EPARAM: a null argument, an unknown kind or shape, a resolution
 * below 1 (1 gives the start value of the reference's linspace), more points than FPV_SPLAT_MAX_POINTS or than ld, ld not a multiple
 * of 4, numbers that are not finite. */
int fpv_cloud_derive(int kind, const double* numbers, const int32_t* resolutions, float* out_points, int64_t ld);
/* One image per drone of the handle at b->state / b->ld on `stream`, under the handle's device: allocates nothing, never
 * synchronises, does not advance the step index and does not touch the rotation.  The struct is checked before the handle is
 * looked at.  FPV_EINVAL / FPV_EALIGN / FPV_EPARAM, by name: null or misaligned pointers, width or height outside 4..128 or width not
 * a multiple of 4, image_ld < W * H or not a multiple of 4, point_ld < first[M] or not a multiple of 4, object_count outside
 * 0..FPV_MAX_BOXES, first not starting at 0, decreasing or past 2^20, a box or an offset that is not finite or a box with min > max,
 * camera numbers that are not fpv_splat_derive's, max_depth not finite or not positive, an unknown encoding, centroid without lit or
 * lit without centroid, fp16 state; FPV_ENODEV for a null handle where there is no device; and in a library built without
 * csrc/fpv_splat.hip. */
int fpv_splat_render(fpv_handle_t h, const fpv_buffers_t* b, const fpv_splat_t* s, void* stream);
/* The kernel's own point and pixel functions on the host (no handle, no device): drone i of n at p[i][3] with attitude q[i][4]
 * (wxyz); every pointer of *s is HOST memory. */
int fpv_splat_eval(const fpv_splat_t* s, int64_t n, const float* p /*[n][3]*/, const float* q /*[n][4] wxyz*/);

const char* fpv_last_error(void);
const char* fpv_error_name(int code);
/* Identifier of what stored bits mean, for checkpoints: 0 = the fp16 state storage words (FPV_FLAG_FP16_STATE), 1 = the
 * in-kernel stick-noise stream.  A checkpoint records the string; a library whose string differs cannot continue it bit for
 * bit (fp16 words: cannot decode it at all).  NULL for any other `which`. */
const char* fpv_encoding_id(int which);

#ifdef __cplusplus
}
#endif
#endif /* FPV_ABI_H */
