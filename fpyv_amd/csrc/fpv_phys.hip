// fpv_phys.hip - the gfx950 kernels of per-drone physics (include/fpv_abi.h "Per-drone physics").
//
// Every drone of a handle with a physics table flies its own airframe: the thirteen constants of the step that depend on mass,
// thrust cubic, drag and the two low-pass rates come from the drone's column of a read-only table phys[FPV_PHYS_ROWS][ld] instead
// of the kernel argument.  The arithmetic is fpv_math.h's lane function, unchanged - it takes its constants through a template
// parameter, and FpvKLane below has FpvK's field names: the table values in VGPRs, the uniform ones forwarded from the kernel
// argument.  An operation reads the same IEEE operands whether a constant sits in an SGPR or a VGPR, so a drone steps bit for bit
// like a drone of a homogeneous handle with its parameters (tests/test_gpu_physics.py).
//
// A translation unit of its own, linked with fpv_hip.hip into the one libfpv_hip.so: fpv_hip.hip's 42 kernels stay exactly as
// they are, and fpv_hip.hip alone still builds (it reaches the two lookup functions at the end of this file through weak
// declarations).  Kahan rows, the guidance override, the AoS head, fp16 state and the Racer have no table kernel: the host
// refuses those combinations by name.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_math.h"
#include "fpv_kernels.h"

namespace {

// one drone's column of the table, in registers
struct FpvPhysRegs { float v[FPV_PHYS_ROWS]; };

// The table is read every step and never written.  Read with ordinary loads it competes with the state rows for the L2 lines the
// rotated traversal comes back for; read with the streaming hint it leaves them alone and is served by the Infinity Cache (46 MB of
// table + 59 MB of state at 2^20 drones).  Measured in one process (profiles/exp_phys_table_loads.log): the hint is worth 6.8 % at
// 2^20 drones and 13 % at 2^23 with the rotated traversal - it is shipped -, and costs 4 % at 2^20 in the plain order, where no
// state row is found again anyway.  -DFPV_EXP_PHYS_TABLE_NT=0 builds the ordinary loads (fpv_exp.h).
__device__ __forceinline__ float ld_phys_row(const float* __restrict__ phys, int r, int64_t ld, uint32_t i)
{
#if FPV_EXP_PHYS_TABLE_NT
    return __builtin_nontemporal_load(&row_at(ROW(phys, r, ld), i));
#else
    return row_at(ROW(phys, r, ld), i);
#endif
}

// `ground` is wave-uniform: the two ground rows are loaded only by launches that can use them (FPV_FLAG_GROUND or an object list)
template <bool ALWAYS_GROUND>
__device__ __forceinline__ void ld_phys(const float* __restrict__ phys, int64_t ld, uint32_t i, bool ground, FpvPhysRegs& T)
{
#pragma unroll
    for (int r = 0; r < FPV_PHYS_GROUND_K_M; ++r) T.v[r] = ld_phys_row(phys, r, ld, i);
    T.v[FPV_PHYS_GROUND_K_M] = T.v[FPV_PHYS_GROUND_C_M] = 0.0f;
    if (ALWAYS_GROUND || ground) {
        T.v[FPV_PHYS_GROUND_K_M] = ld_phys_row(phys, FPV_PHYS_GROUND_K_M, ld, i);
        T.v[FPV_PHYS_GROUND_C_M] = ld_phys_row(phys, FPV_PHYS_GROUND_C_M, ld, i);
    }
}

// FpvK as fpv_drone_step_lane / fpv_collide_objects read it, per lane: the thirteen table constants from registers, the rest
// from the uniform constants U (only what the lane function reads of them).  max_rates - and with it angle_mode - stays uniform.
struct FpvKLane {
    float rate_gain, rate_lim, omkr, omkt, dk3, dk2, dk1, dk0, kdrag_m[3], inv_mass, ground_k_m, ground_c_m;
    float dt, g, half_k, motor_x[4], motor_y[4], motor_c, motor_radius, contact_reach, ceiling, goal[3];
    uint32_t flags, angle_mode;
    __device__ __forceinline__ FpvKLane(const FpvK& U, const FpvPhysRegs& T)
        : rate_gain(-T.v[FPV_PHYS_RATE_LIM]), rate_lim(T.v[FPV_PHYS_RATE_LIM]), omkr(T.v[FPV_PHYS_OMKR]), omkt(T.v[FPV_PHYS_OMKT]),
          dk3(T.v[FPV_PHYS_DK3]), dk2(T.v[FPV_PHYS_DK2]), dk1(T.v[FPV_PHYS_DK1]), dk0(T.v[FPV_PHYS_DK0]),
          kdrag_m{T.v[FPV_PHYS_KDRAG_X], T.v[FPV_PHYS_KDRAG_Y], T.v[FPV_PHYS_KDRAG_Z]}, inv_mass(T.v[FPV_PHYS_INV_MASS]),
          ground_k_m(T.v[FPV_PHYS_GROUND_K_M]), ground_c_m(T.v[FPV_PHYS_GROUND_C_M]),
          dt(U.dt), g(U.g), half_k(U.half_k), motor_x{U.motor_x[0], U.motor_x[1], U.motor_x[2], U.motor_x[3]},
          motor_y{U.motor_y[0], U.motor_y[1], U.motor_y[2], U.motor_y[3]}, motor_c(U.motor_c), motor_radius(U.motor_radius),
          contact_reach(U.contact_reach), ceiling(U.ceiling), goal{U.goal[0], U.goal[1], U.goal[2]}, flags(U.flags), angle_mode(U.angle_mode)
    {
    }
};

// One step with a table: fpv_drone_step_kernel<NOISE, OBJ> (fpv_hip.hip; read the comments above FPV_STEP_PARAMS there) with
// the table loads in its load block.  The leading scalars are FPV_STEP_PARAMS' with the table base in the slot of state_h - a
// table handle has no fp16 state -, so all six are preloaded into SGPRs and the 11 or 13 table loads go out with the 14 state
// loads, before anything has to be waited for; whether the two ground rows are among them is bit 31 of n_start's low word
// (kPhysGroundBit), decided by the host (plan_launch), so that test reads a preloaded SGPR too.  The traversal rotates like every single-step
// kernel's (fpv_hip.hip: launch_step / rotation_blocks; the table is only read and does not count among the written bytes).
template <bool NOISE, bool OBJ>
__global__ __launch_bounds__(kStepBlock) void fpv_drone_step_phys_kernel(float* __restrict__ a_state, const int64_t a_ld,
                                                                         const float4* __restrict__ a_action, const int64_t a_action_ld,
                                                                         const float* __restrict__ a_phys, const int64_t n_start,
                                                                         const FpvK K, const FpvBufD B_)
{
    constexpr bool SECTIONED = NOISE;
    const FpvBufD B = fpv_step_view(B_, a_state, a_ld, a_action, a_action_ld, nullptr);
    __shared__ FpvNormalRow ntab[NOISE ? FPV_NTAB_ROWS : 1];
    if (NOISE) stage_normal_table(ntab);
    // FPV_STEP_INDEX, with n below the ground bit
    const int64_t n = n_start & 0x7fffffffll;
    const bool ground = (n_start & kPhysGroundBit) != 0;
    const uint32_t nblk_ = (uint32_t)((n + 8 * kStepBlock - 1) / (8 * kStepBlock)) * 8u;
    uint32_t blk_ = blockIdx.x + (uint32_t)(n_start >> 32);
    blk_ = blk_ >= nblk_ ? blk_ - nblk_ : blk_;
    const uint32_t i = blk_ * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= n) return;
    FpvDroneState s;
    FpvPhysRegs T;
    // ---- 1. every load of this lane - sticks, state, table - before the first use
    float4 a = (!NOISE || B.action) ? ld_action_any(B.action, B.action_ld, i) : make_float4(0.f, 0.f, 0.f, 0.f);
    ld_drone(B.state, B.ld, i, s);
    ld_phys<OBJ>(a_phys, a_ld, i, ground, T);
    if (NOISE) {
        // the generator's own rows and uniforms come from the kernel argument: fenced off, so that its scalar-load wait does not
        // land in front of the last state and table loads
        __builtin_amdgcn_sched_barrier(0);
        a = apply_stick_noise(K, B, i, a, ntab);
    }
    __builtin_amdgcn_sched_barrier(0);       // vector loads first, the scalar loads of the uniform constants after (fpv_drone_step_kernel)
    // ---- 2. the physics, on its own view of the uniform constants when SECTIONED
    const FpvStepArgs* P = nullptr;
    if (SECTIONED) P = &fpv_step_args_again();
    const FpvK& Kp = SECTIONED ? P->K : K;
    const FpvBufD& Bp = SECTIONED ? P->B : B;
    const FpvStepOut o = fpv_drone_step_lane<OBJ>(FpvKLane(Kp, T), s, a.x, a.y, a.z, a.w, Bp.wx, Bp.wy, Bp.wz, &B_.objs);
    // ---- 3. the stores
    uint32_t j = i;
    if (OBJ || SECTIONED) FPV_KEEP_HERE(j);
    const FpvStepArgs* E = nullptr;
    if (SECTIONED) E = &fpv_step_args_again();
    const FpvK& Ke = SECTIONED ? E->K : K;
    FpvBufD Bs = B;
    if (SECTIONED) { Bs = E->B; Bs.state = E->state; Bs.ld = E->ld; }
    const FpvBufD& Be = Bs;
    if (Be.accel) {
        ST_OUT(row_at(ROW(Be.accel, 0, Be.ld), j), o.ax); ST_OUT(row_at(ROW(Be.accel, 1, Be.ld), j), o.ay); ST_OUT(row_at(ROW(Be.accel, 2, Be.ld), j), o.az);
    }
    if ((Ke.flags & FPV_FLAG_AUTO_RESET) && o.done) fpv_drone_reset_lane(Ke, s);       // a reset lane keeps its physics: the table is not touched
    st_drone(Be.state, Be.ld, j, s);
    emit_outputs(Be, j, true, o.reward, o.done);
}

// k steps with a table in ONE launch: fpv_drone_rollout_kernel<NOISE, OBJ, false, false> (fpv_hip.hip) with the drone's table
// column loaded once before the loop, settled with the state and held in VGPRs for all k steps - per env-step the table costs
// 44/k or 52/k bytes.  It carries the reset-source branch (reset-pose table, jitter), so a handle with per-drone starts AND
// per-drone physics runs here, its single steps included (k = 1).  Sections and argument views as in fpv_drone_rollout_kernel: the
// views read FpvRollArgs at the head of the kernel-argument segment, which is where FpvRollPhysArgs keeps it.
template <bool NOISE, bool OBJ>
__global__ __launch_bounds__(kStepBlock) void fpv_drone_rollout_phys_kernel(const FpvRollPhysArgs PA)
{
    const FpvRollArgs& A = PA.A;
    __shared__ FpvNormalRow ntab[NOISE ? FPV_NTAB_ROWS : 1];
    if (NOISE) stage_normal_table(ntab);
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    FpvDroneState s;
    FpvPhysRegs T;
    const int k = A.R.k;
    const bool has_action = !NOISE || A.B.action;
    float4 a_next = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_action) a_next = ld_action_any(A.B.action, A.B.action_ld, i);
    ld_drone(A.B.state, A.B.ld, i, s);
    ld_phys<OBJ>(PA.phys, A.B.ld, i, PA.ground != 0, T);
    float ns[4] = {0.f, 0.f, 0.f, 0.f};
    if (NOISE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ns[c] = row_at(ROW(A.B.noise_state, c, A.B.ld), i);
    }
    fpv_settle(s.px); fpv_settle(s.py); fpv_settle(s.pz); fpv_settle(s.vx); fpv_settle(s.vy); fpv_settle(s.vz);
    fpv_settle(s.q.w); fpv_settle(s.q.x); fpv_settle(s.q.y); fpv_settle(s.q.z);
    fpv_settle(s.rx); fpv_settle(s.ry); fpv_settle(s.rz); fpv_settle(s.thrust);
#pragma unroll
    for (int r = 0; r < FPV_PHYS_ROWS; ++r) fpv_settle(T.v[r]);
    if (NOISE) { fpv_settle(ns[0]); fpv_settle(ns[1]); fpv_settle(ns[2]); fpv_settle(ns[3]); }
    float av[4] = {0.f, 0.f, 0.f, 0.f};

    auto one_step = [&](const FpvRollArgs& V, const FpvObjects* objs, const float* ap_next, bool prefetch, int t, auto quiet_c) -> FpvStepOut {
        constexpr bool QUIET = decltype(quiet_c)::value;
        av[0] = a_next.x; av[1] = a_next.y; av[2] = a_next.z; av[3] = a_next.w;
        if ((!NOISE || has_action) && (QUIET || prefetch)) a_next = ld_action(reinterpret_cast<const float4*>(ap_next), i);
        if (NOISE) {
            const FpvRollArgs& NV = OBJ ? fpv_args_again() : V;
            FpvNoiseK N = NV.K.noise;
            asm volatile("" : "+s"(N.seed_lo), "+s"(N.seed_hi));
            fpv_stick_noise(N, NV.B.step + (uint64_t)t, (uint64_t)i, ntab, ns, av);
        }
        FpvStepOut o = fpv_drone_step_lane<OBJ, !QUIET, false>(FpvKLane(V.K, T), s, av[0], av[1], av[2], av[3], V.B.wx, V.B.wy, V.B.wz, objs);
        if ((V.K.flags & FPV_FLAG_AUTO_RESET) && o.done) {
            // rare: the reset pose comes through its own view, inside the branch; the lane keeps its physics
            const FpvRollArgs& Z = fpv_args_again();
            fpv_drone_reset_lane(Z.K, s);
            apply_reset_source_k(i, (uint64_t)t, s);
        }
        return o;
    };

    int t = 0;
    if (A.B.ep_return == nullptr && A.R.out_stride == 0 && k > 1) {
        // ---- 1. quiet steps: only the optional per-step done_bits row leaves the lane
        const float* ap = reinterpret_cast<const float*>(A.B.action);
        const int64_t astride = A.R.action_stride;
        unsigned long long* bp = A.R.bits_stride ? A.B.done_bits : nullptr;
        const int64_t bstride = A.R.bits_stride;
        auto quiet_step = [&]() {
            ap += astride;
            const FpvStepOut o = one_step(A, &A.B.objs, ap, true, t, std::true_type{});
            if (bp) {
                const unsigned long long mask = __ballot(o.done);
                if ((threadIdx.x & 63) == 0) bp[i >> 6] = mask;
                bp += bstride;
            }
            ++t;
        };
        if constexpr (!OBJ) { while (t + 1 < k - 1) { quiet_step(); quiet_step(); } }      // two steps per trip (fpv_drone_rollout_kernel)
        while (t < k - 1) quiet_step();
    }
    // ---- 2. the remaining steps, with every output the caller asked for
    FpvStepOut o;
    o.done = false; o.reward = 0.0f; o.ax = o.ay = o.az = 0.0f;
    {
        const FpvRollArgs& G = fpv_args_again();
        RollOut out(G.B, G.R, i, true);
        if (out.bp) out.bp += (int64_t)t * G.R.bits_stride;
        const float* ap = reinterpret_cast<const float*>(G.B.action) + (int64_t)t * G.R.action_stride;
        const int kk = G.R.k;
        if (out.track) { fpv_settle(out.ep_r); fpv_settle(__int_as_float(out.ep_l)); }
        for (; t < kk; ++t) {
            ap += G.R.action_stride;
            o = one_step(G, &G.B.objs, ap, G.R.action_stride != 0 && t + 1 < kk, t, std::false_type{});
            out.template step<false>(i, t, o.reward, o.done);
        }
        out.finish(i, fpv_args_again().B);
    }
    // ---- 3. the stores
    const FpvRollArgs& E = fpv_args_again();
    uint32_t j = i;
    asm volatile("" : "+v"(j));
    if (E.B.accel) {
        ST_OUT(row_at(ROW(E.B.accel, 0, E.B.ld), j), o.ax); ST_OUT(row_at(ROW(E.B.accel, 1, E.B.ld), j), o.ay); ST_OUT(row_at(ROW(E.B.accel, 2, E.B.ld), j), o.az);
    }
    st_drone(E.B.state, E.B.ld, j, s);
    if (NOISE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) row_at(ROW(E.B.noise_state, c, E.B.ld), j) = ns[c];
        if (E.B.action_out) E.B.action_out[j] = make_float4(av[0], av[1], av[2], av[3]);
    }
}

typedef void (*PhysStepFn)(float*, const int64_t, const float4*, const int64_t, const float*, const int64_t, const FpvK, const FpvBufD);
typedef void (*PhysRollFn)(const FpvRollPhysArgs);
const PhysStepFn kPhysStep[2][2] = {{fpv_drone_step_phys_kernel<false, false>, fpv_drone_step_phys_kernel<false, true>},
                                    {fpv_drone_step_phys_kernel<true, false>, fpv_drone_step_phys_kernel<true, true>}};
const PhysRollFn kPhysRoll[2][2] = {{fpv_drone_rollout_phys_kernel<false, false>, fpv_drone_rollout_phys_kernel<false, true>},
                                    {fpv_drone_rollout_phys_kernel<true, false>, fpv_drone_rollout_phys_kernel<true, true>}};

}  // namespace

// what fpv_hip.hip launches (it declares these two weak): the kernel of an instantiation [stick noise][object list]
extern "C" __attribute__((visibility("hidden"))) void* fpv_phys_step_kernel(int noise, int obj)
{
    return reinterpret_cast<void*>(kPhysStep[noise != 0][obj != 0]);
}

extern "C" __attribute__((visibility("hidden"))) void* fpv_phys_roll_kernel(int noise, int obj)
{
    return reinterpret_cast<void*>(kPhysRoll[noise != 0][obj != 0]);
}
