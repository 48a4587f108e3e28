// fpv_pursuit.hip - the gfx950 kernel of the pursuit task (include/fpv_abi.h "Pursuit task"), and the host loop over
// the same lane function.
//
// A call advances every drone's own target along its circular path, measures the distance, pays progress and capture, respawns a
// captured target, observes the target in the body frame and - GUIDE - runs the guidance law of fpv_chase.h against that target,
// writing rotation[n][9] / thrust[n] for the next step's override (fpv_pursuit.h fpv_pursuit_task, fpv_pursuit_guide).  Like the
// range scan, the depth camera and the chase it is a kernel of its own behind entry points of its own (fpv_pursuit_step,
// fpv_pursuit_reset), launched after the step: the step kernels, the state, the step counter and the rotation of the traversal stay
// as they are.
//
// One lane = one drone, 128-thread blocks in the plain order.  The ten state loads, the eight target-row loads, the done byte, the
// reward cells of add_to_reward and - GUIDE - the four PID loads go out before the first use; the two table rows follow the COUNT
// word they are indexed by (one 8-byte load each).  Constants, spawn box, rewards and the chase's FpvChaseK are wave-uniform kernel
// arguments, read section by section (pursuit_args_after below).  Of the target rows only COUNT and PREV_DIST are stored by every lane; centre, radius and SPAWNS by a lane that
// respawned or rebased; PATH_R never.  Observation, position, event and the task's reward leave with the streaming hint like the
// other sensors' rows, rotation / thrust with the stores DESIGN 3.9 chose.  No LDS, no barrier; a lane at or past n returns before
// its first load.  RESET: the mask takes the place of the done bytes and a lane outside it stores nothing at all.
//
// A translation unit of its own, linked with the other units into the one libfpv_hip.so; fpv_hip.hip alone still builds (it reaches
// the two functions at the end of this file through weak declarations and answers "not in this build" without them).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_math.h"
#include "fpv_kernels.h"
#include "fpv_pursuit.h"

namespace {

struct alignas(8) PursuitPair { float x, y; };

// A fresh, opaque view of the kernel argument, ordered after `after` (fpv_kernels.h fpv_args_after has the reason): the uniforms of
// the loads, of the task, of its stores, of the law and of its stores are scalar loads of their own section instead of living in
// SGPRs from the first instruction to the last - with one view the GUIDE kernel spilled 8 SGPRs into VGPR lanes.
__device__ __forceinline__ const FpvPursuitArgs& pursuit_args_after(float after)
{
    typedef const __attribute__((address_space(4))) FpvPursuitArgs* P4;
    P4 p = (P4)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p) : "v"(after));
    return *(const FpvPursuitArgs*)p;
}

template <bool GUIDE, bool RESET>
__global__ __launch_bounds__(kStepBlock) void fpv_pursuit_kernel(const FpvPursuitArgs A)
{
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    // ---- 1. the loads of this lane before the first use
    const float px = row_at(ROW(A.state, FPV_PX, A.ld), i), py = row_at(ROW(A.state, FPV_PY, A.ld), i), pz = row_at(ROW(A.state, FPV_PZ, A.ld), i);
    const float vx = row_at(ROW(A.state, FPV_VX, A.ld), i), vy = row_at(ROW(A.state, FPV_VY, A.ld), i), vz = row_at(ROW(A.state, FPV_VZ, A.ld), i);
    FpvQuat q;
    q.w = row_at(ROW(A.state, FPV_QW, A.ld), i); q.x = row_at(ROW(A.state, FPV_QX, A.ld), i);
    q.y = row_at(ROW(A.state, FPV_QY, A.ld), i); q.z = row_at(ROW(A.state, FPV_QZ, A.ld), i);
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(A.targets);
    FpvTarget T;
    T.count = row_at(ROW(words, FPV_TGT_COUNT, A.tld), i);
    T.cx = row_at(ROW(A.targets, FPV_TGT_CX, A.tld), i); T.cy = row_at(ROW(A.targets, FPV_TGT_CY, A.tld), i);
    T.cz = row_at(ROW(A.targets, FPV_TGT_CZ, A.tld), i); T.path_r = row_at(ROW(A.targets, FPV_TGT_PATH_R, A.tld), i);
    T.radius = row_at(ROW(A.targets, FPV_TGT_RADIUS, A.tld), i); T.prev_dist = row_at(ROW(A.targets, FPV_TGT_PREV_DIST, A.tld), i);
    T.spawns = row_at(ROW(words, FPV_TGT_SPAWNS, A.tld), i);
    const uint8_t flag = A.done ? row_at(A.done, i) : (uint8_t)(RESET ? 1 : 0);
    const bool pay = !RESET && A.P.add_to_reward;
    float reward = 0.0f, ep_return = 0.0f;
    if (pay) reward = row_at(A.reward, i);
    if (pay && A.ep_return) ep_return = row_at(A.ep_return, i);
    float integ = 0.0f, dflt = 0.0f, last = 0.0f, first = 1.0f;
    if (GUIDE) {
        integ = row_at(ROW(A.pid_state, FPV_PID_INTEGRAL, A.pid_ld), i); dflt = row_at(ROW(A.pid_state, FPV_PID_PREV_DERIVATIVE, A.pid_ld), i);
        last = row_at(ROW(A.pid_state, FPV_PID_PREV_ERROR, A.pid_ld), i); first = row_at(ROW(A.pid_state, FPV_PID_IS_FIRST, A.pid_ld), i);
    }
    uint32_t at, before;
    fpv_pursuit_indices(T.count, A.P.resolution, A.P.advance != 0, at, before);
    const PursuitPair* const table = reinterpret_cast<const PursuitPair*>(A.circle);
    const PursuitPair a = row_at(table, at), b = row_at(table, before);
    if (RESET && !flag) return;
    const bool rebase = RESET || flag != 0;
    // ---- 2. the task
    FpvPursuitOut o;
    {
        const FpvPursuitArgs& V = pursuit_args_after(a.x);
        fpv_pursuit_task(V.P, V.circle, i, px, py, pz, vx, vy, vz, q, rebase, a.x, a.y, b.x, b.y, T, o);
    }
    // ---- 3. the rows that changed, the payment, the outputs
    {
        const FpvPursuitArgs& V = pursuit_args_after(o.obs[6]);
        uint32_t* const wout = reinterpret_cast<uint32_t*>(V.targets);
        row_at(ROW(wout, FPV_TGT_COUNT, V.tld), i) = T.count;
        row_at(ROW(V.targets, FPV_TGT_PREV_DIST, V.tld), i) = T.prev_dist;
        if (o.respawned || o.rebased) {
            row_at(ROW(V.targets, FPV_TGT_CX, V.tld), i) = T.cx; row_at(ROW(V.targets, FPV_TGT_CY, V.tld), i) = T.cy;
            row_at(ROW(V.targets, FPV_TGT_CZ, V.tld), i) = T.cz; row_at(ROW(V.targets, FPV_TGT_RADIUS, V.tld), i) = T.radius;
            row_at(ROW(wout, FPV_TGT_SPAWNS, V.tld), i) = T.spawns;
        }
        if (pay && !o.rebased) {
            row_at(V.reward, i) = reward + o.paid;
            if (V.ep_return) row_at(V.ep_return, i) = ep_return + o.paid;
        }
        if (V.obs) {
#pragma unroll
            for (int r = 0; r < FPV_PURSUIT_OBS; ++r) ST_OUT(row_at(ROW(V.obs, r, V.obs_ld), i), o.obs[r]);
        }
        if (V.position) {
#pragma unroll
            for (int r = 0; r < 3; ++r) ST_OUT(row_at(ROW(V.position, r, V.pos_ld), i), o.pos[r]);
        }
        if (V.event) ST_OUT(row_at(V.event, i), o.event);
        if (V.reward_out) ST_OUT(row_at(V.reward_out, i), o.paid);
    }
    if (!GUIDE) return;
    // ---- 4. the law against this lane's target; its PID rows and outputs
    FpvChaseOut g;
    bool pid_dirty;
    {
        const FpvPursuitArgs& V = pursuit_args_after(o.pos[0]);
        pid_dirty = fpv_pursuit_guide(V.K, o.pos[0], o.pos[1], o.pos[2], T.radius, px, py, pz, vx, vy, vz, q, rebase, integ, dflt, last, first, g);
    }
    const FpvPursuitArgs& V = pursuit_args_after(g.rot[0]);
    if (pid_dirty) {
        row_at(ROW(V.pid_state, FPV_PID_INTEGRAL, V.pid_ld), i) = integ; row_at(ROW(V.pid_state, FPV_PID_PREV_DERIVATIVE, V.pid_ld), i) = dflt;
        row_at(ROW(V.pid_state, FPV_PID_PREV_ERROR, V.pid_ld), i) = last; row_at(ROW(V.pid_state, FPV_PID_IS_FIRST, V.pid_ld), i) = first;
    }
    float* const rot = V.rotation + (size_t)i * 9u;          // 36 i does not fit a 32-bit lane offset at 2^28 drones
#pragma unroll
    for (int j = 0; j < 9; ++j) ST_OUT(rot[j], g.rot[j]);
    ST_OUT(row_at(V.thrust, i), g.thrust);
    if (V.pixel_out) {
        PursuitPair w; w.x = g.u; w.y = g.v;
        row_at(reinterpret_cast<PursuitPair*>(V.pixel_out), i) = w;
    }
    if (V.visible) ST_OUT(row_at(V.visible, i), (uint8_t)(g.seen ? 1 : 0));
}

template <bool GUIDE>
void pursuit_host(const FpvPursuitArgs* A, const float* p, const float* v, const float* q, bool reset)
{
    uint32_t* const words = reinterpret_cast<uint32_t*>(A->targets);
    for (int64_t i = 0; i < A->n; ++i) {
        const uint8_t flag = A->done ? A->done[i] : (uint8_t)(reset ? 1 : 0);
        if (reset && !flag) continue;
        float* const t = A->targets + i;
        FpvTarget T;
        T.cx = t[FPV_TGT_CX * A->tld]; T.cy = t[FPV_TGT_CY * A->tld]; T.cz = t[FPV_TGT_CZ * A->tld]; T.path_r = t[FPV_TGT_PATH_R * A->tld];
        T.radius = t[FPV_TGT_RADIUS * A->tld]; T.prev_dist = t[FPV_TGT_PREV_DIST * A->tld];
        T.count = words[FPV_TGT_COUNT * A->tld + i]; T.spawns = words[FPV_TGT_SPAWNS * A->tld + i];
        float* const st = GUIDE ? A->pid_state + i : nullptr;
        float integ = 0.0f, dflt = 0.0f, last = 0.0f, first = 1.0f;
        if (GUIDE) {
            integ = st[FPV_PID_INTEGRAL * A->pid_ld]; dflt = st[FPV_PID_PREV_DERIVATIVE * A->pid_ld];
            last = st[FPV_PID_PREV_ERROR * A->pid_ld]; first = st[FPV_PID_IS_FIRST * A->pid_ld];
        }
        uint32_t at, before;
        fpv_pursuit_indices(T.count, A->P.resolution, A->P.advance != 0, at, before);
        FpvQuat a; a.w = q[4 * i]; a.x = q[4 * i + 1]; a.y = q[4 * i + 2]; a.z = q[4 * i + 3];
        const bool rebase = reset || flag != 0;
        FpvPursuitOut o;
        FpvChaseOut g;
        bool pid_dirty = false;
        fpv_pursuit_task(A->P, A->circle, (uint32_t)i, p[3 * i], p[3 * i + 1], p[3 * i + 2], v[3 * i], v[3 * i + 1], v[3 * i + 2], a, rebase,
                         A->circle[2 * at], A->circle[2 * at + 1], A->circle[2 * before], A->circle[2 * before + 1], T, o);
        if (GUIDE)
            pid_dirty = fpv_pursuit_guide(A->K, o.pos[0], o.pos[1], o.pos[2], T.radius, p[3 * i], p[3 * i + 1], p[3 * i + 2], v[3 * i], v[3 * i + 1],
                                          v[3 * i + 2], a, rebase, integ, dflt, last, first, g);
        words[FPV_TGT_COUNT * A->tld + i] = T.count;
        t[FPV_TGT_PREV_DIST * A->tld] = T.prev_dist;
        if (o.respawned || o.rebased) {
            t[FPV_TGT_CX * A->tld] = T.cx; t[FPV_TGT_CY * A->tld] = T.cy; t[FPV_TGT_CZ * A->tld] = T.cz; t[FPV_TGT_RADIUS * A->tld] = T.radius;
            words[FPV_TGT_SPAWNS * A->tld + i] = T.spawns;
        }
        if (!reset && A->P.add_to_reward && !o.rebased) {
            A->reward[i] = A->reward[i] + o.paid;
            if (A->ep_return) A->ep_return[i] = A->ep_return[i] + o.paid;
        }
        if (A->obs) for (int r = 0; r < FPV_PURSUIT_OBS; ++r) A->obs[r * A->obs_ld + i] = o.obs[r];
        if (A->position) for (int r = 0; r < 3; ++r) A->position[r * A->pos_ld + i] = o.pos[r];
        if (A->event) A->event[i] = o.event;
        if (A->reward_out) A->reward_out[i] = o.paid;
        if (GUIDE) {
            if (pid_dirty) {
                st[FPV_PID_INTEGRAL * A->pid_ld] = integ; st[FPV_PID_PREV_DERIVATIVE * A->pid_ld] = dflt;
                st[FPV_PID_PREV_ERROR * A->pid_ld] = last; st[FPV_PID_IS_FIRST * A->pid_ld] = first;
            }
            for (int j = 0; j < 9; ++j) A->rotation[9 * i + j] = g.rot[j];
            A->thrust[i] = g.thrust;
            if (A->pixel_out) { A->pixel_out[2 * i] = g.u; A->pixel_out[2 * i + 1] = g.v; }
            if (A->visible) A->visible[i] = (uint8_t)(g.seen ? 1 : 0);
        }
    }
}

}  // namespace

// what fpv_hip.hip launches (it declares both weak): the kernel with and without the guidance law, for a step and for a reset ...
extern "C" __attribute__((visibility("hidden"))) void* fpv_pursuit_kernel_fn(int guide, int reset)
{
    if (guide) return reset ? reinterpret_cast<void*>(fpv_pursuit_kernel<true, true>) : reinterpret_cast<void*>(fpv_pursuit_kernel<true, false>);
    return reset ? reinterpret_cast<void*>(fpv_pursuit_kernel<false, true>) : reinterpret_cast<void*>(fpv_pursuit_kernel<false, false>);
}

// ... and the lane function over n drones on the host: every pointer of A is host memory, state is not read (p, v, q are AoS)
extern "C" __attribute__((visibility("hidden"))) void fpv_pursuit_eval_host(const FpvPursuitArgs* A, const float* p, const float* v, const float* q,
                                                                            int guide, int reset)
{
    if (guide) pursuit_host<true>(A, p, v, q, reset != 0);
    else pursuit_host<false>(A, p, v, q, reset != 0);
}
