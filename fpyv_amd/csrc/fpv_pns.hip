// fpv_pns.hip - the gfx950 kernel of point and shoot (include/fpv_abi.h "Point and shoot"), and the host loop over the
// same lane function.
//
// A call reads a drone's position, velocity and attitude, its four guidance-PID rows, its two prev_pixel rows, its four commands and
// either its pixel or its target's centre, and writes the rotation matrix and the thrust force the reference's steered guidance law
// asks for (fpv_pns.h fpv_pns_lane), in the layout the step kernels' override reads: rotation[n][9], thrust[n].  Like the chase it is
// a kernel of its own behind an entry point of its own (fpv_pns_guide): the step kernels, the state, the step counter and the
// rotation of the traversal stay as they are.
//
// One lane = one drone, 128-thread blocks in the plain order.  Every load of the lane goes out before the first use; the camera and
// the law's constants are wave-uniform kernel arguments.  The thrust limit is a closed form: the kernel has no loop.  The PID and
// prev_pixel rows are SoA and are stored back only by guided (or restarted) lanes.  The [n][9] output leaves through the chase's
// per-lane stores, the outputs with the streaming hint; no LDS, no barrier; a lane at or past n returns before its
// first load.
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
#include "fpv_pns.h"

namespace {

struct alignas(8) PnsPair { float x, y; };
struct alignas(16) PnsAction { float a0, a1, a2, a3; };

template <bool PIXEL>
__global__ __launch_bounds__(kStepBlock) void fpv_pns_kernel(const FpvPnsArgs A)
{
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    // ---- 1. the loads of this lane before the first use
    const float px = row_at(ROW(A.state, FPV_PX, A.ld), i), py = row_at(ROW(A.state, FPV_PY, A.ld), i), pz = row_at(ROW(A.state, FPV_PZ, A.ld), i);
    const float vx = row_at(ROW(A.state, FPV_VX, A.ld), i), vy = row_at(ROW(A.state, FPV_VY, A.ld), i), vz = row_at(ROW(A.state, FPV_VZ, A.ld), i);
    FpvQuat q;
    q.w = row_at(ROW(A.state, FPV_QW, A.ld), i); q.x = row_at(ROW(A.state, FPV_QX, A.ld), i);
    q.y = row_at(ROW(A.state, FPV_QY, A.ld), i); q.z = row_at(ROW(A.state, FPV_QZ, A.ld), i);
    float integ = row_at(ROW(A.pid_state, FPV_PID_INTEGRAL, A.pid_ld), i), dflt = row_at(ROW(A.pid_state, FPV_PID_PREV_DERIVATIVE, A.pid_ld), i);
    float last = row_at(ROW(A.pid_state, FPV_PID_PREV_ERROR, A.pid_ld), i), first = row_at(ROW(A.pid_state, FPV_PID_IS_FIRST, A.pid_ld), i);
    float ppx = row_at(ROW(A.prev_pixel, 0, A.prev_ld), i), ppy = row_at(ROW(A.prev_pixel, 1, A.prev_ld), i);
    PnsPair pix = {0.0f, 0.0f};
    float tcx = A.K.tc[0], tcy = A.K.tc[1], tcz = A.K.tc[2];
    if (PIXEL) {
        pix = row_at(reinterpret_cast<const PnsPair*>(A.pixel), i);
    } else if (A.target_rows) {
        tcx = row_at(ROW(A.target_rows, 0, A.target_ld), i); tcy = row_at(ROW(A.target_rows, 1, A.target_ld), i);
        tcz = row_at(ROW(A.target_rows, 2, A.target_ld), i);
    }
    PnsAction act = {0.0f, 0.0f, 0.0f, 0.0f};
    if (A.action) act = row_at(reinterpret_cast<const PnsAction*>(A.action), i);
    const bool restart = A.restart ? row_at(A.restart, i) != 0 : false;
    // ---- 2. the law
    FpvPnsOut o;
    fpv_pns_lane(A.K, tcx, tcy, tcz, px, py, pz, vx, vy, vz, q, PIXEL, pix.x, pix.y, act.a0, act.a1, act.a2, act.a3, restart, integ, dflt, last,
                 first, ppx, ppy, o);
    // ---- 3. the PID and prev_pixel rows of a guided or restarted lane; the outputs of every lane
    if (o.guided || restart) {
        row_at(ROW(A.pid_state, FPV_PID_INTEGRAL, A.pid_ld), i) = integ; row_at(ROW(A.pid_state, FPV_PID_PREV_DERIVATIVE, A.pid_ld), i) = dflt;
        row_at(ROW(A.pid_state, FPV_PID_PREV_ERROR, A.pid_ld), i) = last; row_at(ROW(A.pid_state, FPV_PID_IS_FIRST, A.pid_ld), i) = first;
        row_at(ROW(A.prev_pixel, 0, A.prev_ld), i) = ppx; row_at(ROW(A.prev_pixel, 1, A.prev_ld), i) = ppy;
    }
    float* const rot = A.rotation + (size_t)i * 9u;          // 36 i does not fit a 32-bit lane offset at 2^28 drones
#pragma unroll
    for (int j = 0; j < 9; ++j) ST_OUT(rot[j], o.rot[j]);
    ST_OUT(row_at(A.thrust, i), o.thrust);
    if (A.pixel_velocity) {
        PnsPair w; w.x = o.velx; w.y = o.vely;
        row_at(reinterpret_cast<PnsPair*>(A.pixel_velocity), i) = w;
    }
    if (A.limited) ST_OUT(row_at(A.limited, i), o.limited);
    if (A.visible) ST_OUT(row_at(A.visible, i), (uint8_t)(o.seen ? 1 : 0));
    if (A.throttle) ST_OUT(row_at(A.throttle, i), o.throttle);
}

}  // namespace

// what fpv_hip.hip launches (it declares both weak): the kernel with and without a supplied pixel ...
extern "C" __attribute__((visibility("hidden"))) void* fpv_pns_kernel_fn(int pixel)
{
    return pixel ? reinterpret_cast<void*>(fpv_pns_kernel<true>) : reinterpret_cast<void*>(fpv_pns_kernel<false>);
}

// ... and the lane function over n drones on the host: every pointer of A is host memory, state is not read (p, v, q are AoS)
extern "C" __attribute__((visibility("hidden"))) void fpv_pns_eval_host(const FpvPnsArgs* A, const float* p, const float* v, const float* q)
{
    for (int64_t i = 0; i < A->n; ++i) {
        float* const st = A->pid_state + i;
        float* const pp = A->prev_pixel + i;
        float integ = st[FPV_PID_INTEGRAL * A->pid_ld], dflt = st[FPV_PID_PREV_DERIVATIVE * A->pid_ld];
        float last = st[FPV_PID_PREV_ERROR * A->pid_ld], first = st[FPV_PID_IS_FIRST * A->pid_ld];
        float ppx = pp[0], ppy = pp[A->prev_ld];
        FpvQuat a; a.w = q[4 * i]; a.x = q[4 * i + 1]; a.y = q[4 * i + 2]; a.z = q[4 * i + 3];
        float tc[3] = {A->K.tc[0], A->K.tc[1], A->K.tc[2]};
        if (!A->pixel && A->target_rows)
            for (int k = 0; k < 3; ++k) tc[k] = A->target_rows[k * A->target_ld + i];
        float act[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (A->action)
            for (int k = 0; k < 4; ++k) act[k] = A->action[4 * i + k];
        const bool restart = A->restart && A->restart[i] != 0;
        FpvPnsOut o;
        fpv_pns_lane(A->K, tc[0], tc[1], tc[2], p[3 * i], p[3 * i + 1], p[3 * i + 2], v[3 * i], v[3 * i + 1], v[3 * i + 2], a, A->pixel != nullptr,
                     A->pixel ? A->pixel[2 * i] : 0.0f, A->pixel ? A->pixel[2 * i + 1] : 0.0f, act[0], act[1], act[2], act[3], restart, integ, dflt,
                     last, first, ppx, ppy, o);
        if (o.guided || restart) {
            st[FPV_PID_INTEGRAL * A->pid_ld] = integ; st[FPV_PID_PREV_DERIVATIVE * A->pid_ld] = dflt;
            st[FPV_PID_PREV_ERROR * A->pid_ld] = last; st[FPV_PID_IS_FIRST * A->pid_ld] = first;
            pp[0] = ppx; pp[A->prev_ld] = ppy;
        }
        for (int j = 0; j < 9; ++j) A->rotation[9 * i + j] = o.rot[j];
        A->thrust[i] = o.thrust;
        if (A->pixel_velocity) { A->pixel_velocity[2 * i] = o.velx; A->pixel_velocity[2 * i + 1] = o.vely; }
        if (A->limited) A->limited[i] = o.limited;
        if (A->visible) A->visible[i] = (uint8_t)(o.seen ? 1 : 0);
        if (A->throttle) A->throttle[i] = o.throttle;
    }
}
