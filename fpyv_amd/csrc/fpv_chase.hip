// fpv_chase.hip - the gfx950 kernel of the target chase (include/fpv_abi.h "Target chase"), and the host loop over the
// same lane function.
//
// A call reads a drone's position, velocity and attitude and its four guidance-PID rows and writes the rotation matrix and the
// thrust force the reference's vision guidance law asks for (fpv_chase.h fpv_chase_lane), in the layout the step kernels' override
// reads: rotation[n][9], thrust[n].  Like the range scan and the depth camera it is a kernel of its own behind an entry point of its
// own (fpv_chase_guide): the step kernels, the state, the step counter and the rotation of the traversal stay as they are.
//
// One lane = one drone, 128-thread blocks in the plain order.  The ten state loads, the four PID loads and the pixel load go out
// before the first use; the camera, the target and the law's constants are wave-uniform kernel arguments (scalar loads, no per-lane
// table).  The PID rows are SoA and are stored back only by guided lanes.  The [n][9] output is 36 bytes per lane, lane stride 36
// bytes: the nine stores of a lane compile to two 16-byte stores and one dword store at a 4-byte aligned address, and a wave's
// three store instructions together cover one contiguous 2304-byte span - no LDS, no barrier and no tail logic (DESIGN 3.9 has the
// choice against the AoS head's LDS transpose).  Outputs leave with the streaming hint like the other sensors' rows; a lane at or
// past n returns before its first load.
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
#include "fpv_chase.h"

namespace {

struct alignas(8) ChasePixel { float x, y; };

template <bool PIXEL>
__global__ __launch_bounds__(kStepBlock) void fpv_chase_kernel(const FpvChaseArgs A)
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
    ChasePixel pix = {0.0f, 0.0f};
    if (PIXEL) pix = row_at(reinterpret_cast<const ChasePixel*>(A.pixel), i);
    // ---- 2. the law
    FpvChaseOut o;
    fpv_chase_lane(A.K, px, py, pz, vx, vy, vz, q, PIXEL, pix.x, pix.y, integ, dflt, last, first, o);
    // ---- 3. the PID rows of a guided lane; the outputs of every lane
    if (o.guided) {
        row_at(ROW(A.pid_state, FPV_PID_INTEGRAL, A.pid_ld), i) = integ; row_at(ROW(A.pid_state, FPV_PID_PREV_DERIVATIVE, A.pid_ld), i) = dflt;
        row_at(ROW(A.pid_state, FPV_PID_PREV_ERROR, A.pid_ld), i) = last; row_at(ROW(A.pid_state, FPV_PID_IS_FIRST, A.pid_ld), i) = first;
    }
    float* const rot = A.rotation + (size_t)i * 9u;          // 36 i does not fit a 32-bit lane offset at 2^28 drones
#pragma unroll
    for (int j = 0; j < 9; ++j) ST_OUT(rot[j], o.rot[j]);
    ST_OUT(row_at(A.thrust, i), o.thrust);
    if (A.pixel_out) {
        ChasePixel w; w.x = o.u; w.y = o.v;
        row_at(reinterpret_cast<ChasePixel*>(A.pixel_out), i) = w;
    }
    if (A.visible) ST_OUT(row_at(A.visible, i), (uint8_t)(o.seen ? 1 : 0));
}

}  // namespace

// what fpv_hip.hip launches (it declares both weak): the kernel with and without a supplied pixel ...
extern "C" __attribute__((visibility("hidden"))) void* fpv_chase_kernel_fn(int pixel)
{
    return pixel ? reinterpret_cast<void*>(fpv_chase_kernel<true>) : reinterpret_cast<void*>(fpv_chase_kernel<false>);
}

// ... and the lane function over n drones on the host: every pointer of A is host memory, state is not read (p, v, q are AoS)
extern "C" __attribute__((visibility("hidden"))) void fpv_chase_eval_host(const FpvChaseArgs* A, const float* p, const float* v, const float* q)
{
    for (int64_t i = 0; i < A->n; ++i) {
        float* const st = A->pid_state + i;
        float integ = st[FPV_PID_INTEGRAL * A->pid_ld], dflt = st[FPV_PID_PREV_DERIVATIVE * A->pid_ld];
        float last = st[FPV_PID_PREV_ERROR * A->pid_ld], first = st[FPV_PID_IS_FIRST * A->pid_ld];
        FpvQuat a; a.w = q[4 * i]; a.x = q[4 * i + 1]; a.y = q[4 * i + 2]; a.z = q[4 * i + 3];
        FpvChaseOut o;
        fpv_chase_lane(A->K, p[3 * i], p[3 * i + 1], p[3 * i + 2], v[3 * i], v[3 * i + 1], v[3 * i + 2], a, A->pixel != nullptr,
                       A->pixel ? A->pixel[2 * i] : 0.0f, A->pixel ? A->pixel[2 * i + 1] : 0.0f, integ, dflt, last, first, o);
        if (o.guided) {
            st[FPV_PID_INTEGRAL * A->pid_ld] = integ; st[FPV_PID_PREV_DERIVATIVE * A->pid_ld] = dflt;
            st[FPV_PID_PREV_ERROR * A->pid_ld] = last; st[FPV_PID_IS_FIRST * A->pid_ld] = first;
        }
        for (int j = 0; j < 9; ++j) A->rotation[9 * i + j] = o.rot[j];
        A->thrust[i] = o.thrust;
        if (A->pixel_out) { A->pixel_out[2 * i] = o.u; A->pixel_out[2 * i + 1] = o.v; }
        if (A->visible) A->visible[i] = (uint8_t)(o.seen ? 1 : 0);
    }
}
