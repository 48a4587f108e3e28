// fpv_detect.hip - the gfx950 kernel of the object detections (include/fpv_abi.h "Object detections"), and the host loop
// over the same lane function.
//
// A call reads a drone's position and attitude and writes, for each of up to 72 axis-aligned world boxes - the collidable objects of
// the object list, the gates of the course, optionally the drone's own pursuit target - the box of its in-front corners on the image
// plane, the smallest in-front depth and whether the reference's pruning rule keeps it (fpv_detect.h fpv_detect_lane, the function
// fpv_detect_eval runs).  Like the range scan it reads p and q only and is a kernel of its own behind an entry point of its own
// (fpv_detect_boxes): the step kernels, the state, the step counter and the rotation of the traversal stay as they are.
//
// One lane = one drone, 128-thread blocks in the plain order; blockIdx.y selects a group of up to 8 consecutive slots, so a small
// batch with many boxes still fills the chip (72 boxes: nine times the workgroups) and a lane's loop is at most eight boxes long,
// at the price of reading the pose and forming the camera's rotation once per group.  The seven pose loads (ten with the own-target
// slot, which only the last group reads) go out before the first use.  The box table travels BY VALUE in the kernel argument: a
// moving Target costs no upload, and the slot index is wave-uniform, so a box arrives through scalar loads from the argument
// segment - no scratch (tests/test_isa_detect.py).  The outputs are SoA rows like the ranges - boxes[slot][4][ld], depth[slot][ld],
// visible[slot][ld] -: every store is a coalesced row store, write-only, with the streaming hint.  No LDS, no barrier; a lane at or
// past n returns before its first load; slots at or past count are not written.
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
#include "fpv_detect.h"

namespace {

template <bool OWN>
__global__ __launch_bounds__(kStepBlock) void fpv_detect_kernel(const FpvDetectArgs A)
{
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    const int s0 = (int)blockIdx.y * FPV_DETECT_GROUP;
    const int s1 = s0 + FPV_DETECT_GROUP < A.count ? s0 + FPV_DETECT_GROUP : A.count;
    // ---- 1. the loads of this lane before the first use
    const float px = row_at(ROW(A.state, FPV_PX, A.ld), i), py = row_at(ROW(A.state, FPV_PY, A.ld), i), pz = row_at(ROW(A.state, FPV_PZ, A.ld), i);
    FpvQuat q;
    q.w = row_at(ROW(A.state, FPV_QW, A.ld), i); q.x = row_at(ROW(A.state, FPV_QX, A.ld), i);
    q.y = row_at(ROW(A.state, FPV_QY, A.ld), i); q.z = row_at(ROW(A.state, FPV_QZ, A.ld), i);
    float tx = 0.0f, ty = 0.0f, tz = 0.0f, tr = A.K.tr;
    if (OWN && s1 == A.count) {                              // (uniform: the group that holds the last slot)
        tx = row_at(ROW(A.target_rows, 0, A.target_ld), i); ty = row_at(ROW(A.target_rows, 1, A.target_ld), i);
        tz = row_at(ROW(A.target_rows, 2, A.target_ld), i);
        if (A.target_radius) tr = row_at(A.target_radius, i);
    }
    // ---- 2. the camera's pose once, then a box per slot of the group: six row stores each
    const FpvDetectPose P = fpv_detect_pose(A.K, px, py, pz, q);
    for (int s = s0; s < s1; ++s) {
        float mn[3], mx[3];
        if (OWN && s == A.table_count) {
            fpv_detect_own_box(tx, ty, tz, tr, mn, mx);
        } else {
            const float* const b = A.box[s];
            mn[0] = b[0]; mn[1] = b[1]; mn[2] = b[2]; mx[0] = b[3]; mx[1] = b[4]; mx[2] = b[5];
        }
        FpvDetectOut o;
        fpv_detect_lane(A.K, P, mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], o);
        float* const row = A.boxes + (int64_t)s * 4 * A.out_ld;
        ST_OUT(row_at(ROW(row, 0, A.out_ld), i), o.x0); ST_OUT(row_at(ROW(row, 1, A.out_ld), i), o.y0);
        ST_OUT(row_at(ROW(row, 2, A.out_ld), i), o.x1); ST_OUT(row_at(ROW(row, 3, A.out_ld), i), o.y1);
        ST_OUT(row_at(ROW(A.depth, s, A.out_ld), i), o.depth);
        ST_OUT(row_at(ROW(A.visible, s, A.out_ld), i), (uint8_t)(o.visible ? 1 : 0));
    }
}

}  // namespace

// what fpv_hip.hip launches (it declares both weak): the kernel with and without the own-target slot ...
extern "C" __attribute__((visibility("hidden"))) void* fpv_detect_kernel_fn(int own)
{
    return own ? reinterpret_cast<void*>(fpv_detect_kernel<true>) : reinterpret_cast<void*>(fpv_detect_kernel<false>);
}

// ... and the lane function over n drones on the host: every pointer of A is host memory, state is not read (p, q are AoS)
extern "C" __attribute__((visibility("hidden"))) void fpv_detect_eval_host(const FpvDetectArgs* A, const float* p, const float* q)
{
    const bool own = A->target_rows != nullptr;
    for (int64_t i = 0; i < A->n; ++i) {
        FpvQuat a; a.w = q[4 * i]; a.x = q[4 * i + 1]; a.y = q[4 * i + 2]; a.z = q[4 * i + 3];
        const FpvDetectPose P = fpv_detect_pose(A->K, p[3 * i], p[3 * i + 1], p[3 * i + 2], a);
        for (int s = 0; s < A->count; ++s) {
            float mn[3], mx[3];
            if (own && s == A->table_count) {
                const float tr = A->target_radius ? A->target_radius[i] : A->K.tr;
                fpv_detect_own_box(A->target_rows[i], A->target_rows[A->target_ld + i], A->target_rows[2 * A->target_ld + i], tr, mn, mx);
            } else {
                const float* const b = A->box[s];
                mn[0] = b[0]; mn[1] = b[1]; mn[2] = b[2]; mx[0] = b[3]; mx[1] = b[4]; mx[2] = b[5];
            }
            FpvDetectOut o;
            fpv_detect_lane(A->K, P, mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], o);
            float* const row = A->boxes + (int64_t)s * 4 * A->out_ld + i;
            row[0] = o.x0; row[A->out_ld] = o.y0; row[2 * A->out_ld] = o.x1; row[3 * A->out_ld] = o.y1;
            A->depth[(int64_t)s * A->out_ld + i] = o.depth;
            A->visible[(int64_t)s * A->out_ld + i] = (uint8_t)(o.visible ? 1 : 0);
        }
    }
}
