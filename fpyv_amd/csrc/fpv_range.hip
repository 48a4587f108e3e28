// fpv_range.hip - the gfx950 kernel of the range sensor (include/fpv_abi.h "Range scan").
//
// A scan reads a drone's position and attitude and writes, for each of up to 32 body-frame rays, the distance to the nearest
// object of the collision world (fpv_range.h fpv_range_lane, the function the host's fpv_range_eval runs).  It reads only p and q,
// so it is a kernel of its own behind an entry point of its own (fpv_range_scan) and composes with every fp32 handle - plain,
// physics table, gate course, stick noise, reset sources, Racer, partitions, shards - instead of adding a row to the matrix of
// step-kernel families.  Unlike the step kernels it is not bound by memory: 28 + 4 R bytes per drone against R x objects x a few
// dozen VALU instructions with square roots and true divisions.
//
// One lane = one drone, 128-thread blocks in the plain order (no rotation: nothing this kernel writes is read back by a later
// launch).  The seven state loads go out before the first use; R(q) is formed once; the ray set, the object list and their cull
// rows are wave-uniform kernel arguments read through scalar loads inside loops with uniform trip counts (ray loop outside,
// object loop inside); an object that no lane of the wave is near is skipped for every ray (fpv_range.h "The wave-level cull":
// the same bits with and without).  The rows are SoA, ranges[r][ranges_ld]: one coalesced dword store per ray, write-only, with
// the streaming hint like accel and gate_obs.
//
// A translation unit of its own, linked with fpv_hip.hip, fpv_phys.hip and fpv_gate.hip into the one libfpv_hip.so: their kernels
// stay exactly as they are, and fpv_hip.hip alone still builds (it reaches the lookup function at the end of this file through a
// weak declaration and answers "not in this build" without it).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_math.h"
#include "fpv_kernels.h"
#include "fpv_range.h"

namespace {

__global__ __launch_bounds__(kStepBlock) void fpv_range_scan_kernel(const FpvRangeArgs A)
{
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    // ---- 1. the seven loads of this lane before the first use
    const float px = row_at(ROW(A.state, FPV_PX, A.ld), i), py = row_at(ROW(A.state, FPV_PY, A.ld), i), pz = row_at(ROW(A.state, FPV_PZ, A.ld), i);
    FpvQuat q;
    q.w = row_at(ROW(A.state, FPV_QW, A.ld), i); q.x = row_at(ROW(A.state, FPV_QX, A.ld), i);
    q.y = row_at(ROW(A.state, FPV_QY, A.ld), i); q.z = row_at(ROW(A.state, FPV_QZ, A.ld), i);
    // ---- 2. every ray against every object the wave is near; one row store per ray
    float* const ranges = A.ranges;
    const int64_t ranges_ld = A.ranges_ld;
    fpv_range_lane(A.K, A.T, q, px, py, pz, [&](int r, float t) { ST_OUT(row_at(ROW(ranges, r, ranges_ld), i), t); });
}

}  // namespace

// what fpv_hip.hip launches (it declares this weak)
extern "C" __attribute__((visibility("hidden"))) void* fpv_range_scan_kernel_fn(void)
{
    return reinterpret_cast<void*>(fpv_range_scan_kernel);
}
