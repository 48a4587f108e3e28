// fpv_splat.hip - the gfx950 kernel of the point-cloud camera (include/fpv_abi.h "Point-cloud camera"), and the host
// loop over the same point and pixel functions.
//
// A call reads a drone's position and attitude and writes the reference's splatted image of the world's point clouds
// (Camera.render_depth_image / render_image): prune the objects whose projected box misses the image, project every point of the
// others, truncate, keep the nearest depth per pixel, encode.  Like the other sensors it reads p and q only and is a kernel of its
// own behind an entry point of its own (fpv_splat_render): the step kernels, the state, the step counter and the rotation of the
// traversal stay as they are.
//
// One WORKGROUP = one drone (blockIdx.x), 256 threads: this is a scatter, not a lane per drone or per pixel.  The z-buffer is W * H
// words of dynamic LDS - at the largest image, 128 x 128, all 64 KiB a launch may ask for without further ado, which is why the keep
// flags do not live there too: every wave prunes for itself, lane l the objects l and l + 64, and holds the result as two ballot
// words in scalar registers, so the loop over the objects is wave-uniform by construction and the prune needs no barrier.
//   1. the seven pose loads (uniform in blockIdx), the camera's pose once per thread; the z-buffer is filled with the bits of +inf;
//   2. prune (fpv_splat_keep: the rule of the object detections); barrier (the fill);
//   3. for each kept object the threads stride over its points - three coalesced SoA loads each -, fpv_splat_point, an LDS atomic
//      unsigned min of the bits of the depth; barrier;
//   4. the threads stride over the pixels: four bytes per dword store (u8, mask) or a float (metres);
//   5. with a centroid: per-thread integer sums of the lit pixels' columns and rows and their count, a wave reduction, LDS integer
//      atomics into three words of the z-buffer that has been read by then (two more barriers), one thread divides and stores.
// A workgroup at or past n does not exist; nothing is written past a drone's H * W pixels nor past n in centroid / lit.
//
// A translation unit of its own, linked with the other units into the one libfpv_hip.so; fpv_hip.hip alone still builds (it reaches
// the two functions at the end of this file through weak declarations and answers "not in this build" without them).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_math.h"
#include "fpv_kernels.h"
#include "fpv_splat.h"

namespace {

__device__ __forceinline__ int32_t wave_sum(int32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(FPV_SPLAT_BLOCK) void fpv_splat_kernel(const FpvSplatArgs A)
{
    extern __shared__ uint32_t zbuf[];
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const int32_t npix = A.width * A.height;
    // ---- 1. the pose loads (uniform), then the fill
    const float px = row_at(ROW(A.state, FPV_PX, A.ld), i), py = row_at(ROW(A.state, FPV_PY, A.ld), i), pz = row_at(ROW(A.state, FPV_PZ, A.ld), i);
    FpvQuat q;
    q.w = row_at(ROW(A.state, FPV_QW, A.ld), i); q.x = row_at(ROW(A.state, FPV_QX, A.ld), i);
    q.y = row_at(ROW(A.state, FPV_QY, A.ld), i); q.z = row_at(ROW(A.state, FPV_QZ, A.ld), i);
    for (int32_t k = (int32_t)t; k < npix; k += FPV_SPLAT_BLOCK) zbuf[k] = FPV_SPLAT_EMPTY;
    const FpvDetectPose P = fpv_detect_pose(A.K, px, py, pz, q);
    // ---- 2. prune: every wave for itself, two ballot words
    const int32_t l = (int32_t)(t & 63u);
    bool k0 = false, k1 = false;
    if (l < A.count) k0 = fpv_splat_keep(A.K, P, A.box[l], A.offset[l]);
    if (l + 64 < A.count) k1 = fpv_splat_keep(A.K, P, A.box[l + 64], A.offset[l + 64]);
    const uint64_t keep0 = __ballot(k0), keep1 = __ballot(k1);
    __syncthreads();
    // ---- 3. splat
    for (int32_t m = 0; m < A.count; ++m) {
        if ((((m < 64 ? keep0 : keep1) >> (m & 63)) & 1ull) == 0ull) continue;
        const float ox = A.offset[m][0], oy = A.offset[m][1], oz = A.offset[m][2];
        const int32_t end = A.first[m + 1];
        for (int32_t j = A.first[m] + (int32_t)t; j < end; j += FPV_SPLAT_BLOCK) {
            float depth;
            const int32_t pix = fpv_splat_point(A.K, P, A.width, A.points[j], A.points[A.point_ld + j], A.points[2 * A.point_ld + j], ox, oy, oz, &depth);
            if (pix >= 0) atomicMin(&zbuf[pix], fpv_f32_bits(depth));
        }
    }
    __syncthreads();
    // ---- 4. encode (W is a multiple of 4: so is npix) and 5. the lit pixels of this thread
    int32_t sx = 0, sy = 0, cnt = 0;
    const bool cen = A.centroid != nullptr;
    for (int32_t k = 4 * (int32_t)t; k < npix; k += 4 * FPV_SPLAT_BLOCK) {
        const uint32_t w0 = zbuf[k], w1 = zbuf[k + 1], w2 = zbuf[k + 2], w3 = zbuf[k + 3];
        if (A.encoding == FPV_SPLAT_METRES) {
            float* const out = reinterpret_cast<float*>(A.image) + (int64_t)i * A.image_ld + k;
            out[0] = fpv_splat_depth(w0, A.max_depth); out[1] = fpv_splat_depth(w1, A.max_depth);
            out[2] = fpv_splat_depth(w2, A.max_depth); out[3] = fpv_splat_depth(w3, A.max_depth);
        } else {
            uint32_t* const out = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.image) + (int64_t)i * A.image_ld + k);
            *out = fpv_splat_byte(w0, A.max_depth, A.encoding) | (fpv_splat_byte(w1, A.max_depth, A.encoding) << 8) |
                   (fpv_splat_byte(w2, A.max_depth, A.encoding) << 16) | (fpv_splat_byte(w3, A.max_depth, A.encoding) << 24);
        }
        if (cen) {
            const int32_t y = k / A.width, x = k - y * A.width;             // the four pixels share a row
            const int32_t b0 = fpv_splat_lit(w0, A.max_depth), b1 = fpv_splat_lit(w1, A.max_depth);
            const int32_t b2 = fpv_splat_lit(w2, A.max_depth), b3 = fpv_splat_lit(w3, A.max_depth);
            const int32_t c = b0 + b1 + b2 + b3;
            cnt += c; sy += c * y; sx += c * x + b1 + 2 * b2 + 3 * b3;
        }
    }
    if (!cen) return;                                                        // (uniform)
    __syncthreads();                                                         // every word of the z-buffer has been read
    if (t < 3u) zbuf[t] = 0u;
    __syncthreads();
    sx = wave_sum(sx); sy = wave_sum(sy); cnt = wave_sum(cnt);
    if (l == 0) {
        atomicAdd(&zbuf[0], (uint32_t)sx); atomicAdd(&zbuf[1], (uint32_t)sy); atomicAdd(&zbuf[2], (uint32_t)cnt);
    }
    __syncthreads();
    if (t == 0u) {
        float cx, cy;
        fpv_splat_centroid((int32_t)zbuf[0], (int32_t)zbuf[1], (int32_t)zbuf[2], &cx, &cy);
        A.centroid[2 * (int64_t)i] = cx; A.centroid[2 * (int64_t)i + 1] = cy;
        A.lit[i] = (int32_t)zbuf[2];
    }
}

}  // namespace

// what fpv_hip.hip launches (it declares both weak): the kernel ...
extern "C" __attribute__((visibility("hidden"))) void* fpv_splat_kernel_fn(void)
{
    return reinterpret_cast<void*>(fpv_splat_kernel);
}

// ... and the same functions over n drones on the host: every pointer of A is host memory, state is not read (p, q are AoS)
extern "C" __attribute__((visibility("hidden"))) void fpv_splat_eval_host(const FpvSplatArgs* A, const float* p, const float* q)
{
    const int32_t npix = A->width * A->height;
    std::vector<uint32_t> zbuf((size_t)npix);
    for (int64_t i = 0; i < A->n; ++i) {
        FpvQuat a; a.w = q[4 * i]; a.x = q[4 * i + 1]; a.y = q[4 * i + 2]; a.z = q[4 * i + 3];
        const FpvDetectPose P = fpv_detect_pose(A->K, p[3 * i], p[3 * i + 1], p[3 * i + 2], a);
        for (int32_t k = 0; k < npix; ++k) zbuf[(size_t)k] = FPV_SPLAT_EMPTY;
        for (int32_t m = 0; m < A->count; ++m) {
            if (!fpv_splat_keep(A->K, P, A->box[m], A->offset[m])) continue;
            for (int32_t j = A->first[m]; j < A->first[m + 1]; ++j) {
                float depth;
                const int32_t pix = fpv_splat_point(A->K, P, A->width, A->points[j], A->points[A->point_ld + j], A->points[2 * A->point_ld + j],
                                                    A->offset[m][0], A->offset[m][1], A->offset[m][2], &depth);
                if (pix >= 0) {
                    const uint32_t w = fpv_f32_bits(depth);
                    zbuf[(size_t)pix] = w < zbuf[(size_t)pix] ? w : zbuf[(size_t)pix];
                }
            }
        }
        int32_t sx = 0, sy = 0, cnt = 0;
        for (int32_t k = 0; k < npix; ++k) {
            const uint32_t w = zbuf[(size_t)k];
            if (A->encoding == FPV_SPLAT_METRES) reinterpret_cast<float*>(A->image)[i * A->image_ld + k] = fpv_splat_depth(w, A->max_depth);
            else reinterpret_cast<uint8_t*>(A->image)[i * A->image_ld + k] = (uint8_t)fpv_splat_byte(w, A->max_depth, A->encoding);
            if (A->centroid && fpv_splat_lit(w, A->max_depth)) { sx += k % A->width; sy += k / A->width; cnt += 1; }
        }
        if (A->centroid) {
            fpv_splat_centroid(sx, sy, cnt, &A->centroid[2 * i], &A->centroid[2 * i + 1]);
            A->lit[i] = cnt;
        }
    }
}
