// fpv_depth.hip - the gfx950 kernel of the depth camera (include/fpv_abi.h "Depth camera").
//
// A render reads a drone's position and attitude and writes one depth image of the collision world and the gates as the drone's
// camera sees them (fpv_depth.h fpv_depth_pixel, the function the host's fpv_depth_eval runs).  Like the range scan it reads only
// p and q: a kernel of its own behind an entry point of its own (fpv_depth_render) that composes with every fp32 handle.
//
// One lane = one pixel.  A wave is 64 consecutive pixels of the flattened image of ONE drone (the last wave of an image may be
// ragged); 256-thread blocks in the plain order, and a block may span drones when the image is small.  The wave's global index
// (blockIdx.x * 4 + the wave in the block, made provably uniform with readfirstlane) gives (drone, wave in image): the drone index
// travels in blockIdx.x arithmetic because gridDim.y stops at 65535.  Everything per drone - the seven state values, R(q), the
// origin, every object and gate constant - is uniform in the wave: the state values are loaded once per wave and broadcast from the
// first lane, the rest are scalar loads of the kernel argument and of the gate table.  The cull costs no uniform instruction stream
// per gate: lane g tests object g (then gate g) against the camera origin and one ballot each gives the mask of near ones; the
// pixel function runs over the set bits.  What is left per lane is the direction, the ray set-up with its three true divisions and
// the predicates.
//
// Output [n][image_stride], row-major [H][W] inside, write-only with the streaming hint: lanes of a wave write consecutive
// elements.  FPV_DEPTH_U8 issues no byte store (the project's rule for 2-byte accesses too): the four lanes of a quad combine their
// bytes through two DPP quad permutes and one lane in four stores a dword; W % 4 == 0 keeps a quad inside a row and wholly live.
// All lanes of a live wave run to the end (a lane past the image computes its wave's last pixel and stores nothing), so the quad
// permutes never read a disabled lane.
//
// A translation unit of its own, linked with fpv_hip.hip, fpv_phys.hip, fpv_gate.hip and fpv_range.hip into the one libfpv_hip.so:
// their kernels stay exactly as they are, and fpv_hip.hip alone still builds (it reaches the lookup function at the end of this
// file through a weak declaration and answers "not in this build" without it).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_math.h"
#include "fpv_kernels.h"
#include "fpv_depth.h"

namespace {

constexpr int kDepthBlock = 256;

__device__ __forceinline__ float uniform_of(float x)
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(x)));
}

// quad_perm [1, 0, 3, 2] and [2, 3, 0, 1]: after the two steps every lane of a quad holds the OR of the four
__device__ __forceinline__ uint32_t quad_or(uint32_t x)
{
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false);
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false);
    return x;
}

template <bool U8>
__global__ __launch_bounds__(kDepthBlock) void fpv_depth_render_kernel(const FpvDepthArgs A)
{
    // ---- 1. which drone, which 64 pixels: uniform
    const uint32_t wave = blockIdx.x * (uint32_t)(kDepthBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t drone = wave / A.waves_per_image;
    if (drone >= (uint32_t)A.n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pixels = (uint32_t)(A.K.width * A.K.height);
    const uint32_t pix = (wave - drone * A.waves_per_image) * 64u + lane;
    const bool live = pix < pixels;
    const uint32_t at = live ? pix : pixels - 1u;
    const uint32_t j = at / (uint32_t)A.K.width, i = at - j * (uint32_t)A.K.width;
    // ---- 2. the drone's seven state values, once per wave
    const float px = uniform_of(row_at(ROW(A.state, FPV_PX, A.ld), drone)), py = uniform_of(row_at(ROW(A.state, FPV_PY, A.ld), drone));
    const float pz = uniform_of(row_at(ROW(A.state, FPV_PZ, A.ld), drone));
    FpvQuat q;
    q.w = uniform_of(row_at(ROW(A.state, FPV_QW, A.ld), drone)); q.x = uniform_of(row_at(ROW(A.state, FPV_QX, A.ld), drone));
    q.y = uniform_of(row_at(ROW(A.state, FPV_QY, A.ld), drone)); q.z = uniform_of(row_at(ROW(A.state, FPV_QZ, A.ld), drone));
    const FpvRot R = fpv_rot(q);
    float ox, oy, oz;
    fpv_depth_origin(A.K, R, px, py, pz, &ox, &oy, &oz);
    // ---- 3. the cull: lane g asks about object g, then about gate g; one ballot each
    const bool obj_near = (int)lane < A.T.count && fpv_depth_object_near(A.K, A.T, (int)(lane & (FPV_MAX_OBJECTS - 1)), ox, oy, oz);
    const uint32_t obj_mask = (uint32_t)__builtin_amdgcn_ballot_w64(obj_near);
    uint64_t gate_mask = 0ull;
    if (A.K.gate_count > 0) {
        bool gate_near = false;
        if ((int)lane < A.K.gate_count) {
            const fpv_gate_v4* d = A.gates + (size_t)lane * FPV_GATE_GROUPS;
            gate_near = fpv_depth_gate_near(A.K, d[0], d[3], ox, oy, oz);
        }
        gate_mask = __builtin_amdgcn_ballot_w64(gate_near);
    }
    // ---- 4. the pixel
    const float depth = fpv_depth_pixel(A.K, A.T, A.gates, R, ox, oy, oz, obj_mask, gate_mask, i, j);
    // ---- 5. consecutive elements of the drone's image
    const int64_t base = (int64_t)drone * A.image_stride;
    if (U8) {
        const uint32_t word = quad_or(fpv_depth_u8(depth, A.K.max_depth) << (8u * (lane & 3u)));
        uint32_t* const out = reinterpret_cast<uint32_t*>(A.image) + (base >> 2);
        if (live && (lane & 3u) == 0u) ST_OUT(row_at(out, pix >> 2), word);
    } else {
        float* const out = reinterpret_cast<float*>(A.image) + base;
        if (live) ST_OUT(row_at(out, pix), depth);
    }
}

}  // namespace

// what fpv_hip.hip launches (it declares this weak): the kernel of an encoding
extern "C" __attribute__((visibility("hidden"))) void* fpv_depth_render_kernel_fn(int u8)
{
    return u8 ? reinterpret_cast<void*>(fpv_depth_render_kernel<true>) : reinterpret_cast<void*>(fpv_depth_render_kernel<false>);
}
