// fpv_depth.h - the depth camera (include/fpv_abi.h "Depth camera"): the ONE definition of what a pixel of a drone's
// depth image reports.  fpv_depth_pixel below is what every lane of the gfx950 kernel of fpv_depth.hip runs for its pixel and what
// fpv_depth_eval (fpv_hip.hip, host) runs: the same operations in the same order on the same fp32 values - explicit fmaf,
// fpv_sqrt_flushed, plain '/', compare-and-select instead of fmaxf / fminf, no libm call, -ffp-contract=off - so the host
// reproduces the kernel's images bit for bit.  Everything about the solids is fpv_range.h's own: the ray, the per-object body
// (fpv_range_solid), the hit rule (fpv_range_nearer) and the near test of the cull (fpv_range_near) - called here, defined there.
//
// Camera.  The reference's Camera(camera_pitch_angle, position_relative_to_frame, [W, H], fov): f = W / (2 tan(fov / 2)),
// cx = W / 2, cy = H / 2, rel_rot = WORLD2CAM^T Rx(pitch) = [[0, s, c], [1, 0, 0], [0, -c, s]] (s, c = sin, cos of the pitch: the
// reference hands the pitch to its Euler function as the ROLL, a rotation about x after the axis swap), origin o = p + R(q) rel_pos,
// camera rotation C = R(q) rel_rot.  Pixel (i, j) = column i, row j; its ray goes through the pixel centre:
//     d_b = rel_rot ((i + 1/2 - cx) / f, (j + 1/2 - cy) / f, 1) = a0 + i a_u + j a_v      (fpv_depth_derive: double, narrowed once)
// evaluated per lane as fmaf(j, a_v, fmaf(i, a_u, a0)) per component, and d = R(q) d_b (fpv_range_ray).  d is NOT normalised: its
// camera-frame z is 1, so the ray parameter t IS the reference's depth (the third row of projection_matrix @ point: a z-depth).
//
// Depth.  depth = min(max_depth, nearest hit); nothing hit: max_depth.  Objects are the range sensor's solids with its hit rule
// (t_in <= t_out && t_out >= 0 at max(t_in, 0): 0 from inside).  A gate is a zero-thickness plate in its plane, seen from both
// faces, read from the descriptor row fpv_gates_derive writes: with s = n.(o - c) and nd = n.d the ray meets the plane at
// t = -s / nd; a miss when |nd| < 1e-12 or t < 0.  With x = (o - c) + t d, y = u.x, z = w.x, rho2 = y^2 + (z - zc)^2 it is a hit when
//     |y| <= a + fw && |z| <= hz + fw && rho2 <= (sqrt(r2) + fw)^2         (the aperture grown by the frame width fw; +inf stays +inf)
//     and not (|y| <= a && |z| <= hz && rho2 <= r2)                         (the aperture test of fpv_gate_step, in its form)
// The outer radius is formed once per gate as ro = fpv_sqrt_flushed(r2) + fw, ro2 = ro * ro, a + fw and hz + fw as written.
// A t so large that x overflows makes y or z inf or NaN: every comparison with it is false, the plate is missed, no NaN leaves.
//
// The cull.  Everything about a drone is uniform in a wave (a wave is 64 pixels of ONE drone), so the cull is a function of the
// drone alone: the kernel evaluates it with lane g testing object / gate g and one ballot each, the host with a loop - the same
// masks, and the pixel function takes the masks.  Why a mask cannot change a bit: the rays are not unit here, |d_b| <= dir_len_max
// = sqrt(1 + (W / 2f)^2 + (H / 2f)^2) (the corner of the image plane; the pixel centres lie inside it), and through R of a unit
// quaternion and the narrowing |d| <= dir_len_max (1 + 1e-4).  `reach` = max_depth dir_len_max (1 + 1e-4), rounded up (derive).
// Objects: fpv_range_bounds with `reach` in the place of max_range, measured from the camera origin o: every point of the solid is
// within r_b of its centre, so a ray point on it has t |d| >= |o - c| - r_b > reach (1 + 2e-4) + 1 mm, that is t > max_depth by a
// relative 2e-4 - a thousand times the rounding of the fp32 distance test and of the interval arithmetic.  Gates: every point of
// the plate has |y| <= a + fw and |z| <= hz + fw, so it is within ext = (a + fw) + (hz + fw) of c (the 1-norm bounds the 2-norm); the
// gate is tested when |o - c|^2 < thr^2, thr = (ext + reach) 1.001 + 1 mm in fp32 - the same argument with a relative margin of
// 1e-3 over a rounding of 1e-6.
//
// Encodings.  FPV_DEPTH_METRES: the fp32 depth.  FPV_DEPTH_U8: the reference's image byte (uint8)(255 (1 - depth / max_depth)),
// truncated, in fp32 as  q = depth / max_depth;  v = 255.0f * (1.0f - q);  byte = (uint32_t)v  (0 <= depth <= max_depth: 0 <= v <= 255).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"
#include "fpv_gate.h"
#include "fpv_range.h"

#define FPV_DEPTH_PAR_LEN 1.0e-12f      // |n.d| below this: the ray runs in the gate's plane

// What a render reads besides the drones, the object list and the gate table: uniform, the kernel argument.
struct FpvDepthK {
    float a0[3], au[3], av[3];          // d_b = a0 + i au + j av
    float rel[3];                       // the camera's position in the body frame
    float max_depth, reach, frame_width;
    int32_t width, height, gate_count;
    float near[FPV_MAX_OBJECTS][4];     // fpv_range_bounds' rows for `reach`
};

// the kernel's argument: the state rows read (p: rows 0..2, q: rows 6..9), the gate table, the images written
struct FpvDepthArgs {
    const float* state; int64_t ld; const fpv_gate_v4* gates; void* image; int64_t image_stride; int64_t n;
    uint32_t waves_per_image, pad; FpvDepthK K; FpvObjects T;
};

// the camera origin o = p + R rel
FPV_HD void fpv_depth_origin(const FpvDepthK& K, const FpvRot& R, float px, float py, float pz, float* ox, float* oy, float* oz)
{
    *ox = fmaf(R.r00, K.rel[0], fmaf(R.r01, K.rel[1], fmaf(R.r02, K.rel[2], px)));
    *oy = fmaf(R.r10, K.rel[0], fmaf(R.r11, K.rel[1], fmaf(R.r12, K.rel[2], py)));
    *oz = fmaf(R.r20, K.rel[0], fmaf(R.r21, K.rel[1], fmaf(R.r22, K.rel[2], pz)));
}

// the cull of object k (k < T.count) for a camera at o
FPV_HD bool fpv_depth_object_near(const FpvDepthK& K, const FpvObjects& T, int k, float ox, float oy, float oz)
{
    return fpv_range_near(K.near[k], T.o[k].type, ox, oy, oz);
}

// the cull of the gate whose first and last 16-byte groups are g0 (c.x c.y c.z n.x) and g3 (a hz zc r2)
FPV_HD bool fpv_depth_gate_near(const FpvDepthK& K, const fpv_gate_v4& g0, const fpv_gate_v4& g3, float ox, float oy, float oz)
{
    const float ext = (g3.x + K.frame_width) + (g3.y + K.frame_width);
    const float thr = fmaf(ext + K.reach, 1.001f, 1.0e-3f);
    const float ux = ox - g0.x, uy = oy - g0.y, uz = oz - g0.z;
    return fmaf(ux, ux, fmaf(uy, uy, uz * uz)) < thr * thr;
}

FPV_HD uint32_t fpv_depth_ctz64(uint64_t m)
{
    return (uint32_t)__builtin_ctzll(m);
}

// One pixel (i, j) of one drone: R = fpv_rot(q), o = fpv_depth_origin, obj_mask / gate_mask the drone's cull.  P: a pointer to
// the gate table's first 16-byte group - host or global memory.
template <class P>
FPV_HD float fpv_depth_pixel(const FpvDepthK& K, const FpvObjects& T, P gates, const FpvRot& R, float ox, float oy, float oz,
                             uint32_t obj_mask, uint64_t gate_mask, uint32_t i, uint32_t j)
{
    const float fi = (float)i, fj = (float)j;
    const float bx = fmaf(fj, K.av[0], fmaf(fi, K.au[0], K.a0[0]));
    const float by = fmaf(fj, K.av[1], fmaf(fi, K.au[1], K.a0[1]));
    const float bz = fmaf(fj, K.av[2], fmaf(fi, K.au[2], K.a0[2]));
    const FpvRay y = fpv_range_ray(R, bx, by, bz);
    float best = K.max_depth;
    // ---- the objects: uniform trip count, only predicates differ between lanes
    for (int k = 0; k < T.count; ++k) {
        if (!((obj_mask >> k) & 1u)) continue;
        best = fpv_range_nearer(fpv_range_solid(y, ox, oy, oz, T.o[k]), true, best);
    }
    // ---- the gates the drone is near: the set bits of a uniform mask
    for (uint64_t m = gate_mask; m != 0ull; m &= m - 1ull) {
        const P d = gates + (size_t)fpv_depth_ctz64(m) * FPV_GATE_GROUPS;
        const fpv_gate_v4 g0 = d[0], g1 = d[1], g2 = d[2], g3 = d[3];
        const float cx = ox - g0.x, cy = oy - g0.y, cz = oz - g0.z;
        const float nd = fmaf(g0.w, y.dx, fmaf(g1.x, y.dy, g1.y * y.dz));
        const float s = fmaf(g0.w, cx, fmaf(g1.x, cy, g1.y * cz));
        const bool par = fabsf(nd) < FPV_DEPTH_PAR_LEN;
        const float t = -s / (par ? 1.0f : nd);
        const float xx = fmaf(t, y.dx, cx), xy = fmaf(t, y.dy, cy), xz = fmaf(t, y.dz, cz);
        const float py = fmaf(g1.z, xx, fmaf(g1.w, xy, g2.x * xz));
        const float pz = fmaf(g2.y, xx, fmaf(g2.z, xy, g2.w * xz));
        const float zz = pz - g3.z;
        const float rho2 = fmaf(py, py, zz * zz);
        const float ro = fpv_sqrt_flushed(g3.w) + K.frame_width;
        const bool outer = fabsf(py) <= g3.x + K.frame_width && fabsf(pz) <= g3.y + K.frame_width && rho2 <= ro * ro;
        const bool inner = fabsf(py) <= g3.x && fabsf(pz) <= g3.y && rho2 <= g3.w;
        const bool hit = !par && t >= 0.0f && outer && !inner;
        best = (hit && t < best) ? t : best;
    }
    return best;
}

// FPV_DEPTH_U8: the image byte of a depth, 0..255
FPV_HD uint32_t fpv_depth_u8(float depth, float max_depth)
{
    const float q = depth / max_depth;
    const float v = 255.0f * (1.0f - q);
    return (uint32_t)v;
}

// Host: the direction vectors, the offset, dir_len_max and the reference's own camera numbers from a camera, double arithmetic
// narrowed once.  FPV_OK, or FPV_EPARAM with *why set.
static inline int fpv_depth_derive(const fpv_camera_t& c, fpv_depth_render_t* s, const char** why)
{
    if (c.width < 4 || c.width > FPV_DEPTH_MAX_SIDE || c.height < 4 || c.height > FPV_DEPTH_MAX_SIDE) { *why = "width and height must be 4..128 pixels"; return FPV_EPARAM; }
    if (c.width % 4) { *why = "width must be a multiple of 4"; return FPV_EPARAM; }
    if (!isfinite(c.fov_deg) || !(c.fov_deg > 0.0) || !(c.fov_deg < 180.0)) { *why = "fov must be in (0, 180) degrees"; return FPV_EPARAM; }
    if (!isfinite(c.pitch_deg)) { *why = "pitch is not finite"; return FPV_EPARAM; }
    for (int k = 0; k < 3; ++k)
        if (!isfinite(c.relative_position[k])) { *why = "relative position is not finite"; return FPV_EPARAM; }
    const double rad = 0.017453292519943295;
    const double f = (double)c.width / (2.0 * tan(c.fov_deg * rad / 2.0));
    const double sn = sin(c.pitch_deg * rad), cs = cos(c.pitch_deg * rad);
    const double rr[9] = {0.0, sn, cs, 1.0, 0.0, 0.0, 0.0, -cs, sn};
    const double x0 = (0.5 - 0.5 * c.width) / f, y0 = (0.5 - 0.5 * c.height) / f;
    for (int k = 0; k < 3; ++k) {
        s->dir0[k] = (float)(rr[3 * k] * x0 + rr[3 * k + 1] * y0 + rr[3 * k + 2]);
        s->dir_u[k] = (float)(rr[3 * k] / f);
        s->dir_v[k] = (float)(rr[3 * k + 1] / f);
        s->offset[k] = (float)c.relative_position[k];
    }
    for (int k = 0; k < 9; ++k) s->relative_rotation[k] = rr[k];
    s->focal_length = f;
    const double hw = 0.5 * c.width / f, hh = 0.5 * c.height / f;
    s->dir_len_max = nextafterf((float)sqrt(1.0 + hw * hw + hh * hh), INFINITY);
    s->width = c.width; s->height = c.height;
    return FPV_OK;
}

// Host: `reach` of a render (see "The cull" above), double arithmetic rounded up
static inline float fpv_depth_reach(float max_depth, float dir_len_max)
{
    return nextafterf((float)((double)max_depth * (double)dir_len_max * (1.0 + 1.0e-4)), INFINITY);
}
