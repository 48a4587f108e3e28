// fpv_splat.h - the point-cloud camera (include/fpv_abi.h "Point-cloud camera"): the ONE definition of where a point of
// a cloud lands in a drone's image and of what a pixel of the z-buffer becomes - the reference's Camera.project, render_depth_image
// and render_image (src/utils/components.py:558-568, 602-629).  fpv_splat_keep, fpv_splat_point, fpv_splat_pixel and
// fpv_splat_lit below are what the gfx950 kernel of fpv_splat.hip and fpv_splat_eval (host) run: the same operations in the same
// order on the same fp32 values - explicit fmaf, plain '/', truncf, compare-and-select, -ffp-contract=off - so the host reproduces
// the kernel's outputs bit for bit.
//
// 1. Camera pose: fpv_detect_pose (fpv_detect.h), pcam = p + R(q) rel_pos, Rcam = R(q) rel_rot.
// 2. Prune (pruned_objects_list, :585-600): object m is kept when fpv_detect_lane, pixel mode "int", calls its box - box[m] shifted
//    by offset[m] - visible.  One definition with the object detections.
// 3. Point: X = point + offset, c = Rcam^T (X - pcam); in front when c.z > 0 (:564); u = trunc((f c.x) / c.z + W/2), v likewise
//    (:566-567: astype(int) truncates toward zero, so a coordinate in (-1, 0) lands in column or row 0 - kept); accepted when
//    0 <= u < W and 0 <= v < H (:621-622), compared in float - no cast of a value out of an integer's range; the pixel is v W + u.
// 4. z-buffer: a word per pixel, +inf at first, the unsigned minimum of the bits of c.z (positive floats order like their bits: the
//    result does not depend on the order of arrival).  A NaN is not > 0 and never arrives; +inf arrives and changes nothing.
// 5. Pixel: no point (the word is still +inf) -> max_depth (:627).  u8: z = min(z, max_depth) (:626), the byte of fpv_depth_u8 (:628).
//    metres: the float, not clipped.  mask: 1 where a point landed (:602-612).
// 6. Lit (simulator.py:103): the pixel's u8 byte at this max_depth is > 0.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"
#include "fpv_depth.h"
#include "fpv_detect.h"

#define FPV_SPLAT_BLOCK 256             // threads of the one workgroup of a drone
#define FPV_SPLAT_EMPTY 0x7f800000u     // the bits of +inf: a pixel no point landed in

// the kernel's argument: the state rows read (p, q), the cloud, the outputs, the object tables by value
struct FpvSplatArgs {
    const float* state; int64_t ld; const float* points; int64_t point_ld;
    void* image; int64_t image_ld; float* centroid; int32_t* lit; int64_t n;
    FpvDetectK K;                       // the camera; trunc = 1, clip = 0: the pruning rule reads it
    float max_depth; int32_t encoding, width, height, count;
    int32_t first[FPV_MAX_BOXES + 1];
    float offset[FPV_MAX_BOXES][3];
    float box[FPV_MAX_BOXES][6];
};

// whether the reference's pruning keeps an object: its local box (mn, mx) shifted by its offset
FPV_HD bool fpv_splat_keep(const FpvDetectK& K, const FpvDetectPose& P, const float* box, const float* off)
{
    FpvDetectOut o;
    fpv_detect_lane(K, P, box[0] + off[0], box[1] + off[1], box[2] + off[2], box[3] + off[0], box[4] + off[1], box[5] + off[2], o);
    return o.visible;
}

// one point (x, y, z) of an object at offset (ox, oy, oz): the pixel index v W + u it lands in with *depth its c.z, or -1
FPV_HD int32_t fpv_splat_point(const FpvDetectK& K, const FpvDetectPose& P, int32_t width, float x, float y, float z, float ox, float oy,
                               float oz, float* depth)
{
    const float ex = (x + ox) - P.ox, ey = (y + oy) - P.oy, ez = (z + oz) - P.oz;
    const float ccx = fmaf(P.c[0], ex, fmaf(P.c[3], ey, P.c[6] * ez));          // Rcam^T (X - pcam)
    const float ccy = fmaf(P.c[1], ex, fmaf(P.c[4], ey, P.c[7] * ez));
    const float ccz = fmaf(P.c[2], ex, fmaf(P.c[5], ey, P.c[8] * ez));
    const float u = truncf((K.f * ccx) / ccz + K.cx);
    const float v = truncf((K.f * ccy) / ccz + K.cy);
    *depth = ccz;
    if (!(ccz > 0.0f && u >= 0.0f && u < K.w && v >= 0.0f && v < K.h)) return -1;
    return (int32_t)v * width + (int32_t)u;
}

// the depth a z-buffer word stands for
FPV_HD float fpv_splat_depth(uint32_t word, float max_depth) { return word == FPV_SPLAT_EMPTY ? max_depth : fpv_bits_f32(word); }

// the u8 byte of a z-buffer word
FPV_HD uint32_t fpv_splat_u8(uint32_t word, float max_depth)
{
    const float z = fpv_splat_depth(word, max_depth);
    return fpv_depth_u8(z < max_depth ? z : max_depth, max_depth);
}

// the byte of an encoding that writes bytes (u8, mask)
FPV_HD uint32_t fpv_splat_byte(uint32_t word, float max_depth, int32_t encoding)
{
    return encoding == FPV_SPLAT_MASK ? (word != FPV_SPLAT_EMPTY ? 1u : 0u) : fpv_splat_u8(word, max_depth);
}

FPV_HD bool fpv_splat_lit(uint32_t word, float max_depth) { return fpv_splat_u8(word, max_depth) > 0u; }

// the centroid of `count` lit pixels whose columns sum to sx and rows to sy: exact integers, one division each
FPV_HD void fpv_splat_centroid(int32_t sx, int32_t sy, int32_t count, float* cx, float* cy)
{
    const float qnan = fpv_bits_f32(0x7fc00000u);
    *cx = count > 0 ? (float)sx / (float)count : qnan;
    *cy = count > 0 ? (float)sy / (float)count : qnan;
}

// Host: the three deterministic clouds of the reference in double (numpy's linspace: start + k step, the last value the stop itself),
// narrowed once.  Returns the number of points; out may be null (a query).
static inline double fpv_cloud_linspace(double a, double b, int n, int k)
{
    if (n == 1) return a;
    return k == n - 1 ? b : a + (double)k * ((b - a) / (double)(n - 1));
}

static inline int64_t fpv_cloud_points(int kind, const double* v, const int32_t* r, float* out, int64_t ld)
{
    const double pi = 3.141592653589793;
    if (kind == FPV_CLOUD_GROUND) {
        const int n = r[0];
        if (out)
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    const int64_t k = (int64_t)i * n + j;
                    out[k] = (float)fpv_cloud_linspace(-v[0] / 2.0, v[0] / 2.0, n, j);
                    out[ld + k] = (float)fpv_cloud_linspace(-v[0] / 2.0, v[0] / 2.0, n, i);
                    out[2 * ld + k] = 0.0f;
                }
        return (int64_t)n * n;
    }
    if (kind == FPV_CLOUD_CYLINDER) {
        const int na = r[0], nh = r[1];
        if (out)
            for (int i = 0; i < nh; ++i)
                for (int j = 0; j < na; ++j) {
                    const int64_t k = (int64_t)i * na + j;
                    const double th = fpv_cloud_linspace(0.0, 2.0 * pi, na, j);
                    out[k] = (float)(v[0] + v[3] * cos(th));
                    out[ld + k] = (float)(v[1] + v[3] * sin(th));
                    out[2 * ld + k] = (float)(v[2] + fpv_cloud_linspace(0.0, v[4], nh, i));
                }
        return (int64_t)na * nh;
    }
    // a gate: position v[0..2], rotation v[3..11] row-major, size v[12]; r = {shape, resolution}
    const int shape = r[0], pts = shape == FPV_GATE_RECTANGLE ? 4 : r[1];
    const double size = v[12], coef = shape == FPV_GATE_HALF_CIRCLE ? 1.0 : 2.0;
    if (out)
        for (int j = 0; j <= pts; ++j) {
            const int c = j == pts ? 0 : j;                                         // the first corner again (:805)
            double y, z;
            if (shape == FPV_GATE_RECTANGLE) {
                y = ((c == 1 || c == 2) ? 1.0 : -1.0) * size / 2.0;
                z = (c >= 2 ? 1.0 : -1.0) * size / 2.0;
            } else {
                const double th = fpv_cloud_linspace(0.0, coef * pi, pts, c);
                y = cos(th) * size / coef;
                z = sin(th) * size / coef;
                if (shape == FPV_GATE_HALF_CIRCLE) z -= size / 2.0;
            }
            for (int a = 0; a < 3; ++a) out[a * ld + j] = (float)(v[3 + 3 * a + 1] * y + v[3 + 3 * a + 2] * z + v[a]);
        }
    return (int64_t)pts + 1;
}
