// fpv_detect.h - object detections (include/fpv_abi.h "Object detections"): the ONE definition of the image-plane
// bounding box of an axis-aligned world box in a drone's camera, the reference's Camera.project(attr='bbox3d'), bbox3d_to_bbox2d and
// pruned_objects_list (/root/reference/src/utils/components.py:558-600) over the boxes of helper_functions.bbox3d
// (helper_functions.py:120-136).  fpv_detect_pose and fpv_detect_lane below are what every lane of the gfx950 kernel of
// fpv_detect.hip runs for its drone and what fpv_detect_eval (host) runs: the same operations in the same order on the same fp32
// values - explicit fmaf, plain '/', truncf, compare-and-select instead of fminf / fmaxf, fpv_clamp, -ffp-contract=off - so the host
// reproduces the kernel's outputs bit for bit.
//
// 1. Camera pose (Camera.update, components.py:501-503): pcam = p + R(q) rel_pos, Rcam = R(q) rel_rot.
// 2. Corners in the reference's order (helper_functions.py:126-132): corner k takes x from max when k >= 4, y from max when k is
//    odd, z from max when k is 2, 3, 6 or 7.  c = Rcam^T (X - pcam); its depth is c.z; it is IN FRONT when c.z > 0 (:553); its pixel
//    is ((f c.x) / c.z + W/2, (f c.y) / c.z + H/2).
// 3. Pixel mode "int" (the reference's astype(int)): every pixel coordinate is truncated toward zero with truncf and stays a float -
//    no cast to an integer type (out of range that cast is undefined on the host and saturates on the device).  "float" keeps it.
// 4. Box = componentwise min and max over the in-front corners (:570-575), depth = the smallest in-front depth.
// 5. visible = at least one corner in front && x_max > 0 && y_max > 0 && x_min < W && y_min < H (:589-595).
// 6. No corner in front (the reference's bbox2d raises): box (0, 0, 0, 0), depth 0, visible 0.
// 7. clip: a VISIBLE box is clamped to [0, W] x [0, H]; the reference does not clip.
// A pixel that is NaN (a pose that is not finite; inf - inf in a camera-frame coordinate) loses every comparison: it moves neither
// extreme, and a box no comparison moved keeps +inf / -inf and is not visible.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"

#define FPV_DETECT_GROUP 8              // slots per blockIdx.y of the kernel

// What a call reads besides the drones and the boxes: uniform, part of the kernel argument.
struct FpvDetectK {
    float rr[9];                        // rel_rot, row-major
    float rel[3];                       // rel_pos
    float f, cx, cy, w, h;              // focal length, W/2, H/2, W, H
    float tr;                           // the radius of the own-target slot when no radius row is given
    int32_t trunc, clip;                // pixel mode "int"; clamp visible boxes
};

// the kernel's argument: the state rows read (p, q), the optional per-drone target rows, the three outputs, the box table by value
struct FpvDetectArgs {
    const float* state; int64_t ld; const float* target_rows; int64_t target_ld; const float* target_radius;
    float* boxes; float* depth; uint8_t* visible; int64_t out_ld; int64_t n; int32_t count, table_count; FpvDetectK K;
    float box[FPV_MAX_BOXES][6];
};

struct FpvDetectPose { float c[9]; float ox, oy, oz; };      // Rcam row-major, pcam
struct FpvDetectOut { float x0, y0, x1, y1, depth; bool visible; };

FPV_HD FpvDetectPose fpv_detect_pose(const FpvDetectK& K, float px, float py, float pz, FpvQuat q)
{
    const FpvRot R = fpv_rot(q);
    FpvDetectPose P;
    P.ox = fmaf(R.r00, K.rel[0], fmaf(R.r01, K.rel[1], fmaf(R.r02, K.rel[2], px)));
    P.oy = fmaf(R.r10, K.rel[0], fmaf(R.r11, K.rel[1], fmaf(R.r12, K.rel[2], py)));
    P.oz = fmaf(R.r20, K.rel[0], fmaf(R.r21, K.rel[1], fmaf(R.r22, K.rel[2], pz)));
    const float r[9] = {R.r00, R.r01, R.r02, R.r10, R.r11, R.r12, R.r20, R.r21, R.r22};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            P.c[3 * a + b] = fmaf(r[3 * a], K.rr[b], fmaf(r[3 * a + 1], K.rr[3 + b], r[3 * a + 2] * K.rr[6 + b]));
    return P;
}

// One drone (its camera pose P) against one box (mn, mx)
FPV_HD void fpv_detect_lane(const FpvDetectK& K, const FpvDetectPose& P, float mnx, float mny, float mnz, float mxx, float mxy, float mxz,
                            FpvDetectOut& o)
{
    const float inf = fpv_bits_f32(0x7f800000u), ninf = fpv_bits_f32(0xff800000u);
    float x0 = inf, y0 = inf, x1 = ninf, y1 = ninf, dmin = inf;
    bool any = false;
    const bool trunc = K.trunc != 0;
    // the differences X - pcam of the two values of every axis
    const float dx[2] = {mnx - P.ox, mxx - P.ox}, dy[2] = {mny - P.oy, mxy - P.oy}, dz[2] = {mnz - P.oz, mxz - P.oz};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 8; ++k) {
        const float ex = dx[k >> 2], ey = dy[k & 1], ez = dz[(k >> 1) & 1];
        const float ccx = fmaf(P.c[0], ex, fmaf(P.c[3], ey, P.c[6] * ez));          // Rcam^T (X - pcam)
        const float ccy = fmaf(P.c[1], ex, fmaf(P.c[4], ey, P.c[7] * ez));
        const float ccz = fmaf(P.c[2], ex, fmaf(P.c[5], ey, P.c[8] * ez));
        float u = (K.f * ccx) / ccz + K.cx;
        float v = (K.f * ccy) / ccz + K.cy;
        if (trunc) { u = truncf(u); v = truncf(v); }
        const bool front = ccz > 0.0f;
        any = any || front;
        x0 = (front && u < x0) ? u : x0; x1 = (front && u > x1) ? u : x1;
        y0 = (front && v < y0) ? v : y0; y1 = (front && v > y1) ? v : y1;
        dmin = (front && ccz < dmin) ? ccz : dmin;
    }
    const bool vis = any && x1 > 0.0f && y1 > 0.0f && x0 < K.w && y0 < K.h;
    if (K.clip != 0 && vis) {
        x0 = fpv_clamp(x0, 0.0f, K.w); x1 = fpv_clamp(x1, 0.0f, K.w);
        y0 = fpv_clamp(y0, 0.0f, K.h); y1 = fpv_clamp(y1, 0.0f, K.h);
    }
    o.x0 = any ? x0 : 0.0f; o.y0 = any ? y0 : 0.0f; o.x1 = any ? x1 : 0.0f; o.y1 = any ? y1 : 0.0f;
    o.depth = any ? dmin : 0.0f;
    o.visible = vis;
}

// The lane's own box: centre +- radius of its pursuit target, in fp32
FPV_HD void fpv_detect_own_box(float tx, float ty, float tz, float r, float* mn, float* mx)
{
    mn[0] = tx - r; mn[1] = ty - r; mn[2] = tz - r;
    mx[0] = tx + r; mx[1] = ty + r; mx[2] = tz + r;
}

// Host: the box table of an object list and a course (double arithmetic, narrowed once).  FPV_OK, or FPV_EPARAM with *why and *bad
// (the slot) set.
static inline int fpv_detect_derive_boxes(const fpv_objects_t* objs, const double* ground_size, const fpv_gate_t* gates, int gate_count,
                                          int gate_resolution, fpv_boxes_t* out, int* bad, const char** why)
{
    int m = 0;
    const int no = objs ? objs->count : 0;
    for (int k = 0; k < no; ++k, ++m) {
        const fpv_object_t& o = objs->obj[k];
        double mn[3], mx[3];
        *bad = m;
        if (o.type == FPV_OBJ_GROUND) {
            if (!ground_size) { *why = "a Ground needs its size (ground_size is null)"; return FPV_EPARAM; }
            const double s = ground_size[k];
            if (!isfinite(s) || !(s > 0.0)) { *why = "a Ground must be given its size, finite and positive"; return FPV_EPARAM; }
            mn[0] = mn[1] = -s / 2.0; mx[0] = mx[1] = s / 2.0; mn[2] = mx[2] = 0.0;
        } else if (o.type == FPV_OBJ_CYLINDER) {
            mn[0] = (double)o.x - o.radius; mx[0] = (double)o.x + o.radius; mn[1] = (double)o.y - o.radius; mx[1] = (double)o.y + o.radius;
            mn[2] = o.z; mx[2] = (double)o.z + o.height;
        } else if (o.type == FPV_OBJ_SPHERE) {
            const double c[3] = {o.x, o.y, o.z};
            for (int a = 0; a < 3; ++a) { mn[a] = c[a] - o.radius; mx[a] = c[a] + o.radius; }
        } else { *why = "unknown object type"; return FPV_EPARAM; }
        for (int a = 0; a < 3; ++a) {
            if (!isfinite(mn[a]) || !isfinite(mx[a])) { *why = "the box is not finite"; return FPV_EPARAM; }
            if (mn[a] > mx[a]) { *why = "the box has min > max (a negative radius or height)"; return FPV_EPARAM; }
            out->box[m][a] = (float)mn[a]; out->box[m][3 + a] = (float)mx[a];
        }
    }
    const double pi = 3.141592653589793;
    for (int g = 0; g < gate_count; ++g, ++m) {
        const fpv_gate_t& G = gates[g];
        *bad = m;
        if (!isfinite(G.size) || !(G.size > 0.0)) { *why = "the size of a gate must be finite and positive"; return FPV_EPARAM; }
        if (G.shape < FPV_GATE_RECTANGLE || G.shape > FPV_GATE_HALF_CIRCLE) { *why = "unknown gate shape"; return FPV_EPARAM; }
        double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        const int pts = G.shape == FPV_GATE_RECTANGLE ? 4 : gate_resolution;
        const double coef = G.shape == FPV_GATE_HALF_CIRCLE ? 1.0 : 2.0;
        for (int j = 0; j < pts; ++j) {
            double y, z;                                            // the gate's own frame: x = 0 (components.py:790-800)
            if (G.shape == FPV_GATE_RECTANGLE) {
                y = ((j == 1 || j == 2) ? 1.0 : -1.0) * G.size / 2.0;
                z = (j >= 2 ? 1.0 : -1.0) * G.size / 2.0;
            } else {
                const double stop = coef * pi;
                const double th = pts == 1 ? 0.0 : (j == pts - 1 ? stop : (double)j * (stop / (double)(pts - 1)));      // np.linspace
                y = cos(th) * G.size / coef;
                z = sin(th) * G.size / coef;
                if (G.shape == FPV_GATE_HALF_CIRCLE) z -= G.size / 2.0;
            }
            for (int a = 0; a < 3; ++a) {
                const double w = G.rotation[3 * a + 1] * y + G.rotation[3 * a + 2] * z + G.position[a];
                mn[a] = w < mn[a] ? w : mn[a]; mx[a] = w > mx[a] ? w : mx[a];
            }
        }
        for (int a = 0; a < 3; ++a) {
            if (!isfinite(mn[a]) || !isfinite(mx[a])) { *why = "the box is not finite (the gate's position or rotation is not)"; return FPV_EPARAM; }
            out->box[m][a] = (float)mn[a]; out->box[m][3 + a] = (float)mx[a];
        }
    }
    out->count = m;
    return FPV_OK;
}
