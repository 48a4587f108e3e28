// fpv_chase.h - the target chase (include/fpv_abi.h "Target chase"): the ONE definition of the reference's vision
// guidance law for a drone, Drone.calculate_needed_force_orientation(pixel, target, ref_frame, mode)
// (/root/reference/src/utils/components.py:258-304) fed by the pixel of the target (src/core/simulator.py:102-110).  fpv_chase_lane
// below is what every lane of the gfx950 kernel of fpv_chase.hip runs for its drone and what fpv_chase_eval (host) runs: the same
// operations in the same order on the same fp32 values - explicit fmaf, fpv_sqrt_flushed, plain '/', compare-and-select instead of
// fminf, fpv_clamp, no libm call, -ffp-contract=off - so the host reproduces the kernel's outputs bit for bit.
//
// Camera (components.py:449-503, as DESIGN 3.8 derives it): f = W / (2 tan(fov / 2)), centre (W/2, H/2), rel_rot = WORLD2CAM^T
// Rx(pitch), origin o = p + R(q) rel_pos, rotation C = R(q) rel_rot.  No image is written, so W and H are not bound by the depth
// image's 4..128 (fpv_chase_derive_camera has its own checks: the reference's 640 x 480 is accepted).
//
// 1. Pixel (simulator.py:102-107).  The reference takes the centroid of the splatted pixels of the target in its target-only depth
//    image; THE PROJECTED CENTRE OF THE TARGET IS THIS BUILD'S DEFINITION OF THAT CENTROID:
//        p_c = C^T (c - o) = rel_rot^T (R^T (c - o)),   u = (f p_c.x) / p_c.z + W/2,   v = (f p_c.y) / p_c.z + H/2    (fractional)
//    seen iff p_c.z > 0 && p_c.z <= max_depth && 0 <= u < W && 0 <= v < H.  A caller's own pixel (x, y) replaces all of this; it
//    is seen iff neither component is NaN.  A lane that does not see the target is NOT GUIDED: thrust = NaN (the override's "not
//    overridden" value), rotation = identity, pixel_out = NaN, visible = 0, PID rows untouched - the reference calls neither the law
//    nor the PID in that branch (simulator.py:104-105).
// 2. Direction (Camera.pixel2direction, :505-525, world frame): d = C ((u - W/2) / f, (v - H/2) / f, 1) = R (rel_rot (..)), / |.|.
// 3. The law (:267-304).  world: g = (0, 0, -9.81 m) - the literal 9.81 of kinematics.gravity_vector(mass, g=9.81), not the
//    simulator's gravity -, w = v.  drone: g = R g_world, w = R v (:274-276: `R @ v / |v| @ d` is ((R v) / |v|) . d and the drag
//    is along -(R v); d stays the world-frame direction; |v| and v.z are the world velocity's).
//        s = |v|,  k = (w . d) / s,  drag = -(virtual_drag (1 - k) / 2 s) w                                            (:271-272, :285)
//        lift = [p.z < tof] (-(tof - p.z) virtual_lift (1 + |v.z|)) g                                                   (:286)
//        dist = min(|p - c| - r, UWB_sensor_max_range)                                                                 (:287)
//        m = clip(PID(dist, keep_distance), min_output, max_output)     fpv_pid_axis<float, 1> on the lane's four rows  (:288-290)
//        F = m d + drag + lift - g,   thrust_force = |F|                                                              (:292-293)
//        level: y = F x g;  frontarget: y = F x d;  x = y x F;  rotation = columns x / |x|, y / |y|, F / |F|           (:294-303)
// 4. Where the reference yields NaN, this build defines:
//      s = 0 (below 2^-48 m/s): zero virtual drag.
//      y = 0 - |F x b|^2 <= 1e-12 |F|^2 |b|^2 for the second operand b (F parallel to g, or to d in frontarget; the sine of their
//        angle below 1e-6, where an fp32 cross product holds no direction): b is REPLACED by the world x axis (1, 0, 0), and when F
//        is parallel to that too (same test) by the world y axis (0, 1, 0).  The columns are then x, y, F of the same formulas.
//      F = 0 (|F|^2 below 2^-96): rotation = identity, thrust_force = 0.
//      anything of the result not finite (an overflow of a finite but absurd state): the lane is not guided, as in 1.  The two
//        column norms |x| and |y| count as results: a norm that overflows to +inf where its column is still finite (|F| about
//        1e19 N) would otherwise divide that column to zero - a finite matrix that is no rotation.
//    So no finite state gives a NaN matrix, and every guided lane's matrix is orthonormal.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"

#define FPV_CHASE_PARALLEL 1.0e-12f     // |F x b|^2 <= this |F|^2 |b|^2: F and b are parallel

// What a call reads besides the drones: uniform, the kernel argument.
struct FpvChaseK {
    float rr[9];                        // rel_rot, row-major
    float rel[3];                       // rel_pos
    float f, cx, cy, w, h;              // focal length, W/2, H/2, W, H
    float max_depth;
    float tc[3], tr;                    // the target: centre, radius
    float gz;                           // -9.81 m
    float vdrag, vlift, tof, keep, uwb;
    int32_t frame, mode;                // FPV_CHASE_WORLD / _DRONE, FPV_CHASE_LEVEL / _FRONTARGET
    FpvPidK<float> pid;                 // axis 0
};

// the kernel's argument: the state rows read (p, v, q), the PID rows read and written, the optional pixels, the outputs
struct FpvChaseArgs {
    const float* state; int64_t ld; float* pid_state; int64_t pid_ld; const float* pixel; float* rotation; float* thrust;
    float* pixel_out; uint8_t* visible; int64_t n; FpvChaseK K;
};

struct FpvChaseOut { float rot[9]; float thrust, u, v; bool seen, guided; };

FPV_HD bool fpv_chase_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// One drone against the target of centre (tcx, tcy, tcz) and radius tr (K.tc / K.tr are not read: the pursuit task, fpv_pursuit.h,
// passes each drone's own target).  have_pixel: (pu, pv) is the caller's pixel; else it is computed.  integ / dflt / last / first
// are the lane's PID rows (FPV_PID_*), advanced only when o.guided.
FPV_HD void fpv_chase_lane_at(const FpvChaseK& K, float tcx, float tcy, float tcz, float tr, float px, float py, float pz, float vx,
                              float vy, float vz, FpvQuat q, bool have_pixel, float pu, float pv, float& integ, float& dflt, float& last,
                              float& first, FpvChaseOut& o)
{
    const float qnan = fpv_bits_f32(0x7fc00000u);
    const FpvRot R = fpv_rot(q);
    // ---- 1. the pixel
    float u = pu, v = pv;
    bool seen;
    if (have_pixel) {
        seen = u == u && v == v;
    } else {
        const float ox = fmaf(R.r00, K.rel[0], fmaf(R.r01, K.rel[1], fmaf(R.r02, K.rel[2], px)));
        const float oy = fmaf(R.r10, K.rel[0], fmaf(R.r11, K.rel[1], fmaf(R.r12, K.rel[2], py)));
        const float oz = fmaf(R.r20, K.rel[0], fmaf(R.r21, K.rel[1], fmaf(R.r22, K.rel[2], pz)));
        const float wx = tcx - ox, wy = tcy - oy, wz = tcz - oz;
        const float bx = fmaf(R.r00, wx, fmaf(R.r10, wy, R.r20 * wz));      // R^T (c - o)
        const float by = fmaf(R.r01, wx, fmaf(R.r11, wy, R.r21 * wz));
        const float bz = fmaf(R.r02, wx, fmaf(R.r12, wy, R.r22 * wz));
        const float cxp = fmaf(K.rr[0], bx, fmaf(K.rr[3], by, K.rr[6] * bz));   // rel_rot^T
        const float cyp = fmaf(K.rr[1], bx, fmaf(K.rr[4], by, K.rr[7] * bz));
        const float czp = fmaf(K.rr[2], bx, fmaf(K.rr[5], by, K.rr[8] * bz));
        u = (K.f * cxp) / czp + K.cx;
        v = (K.f * cyp) / czp + K.cy;
        seen = czp > 0.0f && czp <= K.max_depth && u >= 0.0f && u < K.w && v >= 0.0f && v < K.h;
    }
    // ---- 2. the direction
    const float xn = (u - K.cx) / K.f, yn = (v - K.cy) / K.f;
    const float ex = fmaf(K.rr[0], xn, fmaf(K.rr[1], yn, K.rr[2])), ey = fmaf(K.rr[3], xn, fmaf(K.rr[4], yn, K.rr[5]));
    const float ez = fmaf(K.rr[6], xn, fmaf(K.rr[7], yn, K.rr[8]));
    const float hx = fmaf(R.r00, ex, fmaf(R.r01, ey, R.r02 * ez)), hy = fmaf(R.r10, ex, fmaf(R.r11, ey, R.r12 * ez));
    const float hz = fmaf(R.r20, ex, fmaf(R.r21, ey, R.r22 * ez));
    const float hn = fpv_sqrt_flushed(fmaf(hx, hx, fmaf(hy, hy, hz * hz)));
    const float dx = hx / hn, dy = hy / hn, dz = hz / hn;
    // ---- 3. the law
    const bool body = K.frame == FPV_CHASE_DRONE;
    const float gx = body ? R.r02 * K.gz : 0.0f, gy = body ? R.r12 * K.gz : 0.0f, gzz = body ? R.r22 * K.gz : K.gz;
    const float wx = body ? fmaf(R.r00, vx, fmaf(R.r01, vy, R.r02 * vz)) : vx;
    const float wy = body ? fmaf(R.r10, vx, fmaf(R.r11, vy, R.r12 * vz)) : vy;
    const float wz = body ? fmaf(R.r20, vx, fmaf(R.r21, vy, R.r22 * vz)) : vz;
    const float s = fpv_sqrt_flushed(fmaf(vx, vx, fmaf(vy, vy, vz * vz)));
    const float k = fmaf(wx, dx, fmaf(wy, dy, wz * dz)) / (s == 0.0f ? 1.0f : s);
    const float drag = s == 0.0f ? 0.0f : -(K.vdrag * ((1.0f - k) * 0.5f) * s);
    const float lift = pz < K.tof ? -(K.tof - pz) * K.vlift * (1.0f + fabsf(vz)) : 0.0f;
    const float tx = px - tcx, ty = py - tcy, tz = pz - tcz;
    const float far = fpv_sqrt_flushed(fmaf(tx, tx, fmaf(ty, ty, tz * tz))) - tr;
    const float dist = far < K.uwb ? far : K.uwb;
    float i2 = integ, l2 = last, d2 = dflt;
    const float m = fpv_clamp(fpv_pid_axis<float, 1>(K.pid, 0, dist, K.keep, first != 0.0f, i2, l2, d2), K.pid.min_output, K.pid.max_output);
    const float Fx = fmaf(m, dx, fmaf(drag, wx, fmaf(lift, gx, -gx)));
    const float Fy = fmaf(m, dy, fmaf(drag, wy, fmaf(lift, gy, -gy)));
    const float Fz = fmaf(m, dz, fmaf(drag, wz, fmaf(lift, gzz, -gzz)));
    const float ff = fmaf(Fx, Fx, fmaf(Fy, Fy, Fz * Fz));
    const float fn = fpv_sqrt_flushed(ff);
    // the second operand of the first cross product, replaced where F is parallel to it (4.)
    const bool level = K.mode == FPV_CHASE_LEVEL;
    float bx = level ? gx : dx, by = level ? gy : dy, bz = level ? gzz : dz;
    float yx = fmaf(Fy, bz, -(Fz * by)), yy = fmaf(Fz, bx, -(Fx * bz)), yz = fmaf(Fx, by, -(Fy * bx));
    float yy2 = fmaf(yx, yx, fmaf(yy, yy, yz * yz));
    if (!(yy2 > FPV_CHASE_PARALLEL * ff * fmaf(bx, bx, fmaf(by, by, bz * bz)))) {
        yx = 0.0f; yy = Fz; yz = -Fy;                                       // F x (1, 0, 0)
        yy2 = fmaf(yy, yy, yz * yz);
        if (!(yy2 > FPV_CHASE_PARALLEL * ff)) {
            yx = -Fz; yy = 0.0f; yz = Fx;                                   // F x (0, 1, 0)
            yy2 = fmaf(yx, yx, yz * yz);
        }
    }
    const float xx = fmaf(yy, Fz, -(yz * Fy)), xy = fmaf(yz, Fx, -(yx * Fz)), xz = fmaf(yx, Fy, -(yy * Fx));
    const float xnrm = fpv_sqrt_flushed(fmaf(xx, xx, fmaf(xy, xy, xz * xz))), ynrm = fpv_sqrt_flushed(yy2);
    const bool zero = fn == 0.0f;
    o.rot[0] = zero ? 1.0f : xx / xnrm; o.rot[1] = zero ? 0.0f : yx / ynrm; o.rot[2] = zero ? 0.0f : Fx / fn;
    o.rot[3] = zero ? 0.0f : xy / xnrm; o.rot[4] = zero ? 1.0f : yy / ynrm; o.rot[5] = zero ? 0.0f : Fy / fn;
    o.rot[6] = zero ? 0.0f : xz / xnrm; o.rot[7] = zero ? 0.0f : yz / ynrm; o.rot[8] = zero ? 1.0f : Fz / fn;
    bool fin = fpv_chase_finite(fn) && fpv_chase_finite(xnrm) && fpv_chase_finite(ynrm);
    for (int j = 0; j < 9; ++j) fin = fin && fpv_chase_finite(o.rot[j]);
    o.seen = seen;
    o.guided = seen && fin;
    if (!o.guided) {
        for (int j = 0; j < 9; ++j) o.rot[j] = (j == 0 || j == 4 || j == 8) ? 1.0f : 0.0f;
    } else {
        integ = i2; last = l2; dflt = d2; first = 0.0f;
    }
    o.thrust = o.guided ? fn : qnan;
    o.u = seen ? u : qnan;
    o.v = seen ? v : qnan;
}

// One drone against the call's shared target K.tc / K.tr
FPV_HD void fpv_chase_lane(const FpvChaseK& K, float px, float py, float pz, float vx, float vy, float vz, FpvQuat q, bool have_pixel,
                           float pu, float pv, float& integ, float& dflt, float& last, float& first, FpvChaseOut& o)
{
    fpv_chase_lane_at(K, K.tc[0], K.tc[1], K.tc[2], K.tr, px, py, pz, vx, vy, vz, q, have_pixel, pu, pv, integ, dflt, last, first, o);
}

// Host: the camera numbers of a chase from a camera (the arithmetic of DESIGN 3.8's derive, without an image's limits): double.
// FPV_OK, or FPV_EPARAM with *why set.
static inline int fpv_chase_derive_camera(const fpv_camera_t& c, fpv_chase_t* s, const char** why)
{
    if (c.width < 1 || c.width > FPV_CHASE_MAX_SIDE || c.height < 1 || c.height > FPV_CHASE_MAX_SIDE) { *why = "width and height must be 1..16384 pixels"; return FPV_EPARAM; }
    if (!isfinite(c.fov_deg) || !(c.fov_deg > 0.0) || !(c.fov_deg < 180.0)) { *why = "fov must be in (0, 180) degrees"; return FPV_EPARAM; }
    if (!isfinite(c.pitch_deg)) { *why = "pitch is not finite"; return FPV_EPARAM; }
    for (int k = 0; k < 3; ++k)
        if (!isfinite(c.relative_position[k])) { *why = "relative position is not finite"; return FPV_EPARAM; }
    const double rad = 0.017453292519943295;
    const double sn = sin(c.pitch_deg * rad), cs = cos(c.pitch_deg * rad);
    const double rr[9] = {0.0, sn, cs, 1.0, 0.0, 0.0, 0.0, -cs, sn};
    for (int k = 0; k < 9; ++k) s->relative_rotation[k] = rr[k];
    for (int k = 0; k < 3; ++k) s->relative_position[k] = c.relative_position[k];
    s->focal_length = (double)c.width / (2.0 * tan(c.fov_deg * rad / 2.0));
    s->width = c.width; s->height = c.height;
    return FPV_OK;
}
