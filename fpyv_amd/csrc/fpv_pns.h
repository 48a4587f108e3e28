// fpv_pns.h - point and shoot (include/fpv_abi.h "Point and shoot"): the ONE definition of the reference's steered
// guidance law for a drone, Drone.point_and_shoot(pixel, action, ref_frame, mode) (/root/reference/src/utils/components.py:312-381,
// with convert_action2position :383-387 and thrust2throttle :137).  fpv_pns_lane below is what every lane of the gfx950 kernel of
// fpv_pns.hip runs for its drone and what fpv_pns_eval (host) runs: the same operations in the same order on the same fp32 values -
// explicit fmaf, fpv_sqrt_flushed, plain '/', compare-and-select, fpv_clamp, no libm call, -ffp-contract=off - so the host
// reproduces the kernel's outputs bit for bit.  The camera, the pixel of a target's centre, pixel2direction and the frame are those
// of the target chase (fpv_chase.h 1., 2., 3. last line, 4.), restated here on the same FpvChaseK so that fpv_chase.h and the two
// kernels built from it stay byte for byte what they were.
//
// 1. Pixel: the caller's (x, y), seen iff neither is NaN, or the projected centre of the drone's target exactly as fpv_chase.h 1.
//    A lane that does not see the target, or whose action holds a NaN or an infinity, is NOT GUIDED: thrust = NaN, rotation =
//    identity, visible = 0, pixel_velocity = NaN, throttle = NaN, limited = 0; its PID rows and prev_pixel stay as they were.
// 2. Commands: pixel += (a2 W/2, a3 H/2) (:322-323); position.y = trunc((H/2)(1 + a1)) (:383-387, astype(int) truncates toward
//    zero; the action is not clipped).  a0 only feeds position.x and yaw_angle (:355), which the reference computes and discards
//    (:379 is commented out): neither is computed here.
// 3. Pixel velocity (:325-330): prev_pixel NaN is the reference's None: velocity 0; else (pixel - prev_pixel) / dt.  prev_pixel =
//    pixel.
// 4. Force: d = pixel2direction(pixel) (world frame in both ref_frames, :332); virtual drag as the chase's (:336-337 / :340-341:
//    `-(k - 1) / 2 * -R @ v * |v|` is the scalar (1 - k) / 2 |v| times -(R v), formed here as one scalar times w);
//    lift = [p.z < tof] (-(tof - p.z) virtual_lift (-min(v.z, 0))) g (:345);
//    m = PID(pixel.y, position.y), clipped by the PID itself (:350, components.py:54) - fpv_pid_axis<float, 1> on the four rows the
//    chase uses;  B = drag + lift - g,  F = m d + B (:352).
// 5. Thrust limit (:358-366).  The reference shrinks m in a loop until |F| <= Fmax; that loop is a fixed-point iteration of up to
//    10^3 trips that ends where |m d + B| = Fmax and never ends when |min_output d + B| > Fmax.  This build takes the loop's limit in
//    closed form: with b = d . B the larger root of |m d + B|^2 = Fmax^2 is  r = -b + sqrt(b^2 - |B|^2 + Fmax^2).  When |F| > Fmax:
//        m = clip(r, min_output, max_output), F recomputed;  thrust_force = Fmax when r was not clipped (|F(r)| = Fmax is what r
//        solves; the fp32 |F| of the recomputed F is an ulp or two off and is used for the normalisation only), else |F|;  limited = 1.
//        Out of reach - the discriminant is negative, or r was clipped and |F| > Fmax still: m = min_output, the direction of that
//        F, thrust_force = Fmax;  limited = 2.
//    No loop.  Known difference: when |F(m0)| exceeds Fmax by less than 1e-4 of it the reference's first `x 0.9999` can end its loop
//    just below the limit; the closed form returns the limit.
// 6. Frame (:370-380): level: y = F x g;  frontarget: y = F x d;  x = y x F;  columns x / |x|, y / |y|, F / |F|.  Where the reference
//    gives NaN the chase's rules hold (fpv_chase.h 4.): zero drag for |v| = 0, the replacement operand for a parallel cross product,
//    F = 0 -> identity and thrust 0, a result that is not finite -> not guided.
// 7. Restart: a lane whose restart byte is set first resets its PID rows (PID.reset, components.py:35-41) and its prev_pixel
//    (Drone.reset, :166-168) - and stores them even when it is then not guided.
// 8. throttle = clip((c3 T^3 + c2 T^2 + c1 T + c0) / 100 * 2 - 1, -1, 1) for T = thrust_force (:137, Horner like numpy.polyval).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"
#include "fpv_chase.h"

// What a call reads besides the drones: uniform, the kernel argument.  C: the camera, max_depth, gz, vdrag, vlift, tof, frame, mode
// and pid of the chase (its tc, tr, keep and uwb are not read).
struct FpvPnsK {
    FpvChaseK C;
    float fmax;                         // max_throttle_in_force
    float inv[4];                       // thrust -> throttle percent, highest power first
    float tc[3];                        // the shared target's centre
};

// the kernel's argument: the state rows read (p, v, q), the PID and prev_pixel rows read and written, the optional inputs, the outputs
struct FpvPnsArgs {
    const float* state; int64_t ld; float* pid_state; int64_t pid_ld; float* prev_pixel; int64_t prev_ld; const float* pixel;
    const float* target_rows; int64_t target_ld; const float* action; const uint8_t* restart; float* rotation; float* thrust;
    float* pixel_velocity; uint8_t* limited; uint8_t* visible; float* throttle; int64_t n; FpvPnsK K;
};

struct FpvPnsOut { float rot[9]; float thrust, throttle, velx, vely; uint8_t limited; bool seen, guided; };

// One drone.  have_pixel: (pu, pv) is the caller's pixel; else the centre (tcx, tcy, tcz) is projected.  (a0..a3) the action.
// integ / dflt / last / first are the lane's PID rows and (ppx, ppy) its prev_pixel: reset first when `restart`, advanced only
// when o.guided.
FPV_HD void fpv_pns_lane(const FpvPnsK& P, float tcx, float tcy, float tcz, float px, float py, float pz, float vx, float vy, float vz,
                         FpvQuat q, bool have_pixel, float pu, float pv, float a0, float a1, float a2, float a3, bool restart, float& integ,
                         float& dflt, float& last, float& first, float& ppx, float& ppy, FpvPnsOut& o)
{
    const FpvChaseK& K = P.C;
    const float qnan = fpv_bits_f32(0x7fc00000u);
    const FpvRot R = fpv_rot(q);
    if (restart) { integ = 0.0f; dflt = 0.0f; last = 0.0f; first = 1.0f; ppx = qnan; ppy = qnan; }         // 7.
    // ---- 1. the pixel (fpv_chase.h 1.)
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
    seen = seen && fpv_chase_finite(a0) && fpv_chase_finite(a1) && fpv_chase_finite(a2) && fpv_chase_finite(a3);
    // ---- 2. the commands
    u = fmaf(a2, K.cx, u);                                                   // :322-323
    v = fmaf(a3, K.cy, v);
    const float want = __builtin_truncf(fmaf(K.cy, a1, K.cy));               // :383-387, position[1]
    // ---- 3. the pixel velocity
    const bool none = ppx != ppx || ppy != ppy;                              // :325
    const float velx = none ? 0.0f : (u - ppx) / K.pid.dt, vely = none ? 0.0f : (v - ppy) / K.pid.dt;
    // ---- 4. the direction (fpv_chase.h 2.) and the force
    const float xn = (u - K.cx) / K.f, yn = (v - K.cy) / K.f;
    const float ex = fmaf(K.rr[0], xn, fmaf(K.rr[1], yn, K.rr[2])), ey = fmaf(K.rr[3], xn, fmaf(K.rr[4], yn, K.rr[5]));
    const float ez = fmaf(K.rr[6], xn, fmaf(K.rr[7], yn, K.rr[8]));
    const float hx = fmaf(R.r00, ex, fmaf(R.r01, ey, R.r02 * ez)), hy = fmaf(R.r10, ex, fmaf(R.r11, ey, R.r12 * ez));
    const float hz = fmaf(R.r20, ex, fmaf(R.r21, ey, R.r22 * ez));
    const float hn = fpv_sqrt_flushed(fmaf(hx, hx, fmaf(hy, hy, hz * hz)));
    const float dx = hx / hn, dy = hy / hn, dz = hz / hn;
    const bool body = K.frame == FPV_CHASE_DRONE;
    const float gx = body ? R.r02 * K.gz : 0.0f, gy = body ? R.r12 * K.gz : 0.0f, gzz = body ? R.r22 * K.gz : K.gz;
    const float wx = body ? fmaf(R.r00, vx, fmaf(R.r01, vy, R.r02 * vz)) : vx;
    const float wy = body ? fmaf(R.r10, vx, fmaf(R.r11, vy, R.r12 * vz)) : vy;
    const float wz = body ? fmaf(R.r20, vx, fmaf(R.r21, vy, R.r22 * vz)) : vz;
    const float s = fpv_sqrt_flushed(fmaf(vx, vx, fmaf(vy, vy, vz * vz)));
    const float k = fmaf(wx, dx, fmaf(wy, dy, wz * dz)) / (s == 0.0f ? 1.0f : s);
    const float drag = s == 0.0f ? 0.0f : -(K.vdrag * ((1.0f - k) * 0.5f) * s);
    const float lift = pz < K.tof ? -(K.tof - pz) * K.vlift * (vz < 0.0f ? -vz : 0.0f) : 0.0f;       // :345
    float i2 = integ, l2 = last, d2 = dflt;
    float m = fpv_pid_axis<float, 1>(K.pid, 0, v, want, first != 0.0f, i2, l2, d2);                  // :350
    const float Bx = fmaf(drag, wx, fmaf(lift, gx, -gx)), By = fmaf(drag, wy, fmaf(lift, gy, -gy)), Bz = fmaf(drag, wz, fmaf(lift, gzz, -gzz));
    float Fx = fmaf(m, dx, Bx), Fy = fmaf(m, dy, By), Fz = fmaf(m, dz, Bz);                          // :352
    float ff = fmaf(Fx, Fx, fmaf(Fy, Fy, Fz * Fz));
    float fn = fpv_sqrt_flushed(ff);
    // ---- 5. the thrust limit in closed form
    float thrust = fn;
    uint8_t limited = 0;
    if (fn > P.fmax) {
        const float b = fmaf(dx, Bx, fmaf(dy, By, dz * Bz));
        const float disc = fmaf(b, b, fmaf(P.fmax, P.fmax, -fmaf(Bx, Bx, fmaf(By, By, Bz * Bz))));
        const float r = fpv_sqrt_flushed(disc) - b;
        m = fpv_clamp(r, K.pid.min_output, K.pid.max_output);
        Fx = fmaf(m, dx, Bx); Fy = fmaf(m, dy, By); Fz = fmaf(m, dz, Bz);
        ff = fmaf(Fx, Fx, fmaf(Fy, Fy, Fz * Fz));
        fn = fpv_sqrt_flushed(ff);
        const bool solved = disc >= 0.0f && m == r;
        limited = 1;
        thrust = solved ? P.fmax : fn;
        if (!(disc >= 0.0f) || (!solved && fn > P.fmax)) {
            m = K.pid.min_output;
            Fx = fmaf(m, dx, Bx); Fy = fmaf(m, dy, By); Fz = fmaf(m, dz, Bz);
            ff = fmaf(Fx, Fx, fmaf(Fy, Fy, Fz * Fz));
            fn = fpv_sqrt_flushed(ff);
            limited = 2;
            thrust = P.fmax;
        }
    }
    // ---- 6. the frame (fpv_chase.h 3. last line and 4.)
    const bool level = K.mode == FPV_CHASE_LEVEL;
    const float bx = level ? gx : dx, by = level ? gy : dy, bz = level ? gzz : dz;
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
    bool fin = fpv_chase_finite(fn) && fpv_chase_finite(xnrm) && fpv_chase_finite(ynrm) && fpv_chase_finite(velx) && fpv_chase_finite(vely);
    for (int j = 0; j < 9; ++j) fin = fin && fpv_chase_finite(o.rot[j]);
    o.seen = seen;
    o.guided = seen && fin;
    if (!o.guided) {
        for (int j = 0; j < 9; ++j) o.rot[j] = (j == 0 || j == 4 || j == 8) ? 1.0f : 0.0f;
    } else {
        integ = i2; last = l2; dflt = d2; first = 0.0f; ppx = u; ppy = v;
    }
    // ---- 8. the throttle of the thrust
    const float pct = fmaf(fmaf(fmaf(P.inv[0], thrust, P.inv[1]), thrust, P.inv[2]), thrust, P.inv[3]);
    o.thrust = o.guided ? thrust : qnan;
    o.throttle = o.guided ? fpv_clamp(pct / 100.0f * 2.0f - 1.0f, -1.0f, 1.0f) : qnan;
    o.velx = o.guided ? velx : qnan;
    o.vely = o.guided ? vely : qnan;
    o.limited = o.guided ? limited : (uint8_t)0;
}
