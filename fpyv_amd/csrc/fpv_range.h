// fpv_range.h - the range sensor (include/fpv_abi.h "Range scan"): the ONE definition of what a drone's rays report.
// fpv_range_lane below is what the gfx950 kernel of fpv_range.hip runs for its drone and what fpv_range_eval (fpv_hip.hip, host)
// runs: the same operations in the same order on the same fp32 values - explicit fmaf, fpv_sqrt_flushed, plain '/', compare-and-
// select instead of fmaxf / fminf (whose answer for -0 against +0 is the implementation's), no libm call - so the host reproduces
// the kernel's ranges bit for bit.  What a ray does with ONE object is defined here once, for this sensor and for the depth camera
// (fpv_depth.h fpv_depth_pixel): fpv_range_solid (the interval), fpv_range_nearer (the hit rule), fpv_range_near (the cull's test).
//
// Semantics.  A ray set holds 1..FPV_MAX_RAYS directions d_b in the body frame (fpv_rays_derive: unit in double, narrowed once).
// The ray of a drone starts at o = p and runs along d = R(q) d_b, R = fpv_rot(q) (body -> world); d is NOT renormalised and a range
// is the parameter t along d.  Every object is a convex solid in the geometry fpv_collide_objects uses - Ground the half-space
// z <= 0, Cylinder (x-ob.x)^2 + (y-ob.y)^2 <= radius^2 with ob.z <= z <= ob.z + height, Target the ball of `radius` - and a ray
// meets a convex solid in ONE interval [t_in, t_out] (the cylinder: the interval of the infinite cylinder cut with the interval
// of the z-slab); an empty interval is t_in = +inf > t_out = -inf.  The object is hit when t_in <= t_out && t_out >= 0, at range
// max(t_in, 0): an origin inside a solid reports 0.  range = min(max_range, min over the objects hit); nothing hit, an empty list:
// max_range.
//
// Forms that do not cancel.  Ball and circle: with b = oc.d and a = d.d the ray's closest point to the centre is at t_m = b / a,
// the perpendicular vector e = oc - t_m d is formed directly, and the half chord is sqrt((r^2 - |e|^2) / a) - not the textbook
// discriminant b^2 - a (|oc|^2 - r^2), which loses everything when the drone is far from a small object.  What is left is the
// difference t_m - half for a drone close to the surface: an error of ulps of |oc|, which is what DESIGN 3.7 measures it in.
//
// Parallel rays (no NaN).  A ray whose direction has no component across a constraint never changes its answer to it: the
// constraint is satisfied for every t (interval -inf .. +inf) or for none (empty), decided at the origin.  "No component" is
// |d_z| < 1e-12 for the ground and the z-slab and d_x^2 + d_y^2 < 1e-24 for the circle (d.d < 1e-24 for the ball): a ray that
// moves sideways by less than 1e-12 of its length - nothing in fp32 at any max_range - and the threshold keeps every quotient
// below finite (no inf - inf) for coordinates up to 1e19 m.  The three true divisions of a ray - 1 / d_z, 1 / (d_x^2 + d_y^2), 1 / d.d, formed
// once per ray and multiplied with per object (one more rounding than a division per object, a third of the instructions) - are
// taken on a divisor that a select has made 1 in the parallel case; the results of that case are selected, never computed with.  `d_z == 0` over the ground is the parallel
// case of the half-space: 0 below the ground, max_range above it.
//
// The wave-level cull.  Before the ray loop each lane asks, per object, whether its centre is within `thr` of the object's
// bounding-sphere centre (Ground: p_z < thr); `thr` comes from fpv_range_bounds (host, double): (r_b + max_range)(1 + 2e-4) + 1 mm,
// rounded up.  A wave in which no lane is near skips the object for all its rays.  Why the bits cannot depend on that: the
// lane's own flag takes part in the lane's own hit test, on the host and on the device alike, so an object is counted by exactly
// the lanes that are near it whatever the rest of the wave does - the wave's skip only leaves out work whose result every lane
// would have discarded.  Why the flag does not change a range: every point of the solid is within r_b of the centre, so a ray
// point on it has t |d| >= |p - c| - r_b > max_range (1 + 2e-4) + 1 mm, and with |d| <= 1 + 1e-4 (unit rays - fpv_range_constants
// refuses others - through R of a unit quaternion) t exceeds max_range by a relative 1e-4: a thousand times the rounding of the
// fp32 distance test and of the interval arithmetic (ulps of |oc|).  r_b carries the fp32 rounding of the centre.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"

#define FPV_RANGE_PAR_LEN 1.0e-12f      // |d_z| below this: parallel to the ground / the z-slab
#define FPV_RANGE_PAR_SQ 1.0e-24f       // d_x^2 + d_y^2 (d.d) below this: parallel to the cylinder's axis (a ray that does not move)

// What a scan reads besides the drones and the object list: uniform, the kernel argument.  `near` is fpv_range_bounds' row per
// object: the bounding-sphere centre and the distance below which a lane has to test the object (Ground: [3] against p_z).
struct FpvRangeK {
    float max_range;
    int32_t ray_count;
    float rays[FPV_MAX_RAYS][3];
    float near[FPV_MAX_OBJECTS][4];
};

// the kernel's argument: the state rows read (p: rows 0..2, q: rows 6..9 - the leading rows of drone and Racer state alike), the
// range rows written, and the uniform constants
struct FpvRangeArgs { const float* state; int64_t ld; float* ranges; int64_t ranges_ld; int64_t n; FpvRangeK K; FpvObjects T; };

struct FpvInterval { float t_in, t_out; };

// a > b ? a : b and its mirror as compare-and-select: one answer for -0 against +0 on the host and on the device
FPV_HD float fpv_sel_max(float a, float b) { return a > b ? a : b; }
FPV_HD float fpv_sel_min(float a, float b) { return a < b ? a : b; }

// One ray of one lane: the direction, and what every object divides by - formed once per ray with true divisions, on divisors
// that a select has made 1 where the ray is parallel (the flags say so; the quotients of that case are never computed with)
struct FpvRay {
    float dx, dy, dz;
    float inv_dz, inv_a2, inv_a3;       // 1 / d_z, 1 / (d_x^2 + d_y^2), 1 / d.d
    bool par_z, par_2, par_3;
};

FPV_HD FpvRay fpv_range_ray(const FpvRot& R, float bx, float by, float bz)
{
    FpvRay y;
    y.dx = fmaf(R.r00, bx, fmaf(R.r01, by, R.r02 * bz));
    y.dy = fmaf(R.r10, bx, fmaf(R.r11, by, R.r12 * bz));
    y.dz = fmaf(R.r20, bx, fmaf(R.r21, by, R.r22 * bz));
    const float a2 = fmaf(y.dx, y.dx, y.dy * y.dy), a3 = fmaf(y.dz, y.dz, a2);
    y.par_z = fabsf(y.dz) < FPV_RANGE_PAR_LEN; y.par_2 = a2 < FPV_RANGE_PAR_SQ; y.par_3 = a3 < FPV_RANGE_PAR_SQ;
    y.inv_dz = 1.0f / (y.par_z ? 1.0f : y.dz);
    y.inv_a2 = 1.0f / (y.par_2 ? 1.0f : a2);
    y.inv_a3 = 1.0f / (y.par_3 ? 1.0f : a3);
    return y;
}

// the half-space z <= top
FPV_HD FpvInterval fpv_range_below(const FpvRay& y, float oz, float top)
{
    const float t = (top - oz) * y.inv_dz;
    FpvInterval I;
    if (y.par_z) { const bool in = oz <= top; I.t_in = in ? -INFINITY : INFINITY; I.t_out = in ? INFINITY : -INFINITY; }
    else if (y.dz < 0.0f) { I.t_in = t; I.t_out = INFINITY; }
    else { I.t_in = -INFINITY; I.t_out = t; }
    return I;
}

// the slab lo <= z <= hi
FPV_HD FpvInterval fpv_range_slab(const FpvRay& y, float oz, float lo, float hi)
{
    const float t1 = (lo - oz) * y.inv_dz, t2 = (hi - oz) * y.inv_dz;
    FpvInterval I;
    if (y.par_z) { const bool in = lo <= oz && oz <= hi; I.t_in = in ? -INFINITY : INFINITY; I.t_out = in ? INFINITY : -INFINITY; }
    else { I.t_in = fpv_sel_min(t1, t2); I.t_out = fpv_sel_max(t1, t2); }
    return I;
}

// the ball (BALL) or the vertical infinite cylinder (!BALL: z takes no part) of radius r around o + oc
template <bool BALL>
FPV_HD FpvInterval fpv_range_round(const FpvRay& y, float ocx, float ocy, float ocz, float r)
{
    const bool par = BALL ? y.par_3 : y.par_2;
    const float inv_a = BALL ? y.inv_a3 : y.inv_a2;
    const float b = BALL ? fmaf(ocx, y.dx, fmaf(ocy, y.dy, ocz * y.dz)) : fmaf(ocx, y.dx, ocy * y.dy);
    const float tm = par ? 0.0f : b * inv_a;
    const float ex = fmaf(-tm, y.dx, ocx), ey = fmaf(-tm, y.dy, ocy), ez = BALL ? fmaf(-tm, y.dz, ocz) : 0.0f;
    const float e2 = BALL ? fmaf(ex, ex, fmaf(ey, ey, ez * ez)) : fmaf(ex, ex, ey * ey);
    const float h2 = fmaf(r, r, -e2);
    const float half = par ? INFINITY : fpv_sqrt_flushed(h2 * inv_a);
    FpvInterval I;
    const bool meets = h2 >= 0.0f;
    I.t_in = meets ? tm - half : INFINITY;
    I.t_out = meets ? tm + half : -INFINITY;
    return I;
}

// THE per-object body of the range scan and of the depth camera: the interval of the ray from o inside the solid `ob`
FPV_HD FpvInterval fpv_range_solid(const FpvRay& y, float ox, float oy, float oz, const FpvObject& ob)
{
    FpvInterval I;
    if (ob.type == 0) {
        I = fpv_range_below(y, oz, 0.0f);
    } else if (ob.type == 1) {
        I = fpv_range_round<false>(y, ob.x - ox, ob.y - oy, 0.0f, ob.radius);
        const FpvInterval Z = fpv_range_slab(y, oz, ob.z, ob.z + ob.height);
        I.t_in = fpv_sel_max(I.t_in, Z.t_in); I.t_out = fpv_sel_min(I.t_out, Z.t_out);
    } else {
        I = fpv_range_round<true>(y, ob.x - ox, ob.y - oy, ob.z - oz, ob.radius);
    }
    return I;
}

// ... and THE hit rule: `best`, or the range of a solid that is nearer - `counted`: the lane's own cull flag (see the top)
FPV_HD float fpv_range_nearer(const FpvInterval& I, bool counted, float best)
{
    const bool hit = counted && I.t_in <= I.t_out && I.t_out >= 0.0f;
    const float t = fpv_sel_max(I.t_in, 0.0f);
    return (hit && t < best) ? t : best;
}

// THE near test of the cull: is (x, y, z) within c[3] of the bounding-sphere centre c[0..2] (Ground: below c[3])?  `c` is the
// object's `near` row (fpv_range_bounds); the range scan asks for the drone's position, the depth camera for its origin.
FPV_HD bool fpv_range_near(const float* c, int32_t type, float x, float y, float z)
{
    const float ux = x - c[0], uy = y - c[1], uz = z - c[2];
    return type == 0 ? z < c[3] : fmaf(ux, ux, fmaf(uy, uy, uz * uz)) < c[3] * c[3];
}

// One drone, every ray: `out(r, range)` takes the range of ray r (the kernel stores a row element, the host an array element).
template <class Out>
FPV_HD void fpv_range_lane(const FpvRangeK& K, const FpvObjects& T, const FpvQuat& q, float px, float py, float pz, Out&& out)
{
    const FpvRot R = fpv_rot(q);
    // ---- the cull: which objects this lane has to test, and which the wave has (host: the lane is its own wave)
    uint32_t mine = 0u, wave = 0u;
    for (int k = 0; k < T.count; ++k) {
        const bool near = fpv_range_near(K.near[k], T.o[k].type, px, py, pz);
        mine |= near ? 1u << k : 0u;
        if (FPV_WAVE_ANY(near)) wave |= 1u << k;
    }
    // ---- the rays: uniform trip counts, only predicates differ between lanes
    for (int r = 0; r < K.ray_count; ++r) {
        const FpvRay y = fpv_range_ray(R, K.rays[r][0], K.rays[r][1], K.rays[r][2]);
        float best = K.max_range;
        for (int k = 0; k < T.count; ++k) {
            if (!((wave >> k) & 1u)) continue;
            best = fpv_range_nearer(fpv_range_solid(y, px, py, pz, T.o[k]), (mine >> k) & 1u, best);
        }
        out(r, best);
    }
}

// Host: the `near` rows of an object list for one max_range (see "The wave-level cull" above), double arithmetic rounded up.
static inline void fpv_range_bounds(const FpvObjects& T, float max_range, float near[FPV_MAX_OBJECTS][4])
{
    for (int k = 0; k < FPV_MAX_OBJECTS; ++k) near[k][0] = near[k][1] = near[k][2] = near[k][3] = 0.0f;
    for (int k = 0; k < T.count && k < FPV_MAX_OBJECTS; ++k) {
        const FpvObject& ob = T.o[k];
        double c[3] = {0.0, 0.0, 0.0}, rb = 0.0;
        if (ob.type == 1) {
            const double hh = 0.5 * fabs((double)ob.height);
            c[0] = ob.x; c[1] = ob.y; c[2] = (double)ob.z + 0.5 * (double)ob.height;
            rb = sqrt((double)ob.radius * ob.radius + hh * hh);
        } else if (ob.type != 0) {
            c[0] = ob.x; c[1] = ob.y; c[2] = ob.z;
            rb = fabs((double)ob.radius);
        }
        for (int j = 0; j < 3; ++j) {
            near[k][j] = (float)c[j];
            rb += fabs(c[j] - (double)near[k][j]);       // the centre's own rounding
        }
        const double thr = (rb + (double)max_range) * (1.0 + 2.0e-4) + 1.0e-3;
        near[k][3] = nextafterf((float)thr, INFINITY);
    }
}

// Host: unit directions of `count` rays, normalised in double and narrowed once.  FPV_OK, or FPV_EPARAM with *bad the ray.
static inline int fpv_derive_rays(int count, const double* dirs, float* out, int* bad, const char** why)
{
    for (int k = 0; k < count; ++k) {
        const double* d = dirs + 3 * k;
        *bad = k;
        if (!isfinite(d[0]) || !isfinite(d[1]) || !isfinite(d[2])) { *why = "direction is not finite"; return FPV_EPARAM; }
        const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(len > 0.0) || !isfinite(len)) { *why = "direction has no finite, positive length"; return FPV_EPARAM; }
        for (int j = 0; j < 3; ++j) out[3 * k + j] = (float)(d[j] / len);
    }
    return FPV_OK;
}
