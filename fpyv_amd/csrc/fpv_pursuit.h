// fpv_pursuit.h - the pursuit task (include/fpv_abi.h "Pursuit task"): every drone chases a target of its own on a
// circular path of its own, as the reference's simulator does with one drone (/root/reference/src/core/simulator.py:54-110:
// generate_targets once, target.update() every iteration, the guidance law against targets[idx]).  fpv_pursuit_task and _guide below
// are the ONE definition of what happens to a drone and its target in a call: every lane of the gfx950 kernel of fpv_pursuit.hip runs
// them and so does fpv_pursuit_eval on the host - the same operations in the same order on the same fp32 values (explicit fmaf,
// fpv_sqrt_flushed, plain '/', no libm call, -ffp-contract=off), so the host reproduces the kernel bit for bit.
//
// The target rows, targets[FPV_TGT_ROWS][ld], 4-byte cells in the state's column order:
//   CX CY CZ   centre of the path            PATH_R   radius of the path (0: the target stands still at its centre)
//   RADIUS     radius of the sphere          PREV_DIST  the distance the last call measured (what progress is paid against)
//   COUNT      (word) bits 0..16: the path index j in [0, K) of the NEXT update(); bit 31 FPV_TGT_FRESH: the target has not been
//              advanced since it was set, reset or respawned
//   SPAWNS     (word) low 16 bits: respawns so far (the respawn index); high 16 bits: captures in the current episode
// The path is the reference's CircularPath (components.py:743-751, helper_functions.py:151-153): update() puts the target at
// centre + PATH_R (cos th_j, sin th_j, 0), th_j = 2 pi j / K, and steps j.  (cos, sin) come from the shared table circle[K][2]
// (fpv_pursuit_derive: double, rounded once); a coordinate is ONE fmaf(PATH_R, table, centre).  j is kept reduced (j + 1 == K -> 0)
// instead of the reference's free-running count: the same positions, and no wrap of a 32-bit count after 2^32 updates.
// A FRESH target stands where its first update() will put it (index j); that update leaves it there, clears FRESH and steps j.  So
// update() number k after a set / respawn with phase ph gives th_{(ph + k) % K} as the reference's k-th update() of a path started at
// ph does, and the target velocity (t - t_previous) / dt is zero on that first advance.
//
// A call, for one drone (p, v, q after the step; `rebase` = its done byte, or - in the reset call - every lane of the mask):
//   1. advance (unless advance = 0)   2. measure: w = t - p, range = |w|, dist = range - RADIUS (Target.calculate_distance, :773)
//   3. rebase: pays nothing, clears the captures of its episode, respawns when respawn_on_done, PREV_DIST = dist, event 0
//   4. else pays progress (PREV_DIST - dist), PREV_DIST = dist; dist <= capture_distance: + capture, event 1, both counts + 1,
//      respawn, PREV_DIST = the distance to the new target (the jump is never paid)
//   5. respawn: centre = fmaf(span, u, lo) per axis, RADIUS likewise, j = floor(u K), FRESH; u = (w >> 8) 2^-24 of Philox4x32-7 words;
//      PATH_R kept.  key = spawn_seed, counter = (gid lo, gid hi ^ (block << 28), respawn index, FPV_PURSUIT_TAG): block 0 words
//      0..2 = centre x y z, word 3 = radius; block 1 word 0 = phase (j = mulhi(word, K)).  gid = drone_id_offset + lane, the id of
//      the stick noise and the reset jitter.  The reset jitter's counter carries the 64-bit step index in words 2 and 3
//      (fpv_math.h), the physics sample's is (.., "PHYS", 0): word 3 = "TRGT" = 0x54475254 meets the jitter's only at step index
//      >= 0x54475254 * 2^32 (6e18 steps) and the sample's never, so the streams are disjoint under one seed too.
//      After a respawn everything below sees the NEW target (standing at its index j, velocity zero).
//   6. observe: R^T w, R^T (v_target - v), dist; the target keeps its height, and the third component of the difference is formed
//      as the negation -v.z (-0 for v.z = +0)    7. hand the payment to reward[i] / ep_return[i] (never on a rebasing lane, whose
//      last_return the step kernel has just written)    8. GUIDE: the guidance law of fpv_chase.h against THIS target.
#pragma once

#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"
#include "fpv_chase.h"

#define FPV_TGT_INDEX_MASK 0x0001ffffu
#define FPV_PURSUIT_TAG 0x54475254u      /* "TRGT" */

// the uniform data of a call besides the chase's: the kernel argument
struct FpvPursuitK {
    float dt, capture_distance, progress, capture;
    float lo[4], span[4];               // spawn box x y z, sphere radius: lo and hi - lo (narrowed as the reset jitter's are)
    uint32_t seed_lo, seed_hi, gid_lo, gid_hi;
    uint32_t resolution;                // K
    int32_t advance, respawn_on_done, add_to_reward;
};

struct FpvPursuitArgs {
    const float* state; int64_t ld;
    float* targets; int64_t tld;
    const float* circle;                // [K][2]
    const uint8_t* done;                // the done bytes, or the mask of a reset call; null: no lane rebases / every lane is reset
    float* reward; float* ep_return;    // add_to_reward
    float* obs; int64_t obs_ld; float* position; int64_t pos_ld; uint8_t* event; float* reward_out;
    float* pid_state; int64_t pid_ld; float* rotation; float* thrust; float* pixel_out; uint8_t* visible;    // GUIDE
    int64_t n;
    FpvPursuitK P;
    FpvChaseK K;                        // GUIDE (tc / tr unused)
};

// the rows of one target in registers
struct FpvTarget { float cx, cy, cz, path_r, radius, prev_dist; uint32_t count, spawns; };

struct FpvPursuitOut {
    float obs[7], pos[3], paid;
    uint8_t event;
    bool respawned, rebased;
};

// the path index of a COUNT word
FPV_HD uint32_t fpv_pursuit_index(uint32_t count, uint32_t K)
{
    const uint32_t j = count & FPV_TGT_INDEX_MASK;
    return j < K ? j : 0u;              // a cell that was never set: no read past the table
}

// the two table indices a lane reads before it knows anything else: where the target is put by this call (`at`) and where it stood
// before (`before`, used only by an advance of a target that is not fresh)
FPV_HD void fpv_pursuit_indices(uint32_t count, uint32_t K, bool advance, uint32_t& at, uint32_t& before)
{
    const uint32_t j = fpv_pursuit_index(count, K);
    before = j == 0u ? K - 1u : j - 1u;
    at = (advance || (count & FPV_TGT_FRESH)) ? j : before;
}

// the respawn draw (5.): centre, radius and path index of respawn number `index` of drone `gid`
FPV_HD void fpv_pursuit_draw(const FpvPursuitK& P, uint64_t gid, uint32_t index, float c[3], float& radius, uint32_t& j)
{
    uint32_t w0[4], w1[4];
    fpv_philox4x32<FPV_NOISE_PHILOX_ROUNDS>((uint32_t)gid, (uint32_t)(gid >> 32), index, FPV_PURSUIT_TAG, P.seed_lo, P.seed_hi, w0);
    fpv_philox4x32<FPV_NOISE_PHILOX_ROUNDS>((uint32_t)gid, (uint32_t)(gid >> 32) ^ (1u << 28), index, FPV_PURSUIT_TAG, P.seed_lo, P.seed_hi, w1);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = fmaf(P.span[k], (float)(w0[k] >> 8) * 0x1p-24f, P.lo[k]);
    radius = fmaf(P.span[3], (float)(w0[3] >> 8) * 0x1p-24f, P.lo[3]);
    j = (uint32_t)(((uint64_t)w1[0] * (uint64_t)P.resolution) >> 32);
}

// One drone and its target, steps 1 to 7 (the payment is o.paid; the caller hands it over).  (ax, ay) / (bx, by): the table rows of
// fpv_pursuit_indices' `at` / `before`; `circle`: the table, read again only by a lane that respawns.  `rebase`: see above.
FPV_HD void fpv_pursuit_task(const FpvPursuitK& P, const float* circle, uint32_t lane, float px, float py, float pz, float vx, float vy,
                             float vz, FpvQuat q, bool rebase, float ax, float ay, float bx, float by, FpvTarget& T, FpvPursuitOut& o)
{
    // ---- 1. advance
    const bool fresh = (T.count & FPV_TGT_FRESH) != 0u;
    float tx = fmaf(T.path_r, ax, T.cx), ty = fmaf(T.path_r, ay, T.cy), tz = T.cz;
    float ux = 0.0f, uy = 0.0f;                                 // the target's velocity: it keeps its height
    if (P.advance) {
        if (!fresh) {
            ux = (tx - fmaf(T.path_r, bx, T.cx)) / P.dt;
            uy = (ty - fmaf(T.path_r, by, T.cy)) / P.dt;
        }
        const uint32_t j = fpv_pursuit_index(T.count, P.resolution) + 1u;
        T.count = j == P.resolution ? 0u : j;
    }
    // ---- 2. measure
    float wx = tx - px, wy = ty - py, wz = tz - pz;
    float dist = fpv_sqrt_flushed(fmaf(wx, wx, fmaf(wy, wy, wz * wz))) - T.radius;
    // ---- 3. / 4. rebase, or pay and capture
    const bool captured = !rebase && dist <= P.capture_distance;
    o.paid = rebase ? 0.0f : P.progress * (T.prev_dist - dist);
    if (captured) o.paid = o.paid + P.capture;
    o.event = captured ? 1 : 0;
    o.rebased = rebase;
    o.respawned = captured || (rebase && P.respawn_on_done);
    uint32_t respawns = T.spawns & 0xffffu, captures = rebase ? 0u : T.spawns >> 16;
    if (captured) captures = (captures + 1u) & 0xffffu;
    if (o.respawned) {
        // ---- 5. respawn
        float c[3];
        uint32_t j;
        fpv_pursuit_draw(P, (((uint64_t)P.gid_hi << 32) | P.gid_lo) + (uint64_t)lane, respawns, c, T.radius, j);
        respawns = (respawns + 1u) & 0xffffu;
        T.cx = c[0]; T.cy = c[1]; T.cz = c[2];
        T.count = j | FPV_TGT_FRESH;
        tx = fmaf(T.path_r, circle[2u * j], T.cx); ty = fmaf(T.path_r, circle[2u * j + 1u], T.cy); tz = T.cz;
        ux = 0.0f; uy = 0.0f;
        wx = tx - px; wy = ty - py; wz = tz - pz;
        dist = fpv_sqrt_flushed(fmaf(wx, wx, fmaf(wy, wy, wz * wz))) - T.radius;
    }
    T.spawns = respawns | (captures << 16);
    T.prev_dist = dist;
    // ---- 6. observe
    const FpvRot R = fpv_rot(q);
    // (6. above: the negation, not the difference 0 - v.z, which is +0 for v.z = +0)
    const float rx = ux - vx, ry = uy - vy, rz = -vz;
    o.obs[0] = fmaf(R.r00, wx, fmaf(R.r10, wy, R.r20 * wz));
    o.obs[1] = fmaf(R.r01, wx, fmaf(R.r11, wy, R.r21 * wz));
    o.obs[2] = fmaf(R.r02, wx, fmaf(R.r12, wy, R.r22 * wz));
    o.obs[3] = fmaf(R.r00, rx, fmaf(R.r10, ry, R.r20 * rz));
    o.obs[4] = fmaf(R.r01, rx, fmaf(R.r11, ry, R.r21 * rz));
    o.obs[5] = fmaf(R.r02, rx, fmaf(R.r12, ry, R.r22 * rz));
    o.obs[6] = dist;
    o.pos[0] = tx; o.pos[1] = ty; o.pos[2] = tz;
}

// Step 8: the guidance law against the target the task left at (tx, ty, tz) with radius tr.  integ / dflt / last / first are the
// lane's PID rows, cleared first by a rebasing lane (PID.reset, components.py:35-41: what reset(mask) does to them); returns whether
// the rows changed.
FPV_HD bool fpv_pursuit_guide(const FpvChaseK& K, float tx, float ty, float tz, float tr, float px, float py, float pz, float vx, float vy,
                              float vz, FpvQuat q, bool rebase, float& integ, float& dflt, float& last, float& first, FpvChaseOut& g)
{
    if (rebase) { integ = 0.0f; dflt = 0.0f; last = 0.0f; first = 1.0f; }
    fpv_chase_lane_at(K, tx, ty, tz, tr, px, py, pz, vx, vy, vz, q, false, 0.0f, 0.0f, integ, dflt, last, first, g);
    return rebase || g.guided;
}
