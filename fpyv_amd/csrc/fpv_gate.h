// fpv_gate.h - gate courses (include/fpv_abi.h "Gate courses"): the ONE definition of what a step does to a drone's
// race state.  fpv_gate_step below is what the gfx950 kernels of fpv_gate.hip run after the lane function and what fpv_gate_eval
// (fpv_hip.hip, host) runs: the same operations in the same order on the same fp32 values, so the host reproduces the kernels'
// words, rewards, done flags and observation rows bit for bit.  The descriptor rows come from fpv_gates_derive (host, double
// arithmetic narrowed once, at the end of this file).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"

// a descriptor row as four 16-byte groups (one ds_read_b128 / global_load_dwordx4 each):
//   [0] c.x c.y c.z n.x   [1] n.y n.z u.x u.y   [2] u.z w.x w.y w.z   [3] a hz zc r2
// Only groups 0 and 1 are read every step (c and n); 2 and 3 inside the rare forward-crossing branch.
typedef float fpv_gate_v4 __attribute__((ext_vector_type(4)));
#define FPV_GATE_GROUPS (FPV_GATE_FLOATS / 4)

struct FpvGateK {                // uniform constants of a course (fpv_set_gates)
    float progress_gain, pass_bonus, finish_bonus, miss_penalty, crash_penalty;
    uint32_t count;              // 1..FPV_MAX_GATES
    uint32_t finish_at;          // laps * count, 0 = endless
    uint32_t miss_done;
};

struct FpvGateCN { float cx, cy, cz, nx, ny, nz; };     // centre and normal of one gate: what every step reads
struct FpvGateOut { uint32_t word; float reward; bool done; };

// the gate a word points at; a word the caller filled with anything else reads gate 0 (the table has `count` rows)
FPV_HD uint32_t fpv_gate_index(uint32_t word, uint32_t count)
{
    const uint32_t g = word & 0xffu;
    return g < count ? g : 0u;
}

// P: a pointer to the gate's first 16-byte group - host or global memory, or the workgroup's LDS copy of the table
template <class P>
FPV_HD FpvGateCN fpv_gate_cn(P d)
{
    const fpv_gate_v4 a = d[0], b = d[1];
    FpvGateCN r;
    r.cx = a.x; r.cy = a.y; r.cz = a.z; r.nx = a.w; r.ny = b.x; r.nz = b.y;
    return r;
}

// One step of the race for one drone.  `cn` and `d` describe gate g = fpv_gate_index(word, count); (pox, poy, poz) is the position
// the step loaded, (pnx, pny, pnz) the position after the update and before any reset, `phys_done` the lane function's done.
// OUT = false skips the reward (the quiet steps of a k-step launch).  The word's reset is fpv_gate_word_reset, the caller's.
template <bool OUT = true, class P>
FPV_HD FpvGateOut fpv_gate_step(const FpvGateK& G, const FpvGateCN& cn, P d, uint32_t word, float pox, float poy, float poz,
                                float pnx, float pny, float pnz, bool phys_done)
{
    const uint32_t g = fpv_gate_index(word, G.count);
    uint32_t passed = word >> 10, next = g, ev = FPV_GATE_EVENT_NONE;
    const float ox = pox - cn.cx, oy = poy - cn.cy, oz = poz - cn.cz;
    const float ex = pnx - cn.cx, ey = pny - cn.cy, ez = pnz - cn.cz;
    float s0 = fmaf(cn.nx, ox, fmaf(cn.ny, oy, cn.nz * oz));
    const float s1 = fmaf(cn.nx, ex, fmaf(cn.ny, ey, cn.nz * ez));
    const bool cross = s0 < 0.0f && s1 >= 0.0f;
    if (FPV_WAVE_ANY(cross)) {
        // rare: where the segment meets the plane, in the gate's own axes (u, w and the aperture are read only here)
        FPV_KEEP_HERE(s0);
        const fpv_gate_v4 b = d[1], c = d[2], e = d[3];
        const float t = s0 / (s0 - s1);
        const float xx = fmaf(t, pnx - pox, ox), xy = fmaf(t, pny - poy, oy), xz = fmaf(t, pnz - poz, oz);
        const float y = fmaf(b.z, xx, fmaf(b.w, xy, c.x * xz));
        const float z = fmaf(c.y, xx, fmaf(c.z, xy, c.w * xz));
        const float zz = z - e.z;
        const bool inside = fabsf(y) <= e.x && fabsf(z) <= e.y && fmaf(y, y, zz * zz) <= e.w;
        if (cross) {
            if (inside) {
                passed = passed < FPV_GATE_MAX_PASSED ? passed + 1u : passed;
                next = g + 1u < G.count ? g + 1u : 0u;
                ev = (G.finish_at != 0u && passed == G.finish_at) ? FPV_GATE_EVENT_FINISH : FPV_GATE_EVENT_PASS;
            } else {
                ev = FPV_GATE_EVENT_MISS;
            }
        }
    }
    FpvGateOut o;
    o.word = next | (ev << 8) | (passed << 10);
    o.done = phys_done || ev == FPV_GATE_EVENT_FINISH || (ev == FPV_GATE_EVENT_MISS && G.miss_done != 0u);
    o.reward = 0.0f;
    if (OUT) {
        const float d0 = fpv_sqrt_flushed(fmaf(ox, ox, fmaf(oy, oy, oz * oz)));
        const float d1 = fpv_sqrt_flushed(fmaf(ex, ex, fmaf(ey, ey, ez * ez)));
        float r = G.progress_gain * (d0 - d1);
        r += (ev == FPV_GATE_EVENT_PASS || ev == FPV_GATE_EVENT_FINISH) ? G.pass_bonus : 0.0f;
        r += ev == FPV_GATE_EVENT_FINISH ? G.finish_bonus : 0.0f;
        r -= ev == FPV_GATE_EVENT_MISS ? G.miss_penalty : 0.0f;
        r -= phys_done ? G.crash_penalty : 0.0f;
        o.reward = r;
    }
    return o;
}

// any reset of a lane: no gate passed, back to its start gate; the event bits keep describing the step that ended
FPV_HD uint32_t fpv_gate_word_reset(uint32_t word, uint32_t start, uint32_t count)
{
    return (word & 0x300u) | (start < count ? start : 0u);
}

// the observation rows of gate h (`cn`) for a drone at p with attitude q: R^T (c - p), R^T n
FPV_HD void fpv_gate_obs(const FpvGateCN& cn, const FpvQuat& q, float px, float py, float pz, float obs[6])
{
    const FpvRot R = fpv_rot(q);
    const float ex = cn.cx - px, ey = cn.cy - py, ez = cn.cz - pz;
    obs[0] = fmaf(R.r00, ex, fmaf(R.r10, ey, R.r20 * ez));
    obs[1] = fmaf(R.r01, ex, fmaf(R.r11, ey, R.r21 * ez));
    obs[2] = fmaf(R.r02, ex, fmaf(R.r12, ey, R.r22 * ez));
    obs[3] = fmaf(R.r00, cn.nx, fmaf(R.r10, cn.ny, R.r20 * cn.nz));
    obs[4] = fmaf(R.r01, cn.nx, fmaf(R.r11, cn.ny, R.r21 * cn.nz));
    obs[5] = fmaf(R.r02, cn.nx, fmaf(R.r12, cn.ny, R.r22 * cn.nz));
}

// Host: the descriptor row of one gate, double arithmetic narrowed once.  FPV_OK, or FPV_EPARAM with *why set.
static inline int fpv_derive_gate_row(const fpv_gate_t& g, float out[FPV_GATE_FLOATS], const char** why)
{
    if (!(g.size > 0.0) || !isfinite(g.size)) { *why = "size must be positive and finite"; return FPV_EPARAM; }
    if (g.shape < FPV_GATE_RECTANGLE || g.shape > FPV_GATE_HALF_CIRCLE) { *why = "unknown shape (0 rectangle, 1 circle, 2 half_circle)"; return FPV_EPARAM; }
    for (int k = 0; k < 3; ++k)
        if (!isfinite(g.position[k])) { *why = "position is not finite"; return FPV_EPARAM; }
    const double* R = g.rotation;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double dot = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b];      // columns a and b
            if (!(fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-6)) { *why = "rotation is not orthonormal to 1e-6"; return FPV_EPARAM; }
        }
    for (int k = 0; k < 3; ++k) {
        out[k] = (float)g.position[k];
        out[3 + k] = (float)R[3 * k];            // n = column 0
        out[6 + k] = (float)R[3 * k + 1];        // u = column 1
        out[9 + k] = (float)R[3 * k + 2];        // w = column 2
    }
    const double half = 0.5 * g.size;
    if (g.shape == FPV_GATE_RECTANGLE) {
        out[12] = out[13] = (float)half; out[14] = 0.0f; out[15] = INFINITY;
    } else if (g.shape == FPV_GATE_CIRCLE) {
        out[12] = out[13] = (float)half; out[14] = 0.0f; out[15] = (float)(half * half);
    } else {
        out[12] = (float)g.size; out[13] = (float)half; out[14] = (float)-half; out[15] = (float)(g.size * g.size);
    }
    return FPV_OK;
}
