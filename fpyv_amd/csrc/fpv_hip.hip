// fpv_hip.hip - gfx950 kernels + the C ABI of include/fpv_abi.h.
//
// One lane = one drone: every wave instruction touches 256 contiguous bytes of one SoA row.  Measured on MI355X
// (profiles/archive/r01_exp_*.log, r03_exp_wide_rows_beyond_mall.log): 128-thread workgroups beat 64/256/512/1024,
// one drone per lane beats 2/4 with float2/float4 rows at 2^20 AND at 2^23 drones, persistent/grid-stride/prefetch
// loops lose to plain oversubscription, non-temporal hints on the once-touched operands (action in, reward/done out)
// are worth ~0.5 %, and a row stride that is NOT a multiple of 8 KiB is worth 6-9 % (fpv_recommended_ld).  A step is:
// 14 row loads + one 16-byte action load per drone -> ~230 VALU instructions in registers (fpv_math.h) -> 14 row stores
// + reward + done.  There is no reuse, no cross-lane data flow and no dense contraction, so the single-step kernels are
// bound by HBM / the Infinity Cache; the k-step kernels (fpv_step_n) keep the drone in registers and are bound by
// vector-instruction issue.  Wave-level primitives on the data path: the ballot that bit-packs the done mask, the
// fp16 kernels' DPP pair exchange, the object pass's wave-level cull.  Uniform constants ride in the kernel argument.
//
// Replaces, per drone: Drone.step /root/reference/src/utils/components.py:220-248,
// Drone.reset :150-169, Racer.step /root/reference/tests/racer_drone_test.py:95-103.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include <type_traits>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_derive.h"
#include "fpv_math.h"
#include "fpv_kernels.h"
#include "fpv_range.h"
#include "fpv_depth.h"
#include "fpv_chase.h"
#include "fpv_pns.h"
#include "fpv_detect.h"
#include "fpv_splat.h"
#include "fpv_pursuit.h"

namespace {


template <bool NOISE = false, bool OBJ = false, bool KAHAN = false, bool OVR = false>
__global__ __launch_bounds__(kStepBlock) FPV_EXP_STEP_ATTR void fpv_drone_step_kernel(FPV_STEP_PARAMS)
{
    constexpr bool SECTIONED = NOISE || (OBJ && OVR);
    constexpr bool PLAIN = !NOISE && !OBJ && !KAHAN && !OVR;
    FPV_STEP_VIEW;
    __shared__ FpvNormalRow ntab[NOISE ? FPV_NTAB_ROWS : 1];
    if (NOISE) stage_normal_table(ntab);
    FPV_STEP_INDEX;
    // lanes past the end leave at once (a ballot over the remaining lanes still yields the right done bits:
    // exited lanes contribute 0, and a wave whose lane 0 is gone is empty)
    if (i >= n) return;
    FpvDroneState s;
    float ro[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, to = 0.0f;
    // ---- 1. issue every load of this lane before the first use; the sticks
    float4 a = (!NOISE || B.action) ? ld_action_any(B.action, B.action_ld, i) : make_float4(0.f, 0.f, 0.f, 0.f);
    // The plain kernel issues the scalar loads of its constants and of the wind HERE, ahead of the 14 row loads, through one
    // view of the arguments: they are then in flight together with the rows, and the wait for them stands after the last row
    // load as before.  Under the rotated traversal the first generation of waves finds its rows in the L2s and used to wait
    // for constants whose loads went out only after the rows'.  A/B in one process at 2^20 drones (profiles/const_block.md):
    // 19.75 against 20.04 us per launch rotated, 22.35 against 22.61 in the plain order; twins of one build differ by 0.005.
    // The wind goes out AFTER the constants: ahead of them, the dead fourth dword of its dwordx4 load is a register that a
    // constant load then takes, and the hazard costs a wait for every scalar load in front of the row loads.
    const FpvStepArgs* T = nullptr;
    float wind[3] = {0.f, 0.f, 0.f};
    FpvK Kt;
    if (PLAIN) {
        T = &fpv_step_args_again();
        Kt = T->K;
        wind[0] = T->B.wx; wind[1] = T->B.wy; wind[2] = T->B.wz;
        __builtin_amdgcn_sched_barrier(0);
    }
    ld_drone(B.state, B.ld, i, s);
    if (NOISE) a = apply_stick_noise(K, B, i, a, ntab);
    if (OVR) {
#pragma unroll
        for (int k = 0; k < 9; ++k) ro[k] = B.rot_over[(int64_t)i * 9 + k];     // 64-bit index: 36 * i can pass 2^32
        to = B.thrust_over[i];
    }
    // no vector load waits behind a scalar load: without this fence the compiler parks the last four row loads behind an
    // s_waitcnt on the constants (+1.4 % per launch, A/B in one process, plain order, rounds 1-3).  The other instantiations
    // still load their constants after it; only the plain kernel's order has been measured under the rotation.
    __builtin_amdgcn_sched_barrier(0);
    // ---- 2. the physics, on its own view of the constants when SECTIONED
    const FpvStepArgs* P = nullptr;
    if (SECTIONED) P = &fpv_step_args_again();
    const FpvK& Kp = SECTIONED ? P->K : PLAIN ? Kt : K;
    const FpvBufD& Bp = SECTIONED ? P->B : B;
    float kc[6];
    if (KAHAN) {
#pragma unroll
        for (int k = 0; k < 6; ++k) kc[k] = row_at(ROW(Bp.pos_comp, k, a_ld), i);
    }
    const FpvStepOut o = fpv_drone_step_lane<OBJ>(Kp, s, a.x, a.y, a.z, a.w, PLAIN ? wind[0] : Bp.wx, PLAIN ? wind[1] : Bp.wy, PLAIN ? wind[2] : Bp.wz, &B_.objs,   // the table stays in the kernarg segment (a local copy of an indexed array would live in scratch)
                                                  KAHAN ? kc : nullptr, OVR ? ro : nullptr, to);
    // ---- 3. the stores
    // OBJ: the store addresses are formed only now - the 14 row-address pairs the compiler would otherwise carry from
    // the loads to the stores (28 VGPRs) come on top of the object pass's own registers (102 VGPRs, 4 waves per SIMD);
    // the plain kernel is faster WITH the carried addresses (profiles/archive/r02_exp_state_cache_policy.log) and keeps them
    uint32_t j = i;
    if (OBJ || SECTIONED) FPV_KEEP_HERE(j);
    const FpvStepArgs* E = nullptr;
    if (SECTIONED) E = &fpv_step_args_again();
    const FpvK& Ke = SECTIONED ? E->K : PLAIN ? Kt : K;
    FpvBufD Bs = B;
    if (SECTIONED) { Bs = E->B; Bs.state = E->state; Bs.ld = E->ld; }
    const FpvBufD& Be = Bs;
    if (KAHAN) {
        const bool rst = (Ke.flags & FPV_FLAG_AUTO_RESET) && o.done;
#pragma unroll
        for (int k = 0; k < 6; ++k) row_at(ROW(Be.pos_comp, k, Be.ld), j) = rst ? 0.0f : kc[k];
    }
    if (Be.accel) {
        ST_OUT(row_at(ROW(Be.accel, 0, Be.ld), j), o.ax); ST_OUT(row_at(ROW(Be.accel, 1, Be.ld), j), o.ay); ST_OUT(row_at(ROW(Be.accel, 2, Be.ld), j), o.az);
    }
    if ((Ke.flags & FPV_FLAG_AUTO_RESET) && o.done) fpv_drone_reset_lane(Ke, s);
    st_drone(Be.state, Be.ld, j, s);
    emit_outputs(Be, j, true, o.reward, o.done);
}


// k steps of Drone.step in ONE launch (fpv_step_n): the loop `for i in range(time_steps): drone.step(...)`
// of src/core/simulator.py:83-156 for pre-computed or in-kernel-generated sticks.  The lane keeps its
// drone (and the noise / Kahan rows) in registers for all k steps; step t+1's action is in flight while
// step t computes; reward/done leave per step only when asked to.  Per env-step this moves
// 16 (action) + (112 + 5)/k bytes instead of 133, so for k >~ 8 the kernel is bound by the fp32 vector ALUs
// (~190 instructions per env-step), not by HBM.  The arithmetic per step is the single-step kernel's lane function,
// called in the same order: results are bit-identical to k fpv_step launches.
//
// Three sections, each with its own view of the arguments (fpv_args_again):
//   1. the QUIET steps - a launch whose outputs leave only after the last step (no per-step stride, no episode
//      bookkeeping) runs its first k-1 steps in a loop with no output code and only the ~35 uniforms the physics
//      needs; the reset pose is loaded inside the (rare) reset branch;
//   2. the remaining steps - the last one, or all of them when reward/done leave per step or episodes are tracked;
//   3. the stores.
// SQ: launched only for the X frame without the ground-spring flag and without objects (plan_launch):
// the quiet steps use the two-height ground flag (fpv_drone_step_lane<.., SQ = true>).
template <bool NOISE, bool OBJ, bool KAHAN, bool SQ = false>
__global__ __launch_bounds__(kStepBlock) void fpv_drone_rollout_kernel(const FpvRollArgs A)
{
    static_assert(!(SQ && OBJ), "the two-height ground flag does not feed the object pass");
    __shared__ FpvNormalRow ntab[NOISE ? FPV_NTAB_ROWS : 1];
    if (NOISE) stage_normal_table(ntab);
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    FpvDroneState s;
    const int k = A.R.k;
    const bool has_action = !NOISE || A.B.action;
    // rows only for fpv_step_n; the k = 1 launches a reset-source handle's fpv_step is routed to (plan_launch) may carry SoA sticks
    float4 a_next = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (SQ) { if (has_action) a_next = ld_action(A.B.action, i); }
    else { if (has_action) a_next = ld_action_any(A.B.action, A.B.action_ld, i); }
    ld_drone(A.B.state, A.B.ld, i, s);
    float ns[4] = {0.f, 0.f, 0.f, 0.f}, kc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (NOISE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ns[c] = row_at(ROW(A.B.noise_state, c, A.B.ld), i);
    }
    if (KAHAN) {
#pragma unroll
        for (int c = 0; c < 6; ++c) kc[c] = row_at(ROW(A.B.pos_comp, c, A.B.ld), i);
    }
    fpv_settle(s.px); fpv_settle(s.py); fpv_settle(s.pz); fpv_settle(s.vx); fpv_settle(s.vy); fpv_settle(s.vz);
    fpv_settle(s.q.w); fpv_settle(s.q.x); fpv_settle(s.q.y); fpv_settle(s.q.z);
    fpv_settle(s.rx); fpv_settle(s.ry); fpv_settle(s.rz); fpv_settle(s.thrust);
    if (NOISE) { fpv_settle(ns[0]); fpv_settle(ns[1]); fpv_settle(ns[2]); fpv_settle(ns[3]); }
    if (KAHAN) { for (int c = 0; c < 6; ++c) fpv_settle(kc[c]); }
    float av[4] = {0.f, 0.f, 0.f, 0.f};

    // one step on the view V of the arguments.  QUIET steps take their next action unconditionally (there is always
    // a step t + 1 behind a quiet one; a held action - stride 0 - is simply read again: 16 bytes from the cache)
    auto one_step = [&](const FpvRollArgs& V, const FpvObjects* objs, const float* ap_next, bool prefetch, int t, auto quiet_c) -> FpvStepOut {
        constexpr bool QUIET = decltype(quiet_c)::value;
        av[0] = a_next.x; av[1] = a_next.y; av[2] = a_next.z; av[3] = a_next.w;
        if ((!NOISE || has_action) && (QUIET || prefetch)) a_next = ld_action(reinterpret_cast<const float4*>(ap_next), i);
        if (NOISE) {
            // the Philox round keys are uniform and loop-invariant: left alone the compiler keeps all fourteen words
            // in SGPRs for the whole loop; seen through an opaque copy of the seed they are scalar adds per step
            // (with an object list the step's own uniforms fill the SGPR file: the generator then reads its few through a
            // view of its own instead of pushing two of the physics' into VGPR lanes)
            const FpvRollArgs& NV = OBJ ? fpv_args_again() : V;
            FpvNoiseK N = NV.K.noise;
            asm volatile("" : "+s"(N.seed_lo), "+s"(N.seed_hi));
            fpv_stick_noise(N, NV.B.step + (uint64_t)t, (uint64_t)i, ntab, ns, av);
        }
        FpvStepOut o = fpv_drone_step_lane<OBJ, !QUIET, SQ && QUIET>(V.K, s, av[0], av[1], av[2], av[3], V.B.wx, V.B.wy, V.B.wz,
                                                                       objs, KAHAN ? kc : nullptr);
        if ((V.K.flags & FPV_FLAG_AUTO_RESET) && o.done) {
            // rare (once per episode and lane): the reset pose comes through its own view, inside the branch
            const FpvRollArgs& Z = fpv_args_again();
            fpv_drone_reset_lane(Z.K, s);
            // (never launched for a handle with a reset source: the SQ bodies stay as they were)
            if constexpr (!SQ) apply_reset_source_k(i, (uint64_t)t, s);
            if (KAHAN) {
#pragma unroll
                for (int c = 0; c < 6; ++c) kc[c] = 0.0f;
            }
        }
        return o;
    };

    int t = 0;
    if (A.B.ep_return == nullptr && A.R.out_stride == 0 && k > 1) {
        // ---- 1. quiet steps: only the optional per-step done_bits row leaves the lane
        const float* ap = reinterpret_cast<const float*>(A.B.action);
        const int64_t astride = A.R.action_stride;
        unsigned long long* bp = A.R.bits_stride ? A.B.done_bits : nullptr;
        const int64_t bstride = A.R.bits_stride;
        auto quiet_step = [&]() {
            ap += astride;
            const FpvStepOut o = one_step(A, &A.B.objs, ap, true, t, std::true_type{});
            if (bp) {
                const unsigned long long mask = __ballot(o.done);
                if ((threadIdx.x & 63) == 0) bp[i >> 6] = mask;
                bp += bstride;
            }
            ++t;
        };
        // two steps per trip, written out (the compiler declines `#pragma unroll` on this loop - it holds ballots and
        // opaque asm -, which is why round 3's "unrolled by two" measured nothing): the register allocator can then
        // alternate the loop-carried registers instead of copying five of them back every step (+2 %, one-process A/B)
        // (not with an object list: its per-object uniforms already fill the SGPR file, two copies of the pass spill)
        if constexpr (!OBJ) { while (t + 1 < k - 1) { quiet_step(); quiet_step(); } }
        while (t < k - 1) quiet_step();
    }
    // ---- 2. the remaining steps, with every output the caller asked for
    FpvStepOut o;
    o.done = false; o.reward = 0.0f; o.ax = o.ay = o.az = 0.0f;
    {
        const FpvRollArgs& G = fpv_args_again();
        RollOut out(G.B, G.R, i, true);
        if (out.bp) out.bp += (int64_t)t * G.R.bits_stride;
        const float* ap = reinterpret_cast<const float*>(G.B.action) + (int64_t)t * G.R.action_stride;
        const int kk = G.R.k;
        if (out.track) { fpv_settle(out.ep_r); fpv_settle(__int_as_float(out.ep_l)); }
        for (; t < kk; ++t) {
            ap += G.R.action_stride;
            o = one_step(G, &G.B.objs, ap, G.R.action_stride != 0 && t + 1 < kk, t, std::false_type{});
            out.template step<false>(i, t, o.reward, o.done);
        }
        out.finish(i, fpv_args_again().B);
    }
    // ---- 3. the stores: row addresses are formed only now (computed before the loops they would sit in ~30 registers
    //         for all k steps)
    const FpvRollArgs& E = fpv_args_again();
    uint32_t j = i;
    asm volatile("" : "+v"(j));
    if (E.B.accel) {
        ST_OUT(row_at(ROW(E.B.accel, 0, E.B.ld), j), o.ax); ST_OUT(row_at(ROW(E.B.accel, 1, E.B.ld), j), o.ay); ST_OUT(row_at(ROW(E.B.accel, 2, E.B.ld), j), o.az);
    }
    st_drone(E.B.state, E.B.ld, j, s);
    if (NOISE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) row_at(ROW(E.B.noise_state, c, E.B.ld), j) = ns[c];
        if (E.B.action_out) E.B.action_out[j] = make_float4(av[0], av[1], av[2], av[3]);
    }
    if (KAHAN) {
#pragma unroll
        for (int c = 0; c < 6; ++c) row_at(ROW(E.B.pos_comp, c, E.B.ld), j) = kc[c];
    }
}

// Same step + an array-of-structures observation row per drone, obs_aos[i][16] =
// (p3, v3, q4 wxyz, rates3, R_new@acc 3): what a learner that wants an [N, D] matrix consumes, and
// the reference's IMU-style return values (components.py:247-248) in one place.  A lane owns a
// 64-byte row, so storing it directly would scatter 16 dwords at a 64-byte stride; instead each
// wave transposes its 64 x 16 tile through LDS (row pitch 17 words: conflict-free writes) and
// stores it as 4 fully coalesced 1-KiB float4 instructions.  This is the one place on the path
// where LDS staging pays; the SoA state rows never need it.
__global__ __launch_bounds__(kStepBlock) void fpv_drone_step_aos_kernel(FPV_STEP_PARAMS)
{
    FPV_STEP_VIEW;
    constexpr int kPitch = 17;
    __shared__ float tile[kStepBlock / 64][64 * kPitch];
    FPV_STEP_INDEX;
    const bool live = i < n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    FpvStepOut o;
    o.done = false; o.reward = 0.0f; o.ax = o.ay = o.az = 0.0f;
    if (live) {
        FpvDroneState s;
        const float4 a = ld_action(B.action, i);
        ld_drone(B.state, B.ld, i, s);
        o = fpv_drone_step_lane<false>(K, s, a.x, a.y, a.z, a.w, B.wx, B.wy, B.wz);
        if (B.accel) {
            ST_OUT(row_at(ROW(B.accel, 0, B.ld), i), o.ax); ST_OUT(row_at(ROW(B.accel, 1, B.ld), i), o.ay); ST_OUT(row_at(ROW(B.accel, 2, B.ld), i), o.az);
        }
        if ((K.flags & FPV_FLAG_AUTO_RESET) && o.done) {
            fpv_drone_reset_lane(K, s);
            apply_reset_source(K, B, i, B.step, 0u, s);
        }
        st_drone(B.state, B.ld, i, s);
        float* row = &tile[wave][lane * kPitch];
        row[0] = s.px; row[1] = s.py; row[2] = s.pz; row[3] = s.vx; row[4] = s.vy; row[5] = s.vz;
        row[6] = s.q.w; row[7] = s.q.x; row[8] = s.q.y; row[9] = s.q.z; row[10] = s.rx; row[11] = s.ry; row[12] = s.rz;
        row[13] = o.ax; row[14] = o.ay; row[15] = o.az;
    }
    emit_outputs(B, i, live, o.reward, o.done);
    __syncthreads();
    const uint32_t wave_first = i - lane;                // first drone of this wave's tile
    float4* out = reinterpret_cast<float4*>(B.obs_aos) + (int64_t)wave_first * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f4 = j * 64 + lane;                    // float4 index inside the 64 x 16 tile
        const int d = f4 >> 2, c = (f4 & 3) * 4;
        if (wave_first + d < n) {
            const float* src = &tile[wave][d * kPitch + c];
            fpv_v4f v4;
            v4.x = src[0]; v4.y = src[1]; v4.z = src[2]; v4.w = src[3];
            __builtin_nontemporal_store(v4, reinterpret_cast<fpv_v4f*>(out) + f4);      // written once, read by the learner: streaming hint (ST_OUT)
        }
    }
}

// fp16-storage variant (BASELINE config 4): position rows fp32; the rest of a drone is ELEVEN 16-bit words, stored as
// FIVE rows of word pairs - (vx,vy) (vz,v_low) (qa,qb) (qc,rx) (ry,rz) - plus one row of single halves for prev_thrust:
// 3*4 + 5*4 + 2 = 34 state bytes each way, 89 algorithmic bytes per env-step instead of 133.  v, rates and
// thrust are binary16 (v with a 5-bit low word per component in v_low), q is smallest-three 15-bit fixed point: the
// encoding is fpv_pack_half / fpv_unpack_half (fpv_math.h).  One lane = one drone still moves nothing narrower than a dword
// (two-byte accesses waste the memory pipeline: with 11 separate half rows this kernel ran slower than
// the fp32 one): the even/odd lanes of a drone pair read the SAME dword of the thrust row, and on the
// way out the even lane fetches its neighbour's half with one DPP quad-permute and stores the dword.
// Arithmetic and the lane function are unchanged.
__device__ __forceinline__ const uint32_t* thrust_row_h(const FpvBufD& B)
{
    return reinterpret_cast<const uint32_t*>(B.thrust_h);      // follows the pair rows unless the caller placed it (a column partition)
}

__device__ __forceinline__ void ld_drone_h(const FpvBufD& B, uint32_t i, FpvDroneState& s)
{
    s.px = row_at(ROW(B.state, 0, B.ld), i); s.py = row_at(ROW(B.state, 1, B.ld), i); s.pz = row_at(ROW(B.state, 2, B.ld), i);
    const uint32_t* __restrict__ sh = reinterpret_cast<const uint32_t*>(B.state_h);
    FpvHalfState h;
#pragma unroll
    for (int k = 0; k < FPV_HALF_PAIR_ROWS; ++k) h.w[k] = row_at(ROW(sh, k, B.ld), i);
    const uint32_t tw = row_at(thrust_row_h(B), i >> 1);          // shared with the neighbour lane
    h.t = (uint16_t)((i & 1u) ? (tw >> 16) : tw);
    fpv_unpack_half(h, s);
}

// stores the position rows and the five pair words of an already packed state; the thrust half is the caller's
__device__ __forceinline__ void st_packed_h(const FpvBufD& B, uint32_t i, const FpvDroneState& s, const FpvHalfState& h)
{
    row_at(ROW(B.state, 0, B.ld), i) = s.px; row_at(ROW(B.state, 1, B.ld), i) = s.py; row_at(ROW(B.state, 2, B.ld), i) = s.pz;
    uint32_t* __restrict__ sh = reinterpret_cast<uint32_t*>(B.state_h);
#pragma unroll
    for (int k = 0; k < FPV_HALF_PAIR_ROWS; ++k) row_at(ROW(sh, k, B.ld), i) = h.w[k];
}

// packs and stores the position and pair rows; returns the new thrust half (the caller completes the pair).
// `id0` = low word of the global id of this shard's drone 0: the rounding stream of a drone is keyed by its GLOBAL id
// (like its stick-noise stream), so a drone's fp16 trajectory does not depend on the shard or lane it lands in.
__device__ __forceinline__ uint32_t st_drone_h(const FpvBufD& B, uint32_t i, uint32_t id0, uint32_t seed, const FpvDroneState& s)
{
    FpvHalfState h;
    fpv_pack_half(s, seed, id0 + (uint32_t)i, h);
    st_packed_h(B, i, s, h);
    return h.t;
}

// EVERY lane of the wave must call this (no early exit before it): lane 2j writes the dword that holds
// the thrust halves of drones 2j and 2j+1; a dead neighbour (odd n) contributes a zero half.
__device__ __forceinline__ void st_thrust_pair_h(const FpvBufD& B, uint32_t i, bool live, uint32_t my_half)
{
    const uint32_t mine = live ? my_half : 0u;
    const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, true);
    if (live && !(i & 1u)) row_at(const_cast<uint32_t*>(thrust_row_h(B)), i >> 1) = mine | (other << 16);
}

__global__ __launch_bounds__(kStepBlock) void fpv_drone_step_h_kernel(FPV_STEP_PARAMS)
{
    FPV_STEP_VIEW;
    FPV_STEP_INDEX;
    const bool live = i < n;                 // no early exit: the thrust-pair exchange needs whole lane pairs
    FpvStepOut o;
    o.done = false; o.reward = 0.0f; o.ax = o.ay = o.az = 0.0f;
    uint32_t th = 0;
    if (live) {
        FpvDroneState s;
        const float4 a = ld_action(B.action, i);
        ld_drone_h(B, i, s);
        __builtin_amdgcn_sched_barrier(0);       // loads first, constants after (see fpv_drone_step_kernel)
        o = fpv_drone_step_lane<false, true, false, false>(K, s, a.x, a.y, a.z, a.w, B.wx, B.wy, B.wz);
        if (B.accel) {
            ST_OUT(row_at(ROW(B.accel, 0, B.ld), i), o.ax); ST_OUT(row_at(ROW(B.accel, 1, B.ld), i), o.ay); ST_OUT(row_at(ROW(B.accel, 2, B.ld), i), o.az);
        }
        if ((K.flags & FPV_FLAG_AUTO_RESET) && o.done) fpv_drone_reset_lane(K, s);
        th = st_drone_h(B, i, K.noise.id_lo, fpv_round_seed(B.seed, B.step), s);
    }
    st_thrust_pair_h(B, i, live, th);
    emit_outputs(B, i, live, o.reward, o.done);
}

// k steps of the fp16-storage kernel in one launch: the state is rounded to binary16 and widened again
// after EVERY step, in registers, exactly as k single-step launches would do through HBM.  Sections and argument
// views as in fpv_drone_rollout_kernel.  No lane leaves early (the thrust-pair exchange needs whole lane pairs): the
// dead lanes of the last wave shadow the last drone - same loads, same arithmetic, uniform control flow - and store
// nothing.
__global__ __launch_bounds__(kStepBlock) void fpv_drone_rollout_h_kernel(const FpvRollArgs A)
{
    const uint32_t i0 = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    const bool live = i0 < A.n;
    const uint32_t i = live ? i0 : (uint32_t)(A.n - 1);
    FpvDroneState s;
    FpvHalfState h;
    ld_drone_h(A.B, i, s);
    float4 a_next = ld_action(A.B.action, i);
    const int k = A.R.k;
    fpv_settle(s.px); fpv_settle(s.py); fpv_settle(s.pz); fpv_settle(s.vx); fpv_settle(s.vy); fpv_settle(s.vz);
    fpv_settle(s.q.w); fpv_settle(s.q.x); fpv_settle(s.q.y); fpv_settle(s.q.z);
    fpv_settle(s.rx); fpv_settle(s.ry); fpv_settle(s.rz); fpv_settle(s.thrust);
    auto one_step = [&](const FpvRollArgs& V, const float* ap_next, bool prefetch, bool widen, int t, auto quiet_c) -> FpvStepOut {
        constexpr bool QUIET = decltype(quiet_c)::value;
        const float4 a = a_next;
        if (QUIET || prefetch) a_next = ld_action(reinterpret_cast<const float4*>(ap_next), i);
        FpvStepOut o = fpv_drone_step_lane<false, !QUIET, false, false>(V.K, s, a.x, a.y, a.z, a.w, V.B.wx, V.B.wy, V.B.wz);
        if ((V.K.flags & FPV_FLAG_AUTO_RESET) && o.done) {
            const FpvRollArgs& Z = fpv_args_again();
            fpv_drone_reset_lane(Z.K, s);
            apply_reset_source_k(i, (uint64_t)t, s);
        }
        const FpvRollArgs& PV = fpv_args_again();             // the rounding's three uniforms, read where they are used
        fpv_pack_half(s, fpv_round_seed(PV.B.seed, PV.B.step + (uint64_t)t), PV.K.noise.id_lo + (uint32_t)i, h);   // the HBM round trip of a single step, in registers
        if (QUIET || widen) fpv_unpack_half(h, s);
        return o;
    };
    int t = 0;
    if (A.B.ep_return == nullptr && A.R.out_stride == 0 && k > 1) {
        const float* ap = reinterpret_cast<const float*>(A.B.action);
        const int64_t astride = A.R.action_stride;
        unsigned long long* bp = A.R.bits_stride ? A.B.done_bits : nullptr;
        const int64_t bstride = A.R.bits_stride;
        auto quiet_step = [&]() {
            ap += astride;
            const FpvStepOut o = one_step(A, ap, true, true, t, std::true_type{});
            if (bp) {
                const unsigned long long mask = __ballot(live && o.done);
                // with 128-thread workgroups the LAST wave of the grid can be wholly dead (n % 128 in 1..64): its lane 0
                // owns no drone and no mask word - the word at i0 >> 6 would be the next row's first word
                if ((threadIdx.x & 63) == 0 && live) bp[i0 >> 6] = mask;
                bp += bstride;
            }
            ++t;
        };
        while (t + 1 < k - 1) { quiet_step(); quiet_step(); }        // two steps per trip (see fpv_drone_rollout_kernel)
        while (t < k - 1) quiet_step();
    }
    FpvStepOut o;
    o.done = false; o.reward = 0.0f; o.ax = o.ay = o.az = 0.0f;
    {
        const FpvRollArgs& G = fpv_args_again();
        RollOut out(G.B, G.R, i, true);
        if (out.bp) out.bp += (int64_t)t * G.R.bits_stride;
        const float* ap = reinterpret_cast<const float*>(G.B.action) + (int64_t)t * G.R.action_stride;
        const int kk = G.R.k;
        if (out.track) { fpv_settle(out.ep_r); fpv_settle(__int_as_float(out.ep_l)); }
        for (; t < kk; ++t) {
            ap += G.R.action_stride;
            o = one_step(G, ap, G.R.action_stride != 0 && t + 1 < kk, t + 1 < kk, t, std::false_type{});
            out.template step<false>(i0, t, o.reward, o.done, live);
        }
        // "does this lane own a drone" is a compare, not something to carry across the loop in an SGPR pair (the one
        // value this kernel used to spill): ask again, through an opaque copy of the index
        uint32_t jf = i0;
        asm volatile("" : "+v"(jf));
        if ((int64_t)jf < G.n) out.finish(jf, fpv_args_again().B);
    }
    const FpvRollArgs& E = fpv_args_again();
    uint32_t j = i0;                             // form the store addresses after the loops (VGPR pressure)
    asm volatile("" : "+v"(j));
    const bool live_e = (int64_t)j < E.n;
    if (live_e) {
        if (E.B.accel) {
            ST_OUT(row_at(ROW(E.B.accel, 0, E.B.ld), j), o.ax); ST_OUT(row_at(ROW(E.B.accel, 1, E.B.ld), j), o.ay); ST_OUT(row_at(ROW(E.B.accel, 2, E.B.ld), j), o.az);
        }
        st_packed_h(E.B, j, s, h);
    }
    st_thrust_pair_h(E.B, j, live_e, h.t);
}

template <bool WIDE, bool PIDV>
__device__ __forceinline__ void ld_racer(const float* __restrict__ st, int64_t ld, uint32_t i, FpvRacerState& s)
{
    s.px = row_at(ROW(st, FPV_PX, ld), i); s.py = row_at(ROW(st, FPV_PY, ld), i); s.pz = row_at(ROW(st, FPV_PZ, ld), i);
    s.vx = row_at(ROW(st, FPV_VX, ld), i); s.vy = row_at(ROW(st, FPV_VY, ld), i); s.vz = row_at(ROW(st, FPV_VZ, ld), i);
    s.q.w = row_at(ROW(st, FPV_QW, ld), i); s.q.x = row_at(ROW(st, FPV_QX, ld), i); s.q.y = row_at(ROW(st, FPV_QY, ld), i); s.q.z = row_at(ROW(st, FPV_QZ, ld), i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.w[k] = row_at(ROW(st, (FPV_R_OMEGA + k), ld), i);
        s.ierr[k] = row_at(ROW(st, (FPV_R_IERR + k), ld), i);
        s.lerr[k] = row_at(ROW(st, (FPV_R_LERR + k), ld), i);
        s.wlo[k] = WIDE ? row_at(ROW(st, (FPV_R_OMEGA_LO + k), ld), i) : 0.0f;
        s.ilo[k] = WIDE ? row_at(ROW(st, (FPV_R_IERR_LO + k), ld), i) : 0.0f;
        s.dflt[k] = PIDV ? row_at(ROW(st, (FPV_R_DFILT + k), ld), i) : 0.0f;
    }
    s.first = row_at(ROW(st, FPV_R_FIRST, ld), i);
}

template <bool WIDE, bool PIDV>
__device__ __forceinline__ void st_racer(float* __restrict__ st, int64_t ld, uint32_t i, const FpvRacerState& s)
{
    row_at(ROW(st, FPV_PX, ld), i) = s.px; row_at(ROW(st, FPV_PY, ld), i) = s.py; row_at(ROW(st, FPV_PZ, ld), i) = s.pz;
    row_at(ROW(st, FPV_VX, ld), i) = s.vx; row_at(ROW(st, FPV_VY, ld), i) = s.vy; row_at(ROW(st, FPV_VZ, ld), i) = s.vz;
    row_at(ROW(st, FPV_QW, ld), i) = s.q.w; row_at(ROW(st, FPV_QX, ld), i) = s.q.x; row_at(ROW(st, FPV_QY, ld), i) = s.q.y; row_at(ROW(st, FPV_QZ, ld), i) = s.q.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        row_at(ROW(st, (FPV_R_OMEGA + k), ld), i) = s.w[k];
        row_at(ROW(st, (FPV_R_IERR + k), ld), i) = s.ierr[k];
        row_at(ROW(st, (FPV_R_LERR + k), ld), i) = s.lerr[k];
        if (WIDE) { row_at(ROW(st, (FPV_R_OMEGA_LO + k), ld), i) = s.wlo[k]; row_at(ROW(st, (FPV_R_IERR_LO + k), ld), i) = s.ilo[k]; }
        if (PIDV) row_at(ROW(st, (FPV_R_DFILT + k), ld), i) = s.dflt[k];
    }
    row_at(ROW(st, FPV_R_FIRST, ld), i) = s.first;
}

// Racer.step.  WIDE = as written (omega radians per step: float64 rate loop, six extra (hi, lo) rows);
// PIDV = components.PID semantics (three extra rows).  The 181-byte variant (neither) is the
// racer_omega_dt one.
template <bool WIDE, bool PIDV>
__global__ __launch_bounds__(kStepBlock) void fpv_racer_step_kernel(FPV_STEP_PARAMS)
{
    FPV_STEP_VIEW;
    FPV_STEP_INDEX;
    if (i >= n) return;
    FpvRacerState s;
    const float4 a = ld_action(B.action, i);
    ld_racer<WIDE, PIDV>(B.state, B.ld, i, s);
    __builtin_amdgcn_sched_barrier(0);
    const float reward = fpv_racer_step_lane<WIDE, PIDV ? 1 : 0>(K, s, a.x, a.y, a.z, a.w);
    const bool done = !(fabsf(s.pz) <= K.ceiling);            // the Racer has no ground; build-defined ceiling only
    if ((K.flags & FPV_FLAG_AUTO_RESET) && done) fpv_racer_reset_lane(s);
    st_racer<WIDE, PIDV>(B.state, B.ld, i, s);
    emit_outputs(B, i, true, reward, done);
}

// k steps of Racer.step in one launch; the three sections and their argument views are those of fpv_drone_rollout_kernel
// (the as-written variant alone carries 45 double-precision uniforms: through one view they could not all stay in SGPRs
// across the loop together with the pointers of the outputs and the final stores - 75-87 spilled SGPRs in round 2).
template <bool WIDE, bool PIDV>
__global__ __launch_bounds__(kStepBlock) void fpv_racer_rollout_kernel(const FpvRollArgs A)
{
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    FpvRacerState s;
    ld_racer<WIDE, PIDV>(A.B.state, A.B.ld, i, s);
    float4 a_next = ld_action(A.B.action, i);
    const int k = A.R.k;
    fpv_settle(s.px); fpv_settle(s.py); fpv_settle(s.pz); fpv_settle(s.vx); fpv_settle(s.vy); fpv_settle(s.vz);
    fpv_settle(s.q.w); fpv_settle(s.q.x); fpv_settle(s.q.y); fpv_settle(s.q.z); fpv_settle(s.first);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        fpv_settle(s.w[c]); fpv_settle(s.ierr[c]); fpv_settle(s.lerr[c]);
        if (WIDE) { fpv_settle(s.wlo[c]); fpv_settle(s.ilo[c]); }
        if (PIDV) fpv_settle(s.dflt[c]);
    }
    float reward = 0.0f;
    bool done = false;
    auto one_step = [&](const FpvRollArgs& V, const float* ap_next, bool prefetch, auto quiet_c) {
        constexpr bool QUIET = decltype(quiet_c)::value;
        const float4 a = a_next;
        if (QUIET || prefetch) a_next = ld_action(reinterpret_cast<const float4*>(ap_next), i);
        reward = fpv_racer_step_lane<WIDE, PIDV ? 1 : 0, !QUIET, WIDE && !QUIET>(V.K, s, a.x, a.y, a.z, a.w);    // per-axis views where outputs compete for SGPRs
        done = !(fabsf(s.pz) <= V.K.ceiling);              // the Racer has no ground; build-defined ceiling only
        if ((V.K.flags & FPV_FLAG_AUTO_RESET) && done) fpv_racer_reset_lane(s);
    };
    int t = 0;
    if (A.B.ep_return == nullptr && A.R.out_stride == 0 && k > 1) {
        const float* ap = reinterpret_cast<const float*>(A.B.action);
        const int64_t astride = A.R.action_stride;
        unsigned long long* bp = A.R.bits_stride ? A.B.done_bits : nullptr;
        const int64_t bstride = A.R.bits_stride;
        auto quiet_step = [&]() {
            ap += astride;
            one_step(A, ap, true, std::true_type{});
            if (bp) {
                const unsigned long long mask = __ballot(done);
                if ((threadIdx.x & 63) == 0) bp[i >> 6] = mask;
                bp += bstride;
            }
            ++t;
        };
        while (t + 1 < k - 1) { quiet_step(); quiet_step(); }        // two steps per trip (see fpv_drone_rollout_kernel)
        while (t < k - 1) quiet_step();
    }
    {
        const FpvRollArgs& G = fpv_args_again();
        RollOut out(G.B, G.R, i, true);
        if (out.bp) out.bp += (int64_t)t * G.R.bits_stride;
        const float* ap = reinterpret_cast<const float*>(G.B.action) + (int64_t)t * G.R.action_stride;
        const int kk = G.R.k;
        if (out.track) { fpv_settle(out.ep_r); fpv_settle(__int_as_float(out.ep_l)); }
        for (; t < kk; ++t) {
            ap += G.R.action_stride;
            one_step(G, ap, G.R.action_stride != 0 && t + 1 < kk, std::false_type{});
            out.template step<false>(i, t, reward, done);
        }
        out.finish(i, fpv_args_again().B);
    }
    const FpvRollArgs& E = fpv_args_again();
    uint32_t j = i;                                  // form the store addresses after the loops (VGPR pressure)
    asm volatile("" : "+v"(j));
    st_racer<WIDE, PIDV>(E.B.state, E.B.ld, j, s);
}

// Drone.reset (components.py:150-169): p, v, R = E(deg2rad(ypr)) with the triple consumed as
// (roll, pitch, yaw); prev_rates = 0, prev_thrust = 0, done = False.  Racer.reset: zeros + identity.
__global__ __launch_bounds__(kBlock) void fpv_reset_kernel(const FpvK K, const FpvBufD B, const int mode,
                                                           const uint8_t* __restrict__ mask,
                                                           const float* __restrict__ pos,
                                                           const float* __restrict__ vel,
                                                           const float* __restrict__ ypr, const int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    if (mode == FPV_MODE_DRONE) {
        FpvDroneState s;
        fpv_drone_reset_lane(K, s);
        float* tab = const_cast<float*>(B.reset_pose);
        if (tab) {      // the lane's own start (fpv_abi.h "Reset sources"): its table row, replaced where arguments are given
            s.px = tab[0 * B.ld + i]; s.py = tab[1 * B.ld + i]; s.pz = tab[2 * B.ld + i];
            s.vx = tab[3 * B.ld + i]; s.vy = tab[4 * B.ld + i]; s.vz = tab[5 * B.ld + i];
            s.q.w = tab[6 * B.ld + i]; s.q.x = tab[7 * B.ld + i]; s.q.y = tab[8 * B.ld + i]; s.q.z = tab[9 * B.ld + i];
        }
        if (pos) { s.px = pos[3 * i]; s.py = pos[3 * i + 1]; s.pz = pos[3 * i + 2]; }
        if (vel) { s.vx = vel[3 * i]; s.vy = vel[3 * i + 1]; s.vz = vel[3 * i + 2]; }
        if (ypr) s.q = fpv_quat_from_rpy_deg(ypr[3 * i], ypr[3 * i + 1], ypr[3 * i + 2]);
        if (tab && (pos || vel || ypr)) {
            tab[0 * B.ld + i] = s.px; tab[1 * B.ld + i] = s.py; tab[2 * B.ld + i] = s.pz;
            tab[3 * B.ld + i] = s.vx; tab[4 * B.ld + i] = s.vy; tab[5 * B.ld + i] = s.vz;
            tab[6 * B.ld + i] = s.q.w; tab[7 * B.ld + i] = s.q.x; tab[8 * B.ld + i] = s.q.y; tab[9 * B.ld + i] = s.q.z;
        }
        if (K.flags & FPV_FLAG_RESET_JITTER) {
            float pose[10] = {s.px, s.py, s.pz, s.vx, s.vy, s.vz, s.q.w, s.q.x, s.q.y, s.q.z};
            fpv_reset_jitter(B.rj, (((uint64_t)K.noise.id_hi << 32) | K.noise.id_lo) + (uint64_t)i, B.step, 1u, pose);
            s.px = pose[0]; s.py = pose[1]; s.pz = pose[2]; s.vx = pose[3]; s.vy = pose[4]; s.vz = pose[5];
            s.q.w = pose[6]; s.q.x = pose[7]; s.q.y = pose[8]; s.q.z = pose[9];
        }
        if (K.flags & FPV_FLAG_FP16_STATE) {
            // masked lanes are independent here, so the thrust half goes out as a 2-byte store (not a hot path)
            const uint32_t th = st_drone_h(B, (uint32_t)i, K.noise.id_lo, B.seed, s);
            reinterpret_cast<uint16_t*>(const_cast<uint32_t*>(thrust_row_h(B)))[i] = (uint16_t)th;
        } else {
            st_drone(B.state, B.ld, i, s);
        }
    } else {
        FpvRacerState s;
        fpv_racer_reset_lane(s);
        st_racer<true, true>(B.state, B.ld, i, s);          // all 29 rows, whatever the variant uses
    }
    if (B.done) B.done[i] = 0;
    if (B.ep_return) { B.ep_return[i] = 0.0f; B.ep_length[i] = 0; }
    if (B.noise_state) {
#pragma unroll
        for (int k = 0; k < 4; ++k) row_at(ROW(B.noise_state, k, B.ld), i) = 0.0f;      // x_s(0) = 0
    }
    if (B.pos_comp) {
#pragma unroll
        for (int k = 0; k < 6; ++k) row_at(ROW(B.pos_comp, k, B.ld), i) = 0.0f;
    }
}

// The return value of Drone.step for every drone (components.py:247-248): rotation_matrix.T and the "angular velocity
// matrix" E(rates) as [n][3][3] row-major, R_new @ acceleration as [n][3] (copied from the step kernel's accel rows).
// One lane per drone; the outputs are what a caller of the reference's API reads on the host side of the boundary
// (36-byte lane stride: a convenience path, not the hot one - the zero-copy SoA state is the observation).
__global__ __launch_bounds__(kBlock) void fpv_return_triple_kernel(const float* __restrict__ st, const int64_t ld,
                                                                   const float* __restrict__ accel, float* __restrict__ rt,
                                                                   float* __restrict__ gyro, float* __restrict__ acc, const int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    FpvQuat q;
    q.w = st[FPV_QW * ld + i]; q.x = st[FPV_QX * ld + i]; q.y = st[FPV_QY * ld + i]; q.z = st[FPV_QZ * ld + i];
    float a[9], g[9];
    fpv_return_matrices(q, st[FPV_RX * ld + i], st[FPV_RY * ld + i], st[FPV_RZ * ld + i], a, g);
#pragma unroll
    for (int k = 0; k < 9; ++k) { rt[9 * i + k] = a[k]; gyro[9 * i + k] = g[k]; }
    if (acc) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[3 * i + k] = accel[(int64_t)k * ld + i];
    }
}

// fp16 state storage -> the 14 fp32 rows of the state (fpv_abi.h row numbering) for whoever reads the state on the host
// side of the boundary (an observation, a log): the position rows copied, the eleven 16-bit words decoded exactly as the
// step kernel decodes them (fpv_unpack_half: v with its low words, q rebuilt from its three stored components).  One
// launch instead of a dozen tensor operations.
__global__ __launch_bounds__(kBlock) void fpv_widen_state_kernel(const float* __restrict__ pos, const uint16_t* __restrict__ sh16,
                                                                 const uint16_t* __restrict__ thrust16, const int64_t ld,
                                                                 float* __restrict__ out, const int64_t out_ld, const int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t* __restrict__ sh = reinterpret_cast<const uint32_t*>(sh16);
    FpvHalfState h;
#pragma unroll
    for (int k = 0; k < FPV_HALF_PAIR_ROWS; ++k) h.w[k] = sh[(int64_t)k * ld + i];
    h.t = thrust16[i];
    FpvDroneState s;
    fpv_unpack_half(h, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(int64_t)k * out_ld + i] = pos[(int64_t)k * ld + i];
    const float v[11] = {s.vx, s.vy, s.vz, s.q.w, s.q.x, s.q.y, s.q.z, s.rx, s.ry, s.rz, s.thrust};
#pragma unroll
    for (int k = 0; k < 11; ++k) out[(int64_t)(3 + k) * out_ld + i] = v[k];
}

// components.PID.__call__ for n drones (components.py:43-54): one lane per drone, four state rows.
__global__ __launch_bounds__(kBlock) void fpv_pid_kernel(const FpvPidK<float> P, float* __restrict__ st, const int64_t ld,
                                                         const int64_t n, const float* __restrict__ current,
                                                         const float* __restrict__ target, const float target_scalar,
                                                         float* __restrict__ out, float* __restrict__ error_out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float integ = st[FPV_PID_INTEGRAL * ld + i], dflt = st[FPV_PID_PREV_DERIVATIVE * ld + i];
    float last = st[FPV_PID_PREV_ERROR * ld + i];
    const bool first = st[FPV_PID_IS_FIRST * ld + i] != 0.0f;
    const float cur = current[i], tgt = target ? target[i] : target_scalar;
    out[i] = fpv_pid_axis<float, 1>(P, 0, cur, tgt, first, integ, last, dflt);
    if (error_out) error_out[i] = last;                                   // PID.error == previous_error after the call
    st[FPV_PID_INTEGRAL * ld + i] = integ; st[FPV_PID_PREV_DERIVATIVE * ld + i] = dflt;
    st[FPV_PID_PREV_ERROR * ld + i] = last; st[FPV_PID_IS_FIRST * ld + i] = 0.0f;
}

__global__ __launch_bounds__(kBlock) void fpv_pid_reset_kernel(float* __restrict__ st, const int64_t ld, const int64_t n,
                                                               const uint8_t* __restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (mask && !mask[i])) return;
    st[FPV_PID_INTEGRAL * ld + i] = 0.0f; st[FPV_PID_PREV_DERIVATIVE * ld + i] = 0.0f;
    st[FPV_PID_PREV_ERROR * ld + i] = 0.0f; st[FPV_PID_IS_FIRST * ld + i] = 1.0f;
}

// Counter calibration: a copy with the step kernel's access shape (one dword per lane per
// instruction, 256 contiguous bytes per wave) and an exactly known byte count, so FETCH_SIZE /
// WRITE_SIZE read under rocprofv3 can be scaled (MI355X_MICROARCH.md, HBM section).
__global__ __launch_bounds__(kBlock) void fpv_diag_copy_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                               const int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// The same copy with 16 bytes per lane: the chip's streaming ceiling on this box (the guide's "achievable HBM" figure is
// a float4 copy), timed by bench.py next to the step kernel at 2^23 drones.
__global__ __launch_bounds__(kBlock) void fpv_diag_copy4_kernel(fpv_v4f* __restrict__ dst, const fpv_v4f* __restrict__ src,
                                                                const int64_t n4)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n4) dst[i] = src[i];
}

// A wave that idles for `ticks` of the constant-rate wall clock, at most `max_iter` sleeps (an exit every lane reaches
// whatever the clock does): a kernel of known duration on one CU (fpv_diag_busy).
__global__ __launch_bounds__(64) void fpv_diag_busy_kernel(const unsigned long long ticks, const int max_iter)
{
    const unsigned long long t0 = wall_clock64();
    for (int it = 0; it < max_iter; ++it) {
        if (wall_clock64() - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(32);
    }
}

// Which XCD runs which workgroup: every workgroup writes the XCC_ID hardware register of the XCD it landed on (fpv_diag_xcd_map).
// The launch geometry is the step kernels' (kStepBlock threads), so what the probe sees is what a step launch of the same grid gets.
__global__ __launch_bounds__(kStepBlock) void fpv_diag_xcd_kernel(uint32_t* __restrict__ out)
{
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    if (threadIdx.x == 0) out[blockIdx.x] = x & 0xfu;
}

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what)
{
    return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? FPV_ENODEV : FPV_EHIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

// workgroups of `block` threads, one thread per item, for n items
inline dim3 blocks_for(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

template <class T> struct exactly { typedef T type; };      // a parameter type that takes no part in template deduction

// One kernel launch and its check: FPV_OK, or the launch's error under `what`.  The arguments take the kernel's own parameter
// types (P is deduced from the kernel alone), so every argument converts as it would in a direct call.
template <class... P>
int launch(const char* what, void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, const typename exactly<P>::type&... args)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPV_OK : hip_fail(e, what);
}

// The same for a kernel known by its address, with its arguments as the list of pointers that a graph node takes.
int launch_args(const char* what, void* kernel, dim3 grid, dim3 block, hipStream_t s, void** args)
{
    (void)hipLaunchKernel(kernel, grid, block, args, 0, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPV_OK : hip_fail(e, what);
}

}  // namespace

struct fpv_env {
    FpvK K;
    fpv_params_t P;
    int64_t n;
    int device;
    int mode;
    FpvResetJitter rj;   // FPV_FLAG_RESET_JITTER constants (fpv_derive_reset_jitter), copied into every launch's FpvBufD
    uint64_t launches;   // 64-bit step index: counts the steps launched so far; keys the stick-noise stream (Philox
                         // counter words 2 and 3) and the stochastic rounding (fpv_round_seed)
    // rotation of the single-step kernels' start block (FPV_STEP_INDEX): blocks the start moves back per launch
    // (0 = plain order), where the next launch starts, and what the caller asked for (fpv_set_rotation: -1 = automatic)
    int64_t rot_blocks = 0, start_block = 0, rot_request = -1;
    // what the device said about itself at fpv_create, held against the cache model the rotation and the row stride are built on
    // (device_cache_model): a device that is not the one the model was measured on gets the plain order
    fpv_cache_model_t cache;
    // cached hipGraph of the last fpv_rollout_graph call (launch-bound small batches): rebuilt when the
    // SHAPE key changes, re-pointed node by node when only buffer addresses change
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    std::vector<hipGraphNode_t> graph_nodes;
    std::string graph_shape_key, graph_ptr_key;
    // per-drone physics (fpv_set_physics): the caller's table [FPV_PHYS_ROWS][phys_ld] or null, and the rows the last launch loaded
    const float* phys = nullptr;
    int64_t phys_ld = 0;
    int phys_rows_last = 0;
    // a gate course (fpv_set_gates): what the kernels of csrc/fpv_gate.hip read, copied from the caller's struct
    bool gates = false;
    FpvGateArgs ga = {};
};

// The kernels of csrc/fpv_phys.hip, by instantiation: weak, so that this file ALONE still links into a loadable library that
// exports every declared symbol (the sanitizer builds and the ISA tools compile this one file) - there both are null and
// fpv_set_physics says so.  The single-step kernels take FPV_STEP_PARAMS with the table base in the state_h slot and the
// "load the ground rows" bit in n_start (kPhysGroundBit); the k-step kernels take one FpvRollPhysArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_phys_step_kernel(int noise, int obj);
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_phys_roll_kernel(int noise, int obj);
// The kernels of csrc/fpv_gate.hip, weak in the same way (fpv_set_gates says so when they are absent).  The single-step kernel
// takes FPV_STEP_PARAMS with the word base in the state_h slot and one FpvGateArgs after them, the k-step kernels ([stick noise]
// [object list]; the two together have none) one FpvRollGateArgs, the word reset (word, mask, start gates, count, n).
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_gate_step_kernel(void);
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_gate_roll_kernel(int noise, int obj);
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_gate_reset_kernel_fn(void);
// The kernel of csrc/fpv_range.hip, weak in the same way (fpv_range_scan says so when it is absent): one FpvRangeArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_range_scan_kernel_fn(void);
// The kernels of csrc/fpv_depth.hip (one per encoding), weak in the same way (fpv_depth_render says so when they are absent): one
// FpvDepthArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_depth_render_kernel_fn(int u8);
// The kernels of csrc/fpv_chase.hip (with and without a supplied pixel) and its host loop, weak in the same way (fpv_chase_guide and
// fpv_chase_eval say so when they are absent): one FpvChaseArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_chase_kernel_fn(int pixel);
extern "C" __attribute__((weak, visibility("hidden"))) void fpv_chase_eval_host(const FpvChaseArgs* A, const float* p, const float* v, const float* q);
// The kernels of csrc/fpv_pns.hip (with and without a supplied pixel) and its host loop, weak in the same way: one FpvPnsArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_pns_kernel_fn(int pixel);
extern "C" __attribute__((weak, visibility("hidden"))) void fpv_pns_eval_host(const FpvPnsArgs* A, const float* p, const float* v, const float* q);
// The kernels of csrc/fpv_detect.hip (with and without the own-target slot) and its host loop, weak in the same way: one FpvDetectArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_detect_kernel_fn(int own);
extern "C" __attribute__((weak, visibility("hidden"))) void fpv_detect_eval_host(const FpvDetectArgs* A, const float* p, const float* q);
// The kernel of csrc/fpv_splat.hip and its host loop, weak in the same way: one FpvSplatArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_splat_kernel_fn(void);
extern "C" __attribute__((weak, visibility("hidden"))) void fpv_splat_eval_host(const FpvSplatArgs* A, const float* p, const float* q);
// The kernels of csrc/fpv_pursuit.hip ([guidance law][reset call]) and its host loop, weak in the same way (fpv_pursuit_step, _reset
// and _eval say so when they are absent): one FpvPursuitArgs.
extern "C" __attribute__((weak, visibility("hidden"))) void* fpv_pursuit_kernel_fn(int guide, int reset);
extern "C" __attribute__((weak, visibility("hidden"))) void fpv_pursuit_eval_host(const FpvPursuitArgs* A, const float* p, const float* v, const float* q,
                                                                                  int guide, int reset);

namespace {

// the kernel families a call is served by (plan_launch)
enum Family { kPlain, kFp16, kAos, kRacer, kTable, kGate };

// What a physics table (kTable) and a gate course (kGate) cannot be combined with - what their kernels do not carry, refused by
// name.  b null: the handle, asked when the feature is bound (fpv_set_physics, fpv_set_gates); else the buffers of a call
// (check_buffers).  A handle that has the other feature bound is a fp32 drone handle, so the order of the handle's three cannot show.
int check_combination(const fpv_env* h, Family f, const fpv_buffers_t* b)
{
    struct Rule { bool hit; const char* with; };
    const bool table = f == kTable;
    const auto refuse = [&](std::initializer_list<Rule> rules) -> int {
        for (const Rule& r : rules)
            if (r.hit) return fail(FPV_EINVAL, std::string(table ? "a physics table" : "a gate course") + " cannot be combined with " + r.with);
        return FPV_OK;
    };
    if (!b)
        return refuse({{h->mode != FPV_MODE_DRONE, "Racer mode"}, {(h->K.flags & FPV_FLAG_FP16_STATE) != 0, "fp16 state (FPV_FLAG_FP16_STATE)"},
                       table ? Rule{h->gates, "a gate course (fpv_set_gates)"} : Rule{h->phys != nullptr, "a physics table (fpv_set_physics)"}});
    return refuse({{b->pos_comp != nullptr, "Kahan rows (pos_comp)"}, {b->rotation_override != nullptr, "the guidance override (rotation_override)"},
                   {b->obs_aos != nullptr, "the AoS head (obs_aos)"},
                   {!table && (h->K.flags & FPV_FLAG_STICK_NOISE) && b->objects && b->objects->count > 0, "stick noise AND an object list (either one alone is served)"}});
}

// THE intake of an object list - the step's, a scan's, a render's - in three parts (check_buffers asks what the handle can serve
// between the first two): the count (`most`: a sensor's refusal also says how many there may be), the types, and the rows of a
// list that passed both in the kernels' form (*T comes zeroed; `has_ground`, `lo`, `hi` are the step's: fpv_objects_bounds).
int check_object_count(const fpv_objects_t* in, bool most)
{
    if (in && (in->count < 0 || in->count > FPV_MAX_OBJECTS))
        return fail(FPV_EINVAL, "objects.count out of range" + (most ? " (at most " + std::to_string(FPV_MAX_OBJECTS) + " objects)" : std::string()));
    return FPV_OK;
}

int check_object_types(const fpv_objects_t* in)
{
    for (int k = 0; in && k < in->count; ++k)
        if (in->obj[k].type < FPV_OBJ_GROUND || in->obj[k].type > FPV_OBJ_SPHERE) return fail(FPV_EINVAL, "unknown object type");
    return FPV_OK;
}

void copy_objects(const fpv_objects_t* in, FpvObjects* T)
{
    if (!in) return;
    T->count = in->count;
    for (int k = 0; k < T->count; ++k) {
        const fpv_object_t& o = in->obj[k];
        T->o[k].type = o.type; T->o[k].x = o.x; T->o[k].y = o.y; T->o[k].z = o.z; T->o[k].radius = o.radius; T->o[k].height = o.height;
    }
}

// What a scan and a render ask first, `sensor` named in the refusals: of the build (`kernel`: the weak lookup function of
// csrc/`unit`.hip was linked - what a build without it answers to any call), then of the handle and the buffers.
int check_sensor(const fpv_env* h, const fpv_buffers_t* b, const void* s, bool kernel, const std::string& sensor, const char* unit)
{
    if (!kernel) return fail(FPV_EINVAL, "the " + sensor + " is not in this build (the library was linked without csrc/" + unit + ".hip)");
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (!b || !s) return fail(FPV_EINVAL, "null argument");
    if (h->K.flags & FPV_FLAG_FP16_STATE)
        return fail(FPV_EINVAL, "the " + sensor + " cannot read fp16 state (FPV_FLAG_FP16_STATE): a reader of the packed quaternion is the follow-up");
    if (!b->state) return fail(FPV_EINVAL, "fpv_buffers_t.state is null");
    if (b->ld < h->n) return fail(FPV_EALIGN, "fpv_buffers_t.ld is smaller than the number of drones");
    return FPV_OK;
}

// What fpv_range_eval and fpv_depth_eval ask of their arguments first, and pose i of q [n][4] (wxyz)
int check_eval_args(const void* s, int64_t n, const float* p, const float* q)
{
    if (!s || !p || !q) return fail(FPV_EINVAL, "null argument");
    if (n <= 0) return fail(FPV_EINVAL, "n must be positive");
    return FPV_OK;
}

FpvQuat pose_quat(const float* q, int64_t i)
{
    FpvQuat a; a.w = q[4 * i]; a.x = q[4 * i + 1]; a.y = q[4 * i + 2]; a.z = q[4 * i + 3];
    return a;
}

int check_buffers(const fpv_env* h, const fpv_buffers_t* b, bool need_action)  // NOLINT
{
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (!b) return fail(FPV_EINVAL, "null fpv_buffers_t");
    if (!b->state) return fail(FPV_EINVAL, "fpv_buffers_t.state is null");
    const bool noise = (h->K.flags & FPV_FLAG_STICK_NOISE) != 0;
    if (need_action && !b->action && !noise) return fail(FPV_EINVAL, "fpv_buffers_t.action is null");
    if (noise) {
        if (!b->noise_state) return fail(FPV_EINVAL, "FPV_FLAG_STICK_NOISE needs fpv_buffers_t.noise_state");
        if (b->obs_aos) return fail(FPV_EINVAL, "obs_aos and FPV_FLAG_STICK_NOISE cannot be combined");
    }
    if ((uintptr_t)b->action_out & 15) return fail(FPV_EALIGN, "action_out must be 16-byte aligned");
    if (b->action_ld) {
        if (b->action_ld < h->n) return fail(FPV_EALIGN, "action_ld must be >= n");   // dword loads: no alignment rule
        if (h->mode != FPV_MODE_DRONE || (h->K.flags & FPV_FLAG_FP16_STATE) || b->obs_aos)
            return fail(FPV_EINVAL, "SoA actions (action_ld) are supported by the fp32 drone kernel without obs_aos");
    }
    if (b->ld < h->n) return fail(FPV_EALIGN, "fpv_buffers_t.ld is smaller than the number of drones");
    if (b->ld % 4) return fail(FPV_EALIGN, "fpv_buffers_t.ld must be a multiple of 4 floats");
    if (((uintptr_t)b->state & 15) || ((uintptr_t)b->action & 15))
        return fail(FPV_EALIGN, "state and action must be 16-byte aligned");
    if ((uintptr_t)b->done_bits & 7) return fail(FPV_EALIGN, "done_bits must be 8-byte aligned");
    if (b->done_bits_stride && (b->done_bits_stride < (h->n + 63) / 64))
        return fail(FPV_EALIGN, "done_bits_stride must be 0 or >= ceil(n / 64) words");
    if (b->objects && b->objects->count != 0) {
        int rc = check_object_count(b->objects, false);
        if (rc != FPV_OK) return rc;
        if (h->mode != FPV_MODE_DRONE || (h->K.flags & (FPV_FLAG_FP16_STATE | FPV_FLAG_GROUND)) || b->obs_aos)
            return fail(FPV_EINVAL, "objects need drone mode with fp32 state and cannot be combined with "
                                    "FPV_FLAG_GROUND (use a Ground entry) or obs_aos");
        rc = check_object_types(b->objects);
        if (rc != FPV_OK) return rc;
    }
    if (b->pos_comp) {
        if (h->mode != FPV_MODE_DRONE || (h->K.flags & FPV_FLAG_FP16_STATE) || b->obs_aos)
            return fail(FPV_EINVAL, "pos_comp needs drone mode with fp32 state and cannot be combined with obs_aos");
        if ((uintptr_t)b->pos_comp & 15) return fail(FPV_EALIGN, "pos_comp must be 16-byte aligned");
    }
    if (b->obs_aos) {
        if (h->mode != FPV_MODE_DRONE || (h->K.flags & FPV_FLAG_FP16_STATE))
            return fail(FPV_EINVAL, "obs_aos is available in drone mode with fp32 state only");
        if ((uintptr_t)b->obs_aos & 15) return fail(FPV_EALIGN, "obs_aos must be 16-byte aligned");
    }
    if (h->K.flags & FPV_FLAG_FP16_STATE) {
        if (!b->state_h) return fail(FPV_EINVAL, "FPV_FLAG_FP16_STATE needs fpv_buffers_t.state_h");
        if ((uintptr_t)b->state_h & 7) return fail(FPV_EALIGN, "state_h must be 8-byte aligned");
        if ((uintptr_t)b->state_h_thrust & 3) return fail(FPV_EALIGN, "state_h_thrust must be 4-byte aligned (a column range starts at an even drone)");
    }
    if ((b->rotation_override == nullptr) != (b->thrust_override == nullptr))
        return fail(FPV_EINVAL, "rotation_override and thrust_override must be given together (Drone.step: thrust_force is only "
                                "used with rotation_matrix, components.py:230-232)");
    if (b->rotation_override) {
        if (h->mode != FPV_MODE_DRONE || (h->K.flags & (FPV_FLAG_FP16_STATE | FPV_FLAG_STICK_NOISE)) || b->obs_aos || b->pos_comp)
            return fail(FPV_EINVAL, "the guidance override needs drone mode with fp32 state, caller-supplied sticks, and no "
                                    "obs_aos / pos_comp (objects and FPV_FLAG_GROUND are fine)");
        if (((uintptr_t)b->rotation_override & 3) || ((uintptr_t)b->thrust_override & 3))
            return fail(FPV_EALIGN, "rotation_override / thrust_override must be 4-byte aligned");
    }
    if (b->reset_pose || (h->K.flags & FPV_FLAG_RESET_JITTER)) {
        if (h->mode != FPV_MODE_DRONE) return fail(FPV_EINVAL, "reset sources (reset_pose, FPV_FLAG_RESET_JITTER) are drone-mode only");
        if (b->rotation_override) return fail(FPV_EINVAL, "the guidance override cannot be combined with a reset source (reset_pose / FPV_FLAG_RESET_JITTER)");
        if ((uintptr_t)b->reset_pose & 15) return fail(FPV_EALIGN, "reset_pose must be 16-byte aligned");
        if (b->reset_pose && b->ld < h->n) return fail(FPV_EALIGN, "fpv_buffers_t.ld is smaller than the number of drones");
    }
    if (h->phys || h->gates) {
        const int rc = check_combination(h, h->phys ? kTable : kGate, b);
        if (rc != FPV_OK) return rc;
        if (h->phys && b->ld != h->phys_ld) return fail(FPV_EALIGN, "the physics table's row stride must be the state's (fpv_buffers_t.ld)");
    }
    if ((b->ep_return == nullptr) != (b->ep_length == nullptr))
        return fail(FPV_EINVAL, "ep_return and ep_length must be given together");
    if ((b->last_return || b->last_length) && !b->ep_return)
        return fail(FPV_EINVAL, "last_return/last_length need ep_return/ep_length");
    return FPV_OK;
}

// the bounds of the object list are grown by the handle's K.contact_reach (fpv_objects_bounds)
FpvBufD to_device_view(const fpv_env* h, const fpv_buffers_t* b)
{
    const float reach = h->K.contact_reach;
    FpvBufD d;
    memset(&d, 0, sizeof(d));          // padding bytes are part of the graph-cache key
    d.state = b->state; d.ld = b->ld; d.action = reinterpret_cast<const float4*>(b->action);
    d.reward = b->reward; d.done = b->done; d.done_bits = reinterpret_cast<unsigned long long*>(b->done_bits);
    d.accel = b->accel; d.ep_return = b->ep_return; d.ep_length = b->ep_length;
    d.last_return = b->last_return; d.last_length = b->last_length;
    d.wx = b->wind[0]; d.wy = b->wind[1]; d.wz = b->wind[2];
    d.state_h = b->state_h; d.seed = b->rounding_seed; d.obs_aos = b->obs_aos;
    d.pos_comp = b->pos_comp;
    d.noise_state = b->noise_state; d.action_out = reinterpret_cast<float4*>(b->action_out); d.step = 0;
    d.action_ld = b->action_ld;
    d.rot_over = b->rotation_override; d.thrust_over = b->thrust_override;
    d.thrust_h = b->state_h_thrust ? b->state_h_thrust : (b->state_h ? b->state_h + (int64_t)2 * FPV_HALF_PAIR_ROWS * b->ld : nullptr);
    if (b->objects) {
        copy_objects(b->objects, &d.objs);             // (check_buffers has passed the list)
        fpv_objects_bounds(d.objs, reach);
    }
    d.reset_pose = b->reset_pose;
    d.rj = h->rj;
    return d;
}

// Scoped device binding: makes `device` current for the launch and puts the caller's device back on the way out, so
// a single-process host with one handle per GPU ("one process with 8 handles") never finds its thread's
// current device changed by an fpv_* call.  No HIP call at all when the device is already current.
struct DeviceGuard {
    int prev = -1, rc = FPV_OK;
    bool switched = false;
    explicit DeviceGuard(int device)
    {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) { rc = hip_fail(e, "hipGetDevice"); return; }
        if (prev != device) {
            e = hipSetDevice(device);
            if (e != hipSuccess) { rc = hip_fail(e, "hipSetDevice"); return; }
            switched = true;
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// ---- kernel selection: every step kernel has the signature FPV_STEP_PARAMS, every k-step kernel (fpv_step_n) one FpvRollArgs ----
typedef void (*StepKernel)(float*, const int64_t, const float4*, const int64_t, uint16_t*, const int64_t, const FpvK, const FpvBufD);
typedef void (*RollKernel)(const FpvRollArgs);
typedef void (*GateResetKernel)(uint32_t*, const uint8_t*, const uint8_t*, const uint32_t, const int64_t);
// blocks of one single-step launch: n's, in whole rounds of the eight XCDs - every single-step kernel (drone, fp16 state, AoS head,
// Racer) reads n and the start block from one argument, and FPV_STEP_INDEX computes the same number from n
inline int64_t step_grid(int64_t n) { return (n + 8 * kStepBlock - 1) / (8 * kStepBlock) * 8; }

// Optional features of the drone kernels are independent template switches (in-kernel stick noise x object_list collisions x
// Kahan rows), each combination its own instantiation, so the plain kernel keeps its register budget.  Tables [noise][obj][kahan];
// the SQ k-step bodies exist without the object list only: [noise][kahan].  Racer: [wide][pid variant].
const StepKernel kDroneStep[2][2][2] = {
    {{fpv_drone_step_kernel<false, false, false>, fpv_drone_step_kernel<false, false, true>},
     {fpv_drone_step_kernel<false, true, false>, fpv_drone_step_kernel<false, true, true>}},
    {{fpv_drone_step_kernel<true, false, false>, fpv_drone_step_kernel<true, false, true>},
     {fpv_drone_step_kernel<true, true, false>, fpv_drone_step_kernel<true, true, true>}}};
// guidance override: the plain or the object-list kernel (check_buffers), [obj]
const StepKernel kDroneStepOverride[2] = {fpv_drone_step_kernel<false, false, false, true>, fpv_drone_step_kernel<false, true, false, true>};
const RollKernel kDroneRoll[2][2][2] = {
    {{fpv_drone_rollout_kernel<false, false, false>, fpv_drone_rollout_kernel<false, false, true>},
     {fpv_drone_rollout_kernel<false, true, false>, fpv_drone_rollout_kernel<false, true, true>}},
    {{fpv_drone_rollout_kernel<true, false, false>, fpv_drone_rollout_kernel<true, false, true>},
     {fpv_drone_rollout_kernel<true, true, false>, fpv_drone_rollout_kernel<true, true, true>}}};
const RollKernel kDroneRollSq[2][2] = {
    {fpv_drone_rollout_kernel<false, false, false, true>, fpv_drone_rollout_kernel<false, false, true, true>},
    {fpv_drone_rollout_kernel<true, false, false, true>, fpv_drone_rollout_kernel<true, false, true, true>}};
const StepKernel kRacerStep[2][2] = {{fpv_racer_step_kernel<false, false>, fpv_racer_step_kernel<false, true>},
                                     {fpv_racer_step_kernel<true, false>, fpv_racer_step_kernel<true, true>}};
const RollKernel kRacerRoll[2][2] = {{fpv_racer_rollout_kernel<false, false>, fpv_racer_rollout_kernel<false, true>},
                                     {fpv_racer_rollout_kernel<true, false>, fpv_racer_rollout_kernel<true, true>}};

// ---- the launch plan: which kernel serves a call, and on which path, is decided in plan_launch and nowhere else ----
// Reset sources (fpv_abi.h: the reset-pose table, FPV_FLAG_RESET_JITTER) live in the rare reset branch of the kernels that are
// NOT on the headline path: the non-SQ k-step kernels, the fp16 k-step kernel, the AoS-head kernel and the reset kernel.  The
// plain and fp16 single-step kernels and the SQ k-step kernel stay exactly as they were (tests/test_isa_claims.py pins them), so
// a handle with a reset source is routed around them:
//   - its single-step launches (fpv_step, every launch of fpv_rollout) run the k-step kernel with k = 1 - the same lane function
//     in the same order, bit-identical to the single-step kernel - fp32 state on fpv_drone_rollout_kernel (never SQ),
//     fp16 state on fpv_drone_rollout_h_kernel; they do not rotate their traversal;
//   - launches with the AoS head keep fpv_drone_step_aos_kernel, which carries the branch itself (the k-step kernel writes no
//     obs_aos rows);
//   - fpv_step_n never picks SQ; fpv_rollout_graph issues the launches instead of replaying them (the jitter needs the step
//     index of every launch).
// Cost: DESIGN.md "Reset sources".
// A physics table and a gate course follow the same rule with the kernels of fpv_phys.hip and fpv_gate.hip, whose k-step kernels
// carry the branch; a course with stick noise or an object list has no single-step kernel and takes the k = 1 route as well.
// A graph replays frozen kernel arguments, but stick noise, the fp16 rounding and the jitter are keyed by the per-launch step
// index: fpv_rollout_graph hands such a call, and every call whose single steps are the k-step kernel's, to fpv_step_n - the
// same k steps bit for bit, and cheaper than the replay - or to fpv_rollout when the AoS head is written (fpv_step_n writes none).
enum GraphRoute { kReplay, kToStepN, kToRollout };      // what fpv_rollout_graph does with a call
struct Plan {
    Family family;
    void* step;             // the single-step kernel (FPV_STEP_PARAMS; kGate: then one FpvGateArgs), or null: a single step is one step (k = 1) of `roll`, not rotated
    void* roll;             // the k-step kernel, of one FpvRollArgs (kTable: FpvRollPhysArgs, kGate: FpvRollGateArgs)
    bool ground = false;    // kTable: the launch loads the two ground rows
    GraphRoute graph = kReplay;
};

// a kernel's address as a launch and a graph node take it - the one cast (the tables above stay typed by signature)
template <class... P> void* entry(void (*kernel)(P...)) { return reinterpret_cast<void*>(kernel); }

Plan plan_launch(const fpv_env* h, const FpvBufD& d)
{
    const bool noise = (h->K.flags & FPV_FLAG_STICK_NOISE) != 0, fp16 = (h->K.flags & FPV_FLAG_FP16_STATE) != 0;
    const bool obj = d.objs.count > 0, kahan = d.pos_comp != nullptr, aos = d.obs_aos != nullptr, ground = (h->K.flags & FPV_FLAG_GROUND) != 0;
    const bool wide = h->K.r_wide != 0, pidv = h->K.r_pid_variant != 0;
    const bool reset = h->mode == FPV_MODE_DRONE && (d.reset_pose != nullptr || (h->K.flags & FPV_FLAG_RESET_JITTER) != 0);
    // the SQ k-step bodies: X frame, no ground springs, no object list - and no reset source, which they do not carry
    const bool sq = !obj && h->K.motor_square && !ground && !reset;
    Plan p;
    // a course and a table: [stick noise][object list] (a course with both is refused, check_combination); a table launch loads
    // the two ground rows when something reads them; the guidance override has the plain or the object-list kernel (check_buffers)
    if (h->gates) p = {kGate, noise || obj ? nullptr : fpv_gate_step_kernel(), fpv_gate_roll_kernel(noise, obj)};
    else if (h->phys) p = {kTable, fpv_phys_step_kernel(noise, obj), fpv_phys_roll_kernel(noise, obj), ground || obj};
    else if (h->mode != FPV_MODE_DRONE) p = {kRacer, entry(kRacerStep[wide][pidv]), entry(kRacerRoll[wide][pidv])};
    else if (fp16) p = {kFp16, entry(fpv_drone_step_h_kernel), entry(fpv_drone_rollout_h_kernel)};
    else p = {aos ? kAos : kPlain, entry(aos ? fpv_drone_step_aos_kernel : d.rot_over ? kDroneStepOverride[obj] : kDroneStep[noise][obj][kahan]),
              entry(sq ? kDroneRollSq[noise][kahan] : kDroneRoll[noise][obj][kahan])};
    if (reset && !aos) p.step = nullptr;
    p.graph = noise || fp16 || !p.step ? kToStepN : reset ? kToRollout : kReplay;
    return p;
}

// an accepted launch of k steps: the step index advances (a refused launch leaves it where it was) and a table handle remembers
// the rows it loaded
void launched(fpv_env* h, const Plan& p, int k)
{
    h->launches += (uint64_t)k;
    if (p.family == kTable) h->phys_rows_last = p.ground ? FPV_PHYS_ROWS : FPV_PHYS_ROWS - 2;
}

// one launch of the k-step kernel over the handle's drones: R.k steps from the handle's step index
int launch_roll(fpv_env* h, const Plan& p, const FpvBufD& d, const FpvRoll& R, hipStream_t s, const char* what)
{
    FpvRollArgs a = {h->K, d, h->n, R};
    a.B.step = h->launches;
    FpvRollPhysArgs pa;
    FpvRollGateArgs ga;
    void* arg = &a;
    if (p.family == kTable) { pa = {a, h->phys, p.ground ? 1 : 0, 0}; arg = &pa; }
    if (p.family == kGate) { ga = {a, h->ga}; arg = &ga; }
    const int rc = launch_args(what, p.roll, blocks_for(h->n, kStepBlock), dim3(kStepBlock), s, &arg);
    if (rc == FPV_OK) launched(h, p, R.k);
    return rc;
}

// The arguments of one single-step launch, filled in place - for the direct launch (launch_step) and for the kernel node of a
// graph alike: FPV_STEP_PARAMS' eight and the gate kernel's ninth (the other kernels do not read it).  The fifth is state_h - or
// the physics table or the gate word, whose kernels read no fp16 state -, the sixth n | start block << 32, with kPhysGroundBit
// when a table launch loads the ground rows.  np.kernelParams points at this object's own members, which hipLaunchKernel /
// hipGraphAddKernelNode / hipGraphExecKernelNodeSetParams copy - so it is used where it is built and never copied.
struct StepLaunch {
    FpvBufD d;
    FpvK K;
    int64_t n_start;
    void* slot5;
    FpvGateArgs ga;
    void* args[9];
    hipKernelNodeParams np;
    StepLaunch(const fpv_env* h, const Plan& p, const FpvBufD& dt, int64_t start)
        : d(dt), K(h->K), n_start(h->n | (start << 32) | (p.ground ? kPhysGroundBit : 0)),
          slot5(p.family == kGate ? (void*)h->ga.word : p.family == kTable ? (void*)const_cast<float*>(h->phys) : (void*)dt.state_h),
          ga(h->ga), args{&d.state, &d.ld, &d.action, &d.action_ld, &slot5, &n_start, &K, &d, &ga}
    {
        memset(&np, 0, sizeof(np));
        np.func = p.step; np.kernelParams = args;
        np.gridDim = dim3((unsigned)step_grid(h->n)); np.blockDim = dim3(kStepBlock);
    }
    StepLaunch(const StepLaunch&) = delete;
    StepLaunch& operator=(const StepLaunch&) = delete;
};

int64_t rotation_blocks(const fpv_env* h, const FpvBufD* d);      // below, with the cache sizes

// one single step from the handle's step index; a step of the k-step kernel returns before the rotation is touched
// (fpv_get_rotation reports what the last rotating launch set)
int launch_step(fpv_env* h, const Plan& p, const FpvBufD& d, hipStream_t s)
{
    // one step of the k-step kernel: reward / done / done_bits / episode sums leave after it, as after a single step
    if (!p.step) return launch_roll(h, p, d, FpvRoll{1, 0, 0, 0, 0}, s, "step kernel launch");
    const int64_t nblk = step_grid(h->n);
    h->rot_blocks = rotation_blocks(h, &d);
    const int64_t start = h->rot_blocks > 0 ? h->start_block % nblk : 0;
    StepLaunch L(h, p, d, start);
    L.d.step = h->launches;
    const int rc = launch_args("step kernel launch", L.np.func, L.np.gridDim, L.np.blockDim, s, L.np.kernelParams);
    if (rc != FPV_OK) return rc;
    launched(h, p, 1);
    if (h->rot_blocks > 0) h->start_block = (start + nblk - h->rot_blocks % nblk) % nblk;
    return FPV_OK;
}

// SHAPE of a graph: what patching its nodes cannot change - the kernel, the grid, the number of nodes - and every non-pointer
// argument of its launches, the handle's table and course with them (each zero-padded where it was filled).  Everything else in
// the view is a buffer address.  (The rounding seed and the jitter constants are arguments and so in the key, though no kernel a
// graph replays reads them: a changed seed on a handle without fp16 state rebuilds the graph where a patch would have done.)
template <class... T> std::string bytes_of(const T&... v)
{
    std::string s;
    (s.append(reinterpret_cast<const char*>(&v), sizeof(v)), ...);
    return s;
}

// MI355X: 256 MiB Infinity Cache (memory-side, shared by the eight XCDs) behind eight L2s of 4 MiB, one per XCD
// (/opt/skills/guides/MI355X_MICROARCH.md).  Both keep what was touched last, and both keep it across a kernel boundary (an L2
// line written by workgroup b is read again by the workgroup that gets the same block in the next launch: workgroups go to
// the XCDs round-robin, so a start that is a multiple of 8 blocks keeps every block on its XCD).  The rotation step is the
// drones whose WRITTEN bytes fill the cache level that the launch overflows (rotation_blocks):
//   a launch writes less than the L2s hold          plain order (everything is found again anyway)
//   more than the L2s, less than the Infinity Cache   61/64 * 32 MiB / written bytes per drone   (2^19 drones for the plain kernel's 61 B)
//   more than the Infinity Cache                    61/64 * 256 MiB / written bytes per drone  (2^22 drones)
// Measured (profiles/r05_exp_rotation_step_sweep.log): at 2^23 drones the launch time is flat from 30 000 to 35 000 blocks of 128 drones
// and 7 % worse at 36 000; at 2^20 drones it falls from 22.7 us (plain) to 20.2 us at 4096 blocks and is back at 21.9 us at 5120.
constexpr int kModelXcds = 8, kModelComputeUnits = 256;
constexpr int64_t kModelL2BytesPerXcd = (int64_t)4 << 20;
constexpr int64_t kInfinityCacheBytes = (int64_t)256 << 20;
constexpr int64_t kL2Bytes = (int64_t)kModelXcds * kModelL2BytesPerXcd;

// The rotation (block -> XCD round-robin over EIGHT XCDs, 8 x 4 MiB of L2, 256 MiB of Infinity Cache) and the row-stride rule (an
// L2 set hash fitted on this silicon) are a model of ONE device: gfx950 in its single-partition mode, 256 compute units.  HIP says
// which architecture a device is, how many compute units the process sees and how large ONE L2 is; it does not say how many XCDs
// there are or how large the Infinity Cache is - those follow from "gfx950 with all 256 CUs" (a CPX / DPX / QPX compute partition
// shows 32 / 128 / 64 CUs and one, four or two L2s: other rounds, another share).  Anything else gets the plain order and the
// conservative stride: results are the same bits either way, only the traversal's cache reuse is at stake.
void check_cache_model(const char* arch, int compute_units, int64_t l2_bytes, fpv_cache_model_t* m)
{
    memset(m, 0, sizeof(*m));
    m->struct_size = (uint32_t)sizeof(*m);
    m->compute_units = compute_units;
    m->l2_bytes_per_xcd = l2_bytes;
    snprintf(m->arch, sizeof(m->arch), "%s", arch ? arch : "");
    std::string why;
    if (strncmp(m->arch, "gfx950", 6) != 0 || (m->arch[6] != '\0' && m->arch[6] != ':'))
        why = std::string("architecture '") + m->arch + "' is not gfx950";
    else if (compute_units != kModelComputeUnits)
        why = "the process sees " + std::to_string(compute_units) + " compute units, not " + std::to_string(kModelComputeUnits)
              + " (a compute partition of the chip? the model is eight XCDs of 32 CUs in single-partition mode)";
    else if (l2_bytes != 0 && l2_bytes != kModelL2BytesPerXcd)          // 0 = the runtime does not report it: architecture and CU count pin the silicon
        why = "the device reports an L2 of " + std::to_string(l2_bytes) + " bytes, not " + std::to_string(kModelL2BytesPerXcd);
    if (why.empty()) {
        m->matches = 1; m->xcds = kModelXcds; m->infinity_cache_bytes = kInfinityCacheBytes;
    } else {
        why += ": plain traversal order and the conservative row stride (same results; no cache-aware rotation)";
        snprintf(m->reason, sizeof(m->reason), "%s", why.c_str());
    }
}

// asked once per device and process (hipGetDeviceProperties is a millisecond, fpv_create may be called hundreds of times)
int device_cache_model(int device, fpv_cache_model_t* out)
{
    static std::mutex mu;
    static std::vector<std::pair<int, fpv_cache_model_t>> known;
    const auto cached = [&] {                   // under mu
        for (const auto& k : known)
            if (k.first == device) { *out = k.second; return true; }
        return false;
    };
    {
        const std::lock_guard<std::mutex> lock(mu);
        if (cached()) return FPV_OK;
    }
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
    check_cache_model(prop.gcnArchName, prop.multiProcessorCount, (int64_t)prop.l2CacheSize, out);
    const std::lock_guard<std::mutex> lock(mu);
    if (!cached()) known.emplace_back(device, *out);      // another thread may have asked for the same device meanwhile
    return FPV_OK;
}

// Bytes of one drone's state in a layout (`K` = a handle's constants, or null for the mode's base layout): 14 fp32 rows; fp16
// state: 3 fp32 rows, the half-pair rows and the thrust half; Racer: 20 base rows (+6 (hi, lo) rows as written, +3 components.PID)
int state_bytes(int mode, const FpvK* K)
{
    if (mode == FPV_MODE_RACER) return 4 * (20 + (K && K->r_wide ? 6 : 0) + (K && K->r_pid_variant ? 3 : 0));
    if (K && (K->flags & FPV_FLAG_FP16_STATE)) return 3 * 4 + FPV_HALF_PAIR_ROWS * 4 + 2;
    return 4 * FPV_DRONE_ROWS;
}

// what one step moves per drone (fpv_algorithmic_bytes): state read + write, action read, reward + done write
int algorithmic_bytes(int mode, const FpvK* K) { return state_bytes(mode, K) * 2 + 16 + 4 + 1; }

// Bytes per drone that one launch WRITES and that compete for a cache between two visits of a drone (reads of rows that are
// written back are the same lines).  The plain kernel: 14 rows + reward + done = 61 B, and 4096 blocks of 128 drones x 61 B are the
// 32 MB of the eight L2s - where the sweep has its optimum (reward and done carry a streaming hint but stay in the count: the 61/64
// factor was fitted with them in).  The stick rows are only read; the accel rows and the AoS head are write-only rows stored with
// the streaming hint (ST_OUT) and measured not to compete (profiles/r06_exp_nt_output_rows.log).  `d` = the buffers of the launch,
// or null for an estimate from the handle alone (fpv_get_rotation before the first launch).
int64_t written_bytes_per_drone(const fpv_env* h, const FpvBufD* d)
{
    int64_t b = state_bytes(h->mode, &h->K);
    if (h->K.flags & FPV_FLAG_STICK_NOISE) b += 16;            // the four EMA rows
    if (h->gates) b += 4;                                       // the gate word (the obs rows are streaming stores, like accel)
    if (!d) return b + 5;
    if (d->reward) b += 4;
    if (d->done) b += 1;
    // (accel rows and the AoS observation head are written with the streaming hint - ST_OUT - and do not compete for the cache)
    if (d->pos_comp) b += 24;
    if (d->action_out) b += 16;
    if (d->ep_return) b += 8;                                   // running return and length (the last_* rows only when an episode ends)
    return b;
}

// blocks the start moves back per launch for these buffers: the cache level that the launch's writes overflow, 61/64 of it
// (the factor that puts the plain kernel on its measured optimum: 2^19 drones for the L2s, 2^22 for the Infinity Cache),
// whole rounds of the eight XCDs; an explicit request (fpv_set_rotation >= 0) as given
int64_t rotation_blocks(const fpv_env* h, const FpvBufD* d)
{
    const int64_t nblk = step_grid(h->n);
    if (h->rot_request >= 0) return (h->rot_request / kStepBlock) % (nblk > 0 ? nblk : 1);
    if (!h->cache.matches) return 0;             // not the device the model was measured on: plain order (fpv_get_cache_model says why)
    const int64_t bytes = written_bytes_per_drone(h, d);
    const int64_t fit_mall = kInfinityCacheBytes / 64 * 61 / bytes / kStepBlock / 8 * 8;
    const int64_t fit_l2 = kL2Bytes / 64 * 61 / bytes / kStepBlock / 8 * 8;
    return nblk > fit_mall ? fit_mall : nblk > fit_l2 ? fit_l2 : 0;
}

void update_rotation(fpv_env* h)
{
    h->rot_blocks = rotation_blocks(h, nullptr);
    h->start_block = 0;
}

// Which row stride keeps the rows that a launch finds again in an XCD's L2 from piling up in a few of its sets?  An XCD runs every
// eighth block, so of each row it touches 512 B of every 4 KiB; its L2 (4 MiB, 16 ways, 128-B lines: 2048 sets) indexes a line by
// its address folded once, set = (L ^ (L >> 11)) & 2047 with L = address / 128 - the fold distance is what the measurements fix
// (profiles/r05_exp_row_stride_l2_sets.log: 34 populations x 8 strides; folds of 10 or 12 bits do not explain them, 11 does).  The
// rows of one drone block sit r * stride apart: when the stride's low bits repeat its bits from 2^18 up (2^19 drones with the
// former 1 KiB pad: 2 MiB + 1 KiB), every row of a column meets in the same set and the L2 keeps a fraction of them - 13.2 us per
// launch at 2^19 drones against 10.7 us one class of stride further.  l2_set_overflow = the fraction of the lines of `blocks`
// blocks x 14 rows, as one XCD sees them, beyond the 16 ways of their set; taken over the fold and its additive twins (the
// measured penalty is symmetric in the sign of the low bits, the XOR alone is not).
constexpr int64_t kL2ModelFromDrones = 1 << 18;     // up to here a launch's rows are a fraction of the L2s: no stride measured any different
constexpr int64_t kL2ModelToDrones = 1 << 21;
constexpr double kL2OverflowOk = 0.06;
double l2_set_overflow(int64_t stride_bytes, int64_t blocks)
{
    double worst = 0.0;
    std::vector<uint16_t> cnt(2048);
    for (int mode = 0; mode < 3; ++mode) {
        std::fill(cnt.begin(), cnt.end(), (uint16_t)0);
        int64_t lines = 0;
        for (int64_t r = 0; r < FPV_DRONE_ROWS; ++r)
            for (int64_t j = 0; j < blocks / 8; ++j)
                for (int64_t l = 0; l < 4; ++l, ++lines) {
                    const int64_t L = (r * stride_bytes + j * 4096 + l * 128) >> 7, F = L >> 11;
                    ++cnt[(size_t)((mode == 0 ? (L ^ F) : mode == 1 ? (L + F) : (L - F)) & 2047)];
                }
        int64_t over = 0;
        for (const uint16_t c : cnt) over += c > 16 ? c - 16 : 0;
        worst = std::max(worst, lines ? (double)over / (double)lines : 0.0);
    }
    return worst;
}

// The row stride that needs no model of the caches: n rounded up to 64 floats and kept at least 1 KiB past a multiple of 8 KiB.
// 14 rows whose stride is (nearly) a multiple of 8 KiB land on the same HBM channel/bank set: measured at 2^20 drones, stride mod
// 8 KiB = 0 costs 6-9 %, 256-448 B still 2-3 %, 1-4 KiB nothing.
int64_t conservative_ld(int64_t n)
{
    int64_t ld = (n + 63) / 64 * 64;
    const int64_t r = ld % 2048;
    if (r < 256) ld += 256 - r;
    return ld;
}

int check_device_index(int device)
{
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(FPV_ENODEV, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0 || device >= count) return fail(FPV_ENODEV, "device index out of range");
    return FPV_OK;
}

// the kernel constants and the reset jitter of `params` (fpv_derive.h): FPV_OK, or the error code with *why set
int derive(const fpv_params_t* params, FpvK* K, FpvResetJitter* J, const char** why)
{
    const int rc = fpv_derive_constants(params, K, why);
    return rc == FPV_OK ? fpv_derive_reset_jitter(params, J, why) : rc;
}

}  // namespace

extern "C" {

int fpv_abi_version(void) { return FPV_ABI_VERSION; }

int fpv_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(fpv_params_t);
        case 1: return (int)sizeof(fpv_buffers_t);
        case 2: return (int)sizeof(fpv_objects_t);
        case 3: return (int)sizeof(fpv_pid_params_t);
        case 4: return (int)sizeof(fpv_cache_model_t);
        case 5: return (int)sizeof(fpv_gate_course_t);
        case 6: return (int)sizeof(fpv_range_scan_t);
        case 7: return (int)sizeof(fpv_depth_render_t);
        case 8: return (int)sizeof(fpv_chase_t);
        case 10: return (int)sizeof(fpv_pursuit_t);        // 9 stays refused: the tests of six features hold it to "no such struct"
        case 12: return (int)sizeof(fpv_pns_t);            // 11 stays refused like 9
        case 14: return (int)sizeof(fpv_detect_t);         // 13 and 15 stay refused like 9
        case 16: return (int)sizeof(fpv_boxes_t);
        case 18: return (int)sizeof(fpv_splat_t);          // 17 stays refused like 9
        default: return fail(FPV_EINVAL, "fpv_sizeof: 0 = fpv_params_t, 1 = fpv_buffers_t, 2 = fpv_objects_t, 3 = fpv_pid_params_t, 4 = fpv_cache_model_t, 5 = fpv_gate_course_t, 6 = fpv_range_scan_t, 7 = fpv_depth_render_t, 8 = fpv_chase_t, 10 = fpv_pursuit_t, 12 = fpv_pns_t, 14 = fpv_detect_t, 16 = fpv_boxes_t, 18 = fpv_splat_t");
    }
}

int fpv_state_rows(int mode)
{
    if (mode == FPV_MODE_DRONE) return FPV_DRONE_ROWS;
    if (mode == FPV_MODE_RACER) return FPV_RACER_ROWS;
    return fail(FPV_EINVAL, "unknown mode");
}

int fpv_algorithmic_bytes(int mode)
{
    if (mode != FPV_MODE_DRONE && mode != FPV_MODE_RACER) return fail(FPV_EINVAL, "unknown mode");
    return algorithmic_bytes(mode, nullptr);   // 133; Racer base rows (181 B); variants: fpv_handle_algorithmic_bytes
}

int fpv_handle_algorithmic_bytes(fpv_handle_t h)
{
    if (!h) return fail(FPV_EINVAL, "null handle");
    // the rows the selected kernel actually moves (fp16 state: 89); a physics table: + the rows the last launch loaded (before
    // the first launch: what the handle's flags alone ask for)
    const int rows = !h->phys ? 0 : h->phys_rows_last ? h->phys_rows_last : (h->K.flags & FPV_FLAG_GROUND) ? FPV_PHYS_ROWS : FPV_PHYS_ROWS - 2;
    // a gate course: the word read and written, and the six observation rows when they are bound
    const int gate = !h->gates ? 0 : 8 + (h->ga.obs ? 24 : 0);
    return algorithmic_bytes(h->mode, &h->K) + 4 * rows + gate;
}

int fpv_physics_rows(void) { return FPV_PHYS_ROWS; }

int fpv_physics_derive(const fpv_params_t* base, int64_t n, const double* inputs, float* out_rows, int64_t out_ld)
{
    if (!base || !out_rows) return fail(FPV_EINVAL, "null argument");
    if (n <= 0 || out_ld < n) return fail(FPV_EINVAL, "need 0 < n <= out_ld");
    FpvK K;
    const char* why = "";
    int rc = fpv_derive_constants(base, &K, &why);
    if (rc != FPV_OK) return fail(rc, why);
    if (base->mode != FPV_MODE_DRONE) return fail(FPV_EINVAL, "per-drone physics is a drone-mode feature");
    int64_t bad = -1;
    rc = fpv_derive_physics_table(base, n, inputs, out_rows, out_ld, &bad, &why);
    return rc == FPV_OK ? FPV_OK : fail(rc, "drone " + std::to_string(bad) + ": " + why);
}

int fpv_physics_sample(const fpv_params_t* base, uint64_t seed, uint64_t global_id0, int64_t n, const double* ranges, double* out_inputs)
{
    if (!base || !ranges || !out_inputs) return fail(FPV_EINVAL, "null argument");
    if (n <= 0) return fail(FPV_EINVAL, "n must be positive");
    FpvK K;
    const char* why = "";
    const int rc = fpv_derive_constants(base, &K, &why);
    if (rc != FPV_OK) return fail(rc, why);
    for (int c = 0; c < 2 * FPV_PHYS_INPUTS; ++c)
        if (!(c / 2 >= FPV_PHYS_IN_C2 && c / 2 <= FPV_PHYS_IN_C0) && !isfinite(ranges[c]))      // (the c2 c1 c0 rows are not read)
            return fail(FPV_EPARAM, "fpv_physics_sample: a range bound is not finite");
    fpv_sample_physics_inputs(base, seed, global_id0, n, ranges, out_inputs);
    return FPV_OK;
}

int fpv_set_physics(fpv_handle_t h, const float* table, int64_t ld)
{
    if (table && (!fpv_phys_step_kernel || !fpv_phys_roll_kernel))        // (asked first: what a build without the kernels answers to any bind)
        return fail(FPV_EINVAL, "per-drone physics is not in this build (the library was linked without csrc/fpv_phys.hip)");
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (table) {
        const int rc = check_combination(h, kTable, nullptr);
        if (rc != FPV_OK) return rc;
        if ((uintptr_t)table & 15) return fail(FPV_EALIGN, "the physics table must be 16-byte aligned");
        if (ld < h->n) return fail(FPV_EALIGN, "the physics table's ld is smaller than the number of drones");
        if (ld % 4) return fail(FPV_EALIGN, "the physics table's ld must be a multiple of 4 floats");
    }
    h->phys = table;
    h->phys_ld = table ? ld : 0;
    h->phys_rows_last = 0;
    h->graph_shape_key.clear();         // a cached graph carries the kernels and the table of the old binding
    return FPV_OK;
}

int fpv_get_physics(fpv_handle_t h, const float** table, int64_t* ld)
{
    if (!h || !table || !ld) return fail(FPV_EINVAL, "null argument");
    *table = h->phys; *ld = h->phys_ld;
    return FPV_OK;
}

int fpv_gates_derive(int count, const fpv_gate_t* gates, float* out_rows)
{
    if (!gates || !out_rows) return fail(FPV_EINVAL, "null argument");
    if (count < 1 || count > FPV_MAX_GATES) return fail(FPV_EPARAM, "a course has 1.." + std::to_string(FPV_MAX_GATES) + " gates, not " + std::to_string(count));
    for (int k = 0; k < count; ++k) {
        const char* why = "";
        const int rc = fpv_derive_gate_row(gates[k], out_rows + (int64_t)k * FPV_GATE_FLOATS, &why);
        if (rc != FPV_OK) return fail(rc, "gate " + std::to_string(k) + ": " + why);
    }
    return FPV_OK;
}

namespace {

// the uniform constants of a course, checked: FPV_OK or the error
int gate_constants(const fpv_gate_course_t* c, FpvGateK* G)
{
    if (c->struct_size != sizeof(fpv_gate_course_t)) return fail(FPV_EINVAL, "fpv_gate_course_t.struct_size does not match this library");
    if (c->count < 1 || c->count > FPV_MAX_GATES) return fail(FPV_EPARAM, "a course has 1.." + std::to_string(FPV_MAX_GATES) + " gates, not " + std::to_string(c->count));
    if (c->laps < 0 || (int64_t)c->laps * c->count > (int64_t)FPV_GATE_MAX_PASSED)
        return fail(FPV_EPARAM, "laps must be >= 0 and laps * count at most 2^22 - 1 (the word counts the gates passed in 22 bits)");
    const float r[5] = {c->progress_gain, c->pass_bonus, c->finish_bonus, c->miss_penalty, c->crash_penalty};
    for (const float x : r)
        if (!isfinite(x)) return fail(FPV_EPARAM, "a reward constant of the course is not finite");
    memset(G, 0, sizeof(*G));
    G->progress_gain = c->progress_gain; G->pass_bonus = c->pass_bonus; G->finish_bonus = c->finish_bonus;
    G->miss_penalty = c->miss_penalty; G->crash_penalty = c->crash_penalty;
    G->count = (uint32_t)c->count; G->finish_at = (uint32_t)(c->laps * c->count); G->miss_done = c->miss_is_done ? 1u : 0u;
    return FPV_OK;
}

}  // namespace

int fpv_set_gates(fpv_handle_t h, const fpv_gate_course_t* c)
{
    if (c && (!fpv_gate_step_kernel || !fpv_gate_roll_kernel || !fpv_gate_reset_kernel_fn))      // (asked first: what a build without the kernels answers to any bind)
        return fail(FPV_EINVAL, "gate courses are not in this build (the library was linked without csrc/fpv_gate.hip)");
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (!c) {
        h->gates = false;
        memset(&h->ga, 0, sizeof(h->ga));
        update_rotation(h);
        h->graph_shape_key.clear();
        return FPV_OK;
    }
    FpvGateArgs a;
    memset(&a, 0, sizeof(a));          // padding bytes are part of the graph-cache key
    int rc = gate_constants(c, &a.K);
    if (rc == FPV_OK) rc = check_combination(h, kGate, nullptr);
    if (rc != FPV_OK) return rc;
    if (!c->descriptors || !c->gate_word) return fail(FPV_EINVAL, "fpv_gate_course_t.descriptors and gate_word must be given");
    if ((uintptr_t)c->descriptors & 15) return fail(FPV_EALIGN, "the gate descriptors must be 16-byte aligned");
    if (((uintptr_t)c->gate_word & 3) || ((uintptr_t)c->gate_obs & 3)) return fail(FPV_EALIGN, "gate_word and gate_obs must be 4-byte aligned");
    if (c->gate_obs && c->gate_obs_ld < h->n) return fail(FPV_EALIGN, "gate_obs_ld is smaller than the number of drones");
    a.tab = reinterpret_cast<const fpv_gate_v4*>(c->descriptors);
    a.word = c->gate_word; a.obs = c->gate_obs; a.obs_ld = c->gate_obs ? c->gate_obs_ld : 0; a.start = c->gate_start;
    h->ga = a;
    h->gates = true;
    update_rotation(h);
    h->graph_shape_key.clear();         // a cached graph carries the kernels and the course of the old binding
    return FPV_OK;
}

int fpv_gate_eval(const fpv_gate_course_t* c, int64_t n, const float* p_old, const float* p_new, const float* q_new,
                  const uint8_t* physics_done, const uint32_t* word_in, int auto_reset, const float* p_after, const float* q_after,
                  uint32_t* word_out, float* reward, uint8_t* done, float* obs)
{
    if (!c || !p_old || !p_new || !q_new || !word_in || !word_out || !reward || !done) return fail(FPV_EINVAL, "null argument");
    if (n <= 0) return fail(FPV_EINVAL, "n must be positive");
    FpvGateK G;
    const int rc = gate_constants(c, &G);
    if (rc != FPV_OK) return rc;
    if (!c->descriptors) return fail(FPV_EINVAL, "fpv_gate_course_t.descriptors must be given (host memory)");
    alignas(16) float rows[FPV_MAX_GATES * FPV_GATE_FLOATS];
    memcpy(rows, c->descriptors, sizeof(float) * FPV_GATE_FLOATS * (size_t)c->count);
    const fpv_gate_v4* tab = reinterpret_cast<const fpv_gate_v4*>(rows);
    for (int64_t i = 0; i < n; ++i) {
        const float* po = p_old + 3 * i; const float* pn = p_new + 3 * i;
        const uint32_t g = fpv_gate_index(word_in[i], G.count);
        const fpv_gate_v4* d = tab + g * FPV_GATE_GROUPS;
        const FpvGateOut o = fpv_gate_step<true>(G, fpv_gate_cn(d), d, word_in[i], po[0], po[1], po[2], pn[0], pn[1], pn[2],
                                                 physics_done && physics_done[i]);
        uint32_t w = o.word;
        const float* pa = pn; const float* qa = q_new + 4 * i;
        if (auto_reset && o.done) {
            w = fpv_gate_word_reset(w, c->gate_start ? (uint32_t)c->gate_start[i] : 0u, G.count);
            if (p_after) pa = p_after + 3 * i;
            if (q_after) qa = q_after + 4 * i;
        }
        word_out[i] = w; reward[i] = o.reward; done[i] = o.done ? 1 : 0;
        if (obs) {
            FpvQuat q; q.w = qa[0]; q.x = qa[1]; q.y = qa[2]; q.z = qa[3];
            fpv_gate_obs(fpv_gate_cn(tab + fpv_gate_index(w, G.count) * FPV_GATE_GROUPS), q, pa[0], pa[1], pa[2], obs + 6 * i);
        }
    }
    return FPV_OK;
}

int fpv_rays_derive(int count, const double* dirs, float* out)
{
    if (!dirs || !out) return fail(FPV_EINVAL, "null argument");
    if (count < 1 || count > FPV_MAX_RAYS) return fail(FPV_EPARAM, "a ray set has 1.." + std::to_string(FPV_MAX_RAYS) + " rays, not " + std::to_string(count));
    int bad = -1;
    const char* why = "";
    const int rc = fpv_derive_rays(count, dirs, out, &bad, &why);
    return rc == FPV_OK ? FPV_OK : fail(rc, "ray " + std::to_string(bad) + ": " + why);
}

namespace {

// the uniform constants of a scan and its object list, checked (everything of fpv_range_scan_t but `ranges`): FPV_OK or the error
int range_constants(const fpv_range_scan_t* s, FpvRangeK* K, FpvObjects* T)
{
    if (s->struct_size != sizeof(fpv_range_scan_t)) return fail(FPV_EINVAL, "fpv_range_scan_t.struct_size does not match this library");
    if (s->ray_count < 1 || s->ray_count > FPV_MAX_RAYS)
        return fail(FPV_EINVAL, "ray_count: a ray set has 1.." + std::to_string(FPV_MAX_RAYS) + " rays, not " + std::to_string(s->ray_count));
    if (!isfinite(s->max_range) || !(s->max_range > 0.0f)) return fail(FPV_EINVAL, "max_range must be finite and positive");
    memset(K, 0, sizeof(*K));
    memset(T, 0, sizeof(*T));
    K->max_range = s->max_range; K->ray_count = s->ray_count;
    for (int r = 0; r < s->ray_count; ++r) {
        const float* d = s->rays[r];
        const double l2 = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
        if (!(fabs(l2 - 1.0) <= 1.0e-4)) return fail(FPV_EINVAL, "ray " + std::to_string(r) + " is not a unit direction (rays come from fpv_rays_derive)");
        for (int j = 0; j < 3; ++j) K->rays[r][j] = d[j];
    }
    int rc = check_object_count(s->objects, true);
    if (rc == FPV_OK) rc = check_object_types(s->objects);
    if (rc != FPV_OK) return rc;
    copy_objects(s->objects, T);
    fpv_range_bounds(*T, K->max_range, K->near);
    return FPV_OK;
}

}  // namespace

int fpv_range_scan(fpv_handle_t h, const fpv_buffers_t* b, const fpv_range_scan_t* s, void* stream)
{
    int rc = check_sensor(h, b, s, fpv_range_scan_kernel_fn != nullptr, "range scan", "fpv_range");
    if (rc != FPV_OK) return rc;
    FpvRangeArgs A;
    memset(&A, 0, sizeof(A));
    rc = range_constants(s, &A.K, &A.T);
    if (rc != FPV_OK) return rc;
    if (!s->ranges) return fail(FPV_EINVAL, "fpv_range_scan_t.ranges is null");
    if ((uintptr_t)s->ranges & 3) return fail(FPV_EALIGN, "ranges must be 4-byte aligned");
    if (s->ranges_ld < h->n) return fail(FPV_EALIGN, "ranges_ld is smaller than the number of drones");
    if (s->ranges_ld % 4) return fail(FPV_EALIGN, "ranges_ld must be a multiple of 4 floats");
    A.state = b->state; A.ld = b->ld; A.ranges = s->ranges; A.ranges_ld = s->ranges_ld; A.n = h->n;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    void* arg = &A;
    return launch_args("range scan launch", fpv_range_scan_kernel_fn(), blocks_for(h->n, kStepBlock), dim3(kStepBlock), (hipStream_t)stream, &arg);
}

int fpv_range_eval(const fpv_range_scan_t* s, int64_t n, const float* p, const float* q)
{
    int rc = check_eval_args(s, n, p, q);
    if (rc != FPV_OK) return rc;
    FpvRangeK K;
    FpvObjects T;
    rc = range_constants(s, &K, &T);
    if (rc != FPV_OK) return rc;
    if (!s->ranges) return fail(FPV_EINVAL, "fpv_range_scan_t.ranges is null");
    if (s->ranges_ld < n) return fail(FPV_EALIGN, "ranges_ld is smaller than n");
    if (s->ranges_ld % 4) return fail(FPV_EALIGN, "ranges_ld must be a multiple of 4 floats");
    float* const out = s->ranges;
    const int64_t ld = s->ranges_ld;
    for (int64_t i = 0; i < n; ++i)
        fpv_range_lane(K, T, pose_quat(q, i), p[3 * i], p[3 * i + 1], p[3 * i + 2], [&](int r, float t) { out[(int64_t)r * ld + i] = t; });
    return FPV_OK;
}

int fpv_camera_derive(const fpv_camera_t* camera, fpv_depth_render_t* out)
{
    if (!camera || !out) return fail(FPV_EINVAL, "null argument");
    const char* why = "";
    const int rc = fpv_depth_derive(*camera, out, &why);
    return rc == FPV_OK ? FPV_OK : fail(rc, std::string("camera: ") + why);
}

namespace {

// the uniform constants of a render and its object list, checked (everything of fpv_depth_render_t but `image` and the gate
// table's address space): FPV_OK or the error
int depth_constants(const fpv_depth_render_t* s, FpvDepthK* K, FpvObjects* T)
{
    if (s->struct_size != sizeof(fpv_depth_render_t)) return fail(FPV_EINVAL, "fpv_depth_render_t.struct_size does not match this library");
    if (s->width < 4 || s->width > FPV_DEPTH_MAX_SIDE || s->height < 4 || s->height > FPV_DEPTH_MAX_SIDE)
        return fail(FPV_EINVAL, "width and height must be 4.." + std::to_string(FPV_DEPTH_MAX_SIDE) + " pixels, not " + std::to_string(s->width) + " x " + std::to_string(s->height));
    if (s->width % 4) return fail(FPV_EINVAL, "width must be a multiple of 4 (four pixels share a dword of the byte image)");
    if (s->encoding != FPV_DEPTH_METRES && s->encoding != FPV_DEPTH_U8) return fail(FPV_EINVAL, "unknown encoding (0 FPV_DEPTH_METRES, 1 FPV_DEPTH_U8)");
    if (!isfinite(s->max_depth) || !(s->max_depth > 0.0f)) return fail(FPV_EINVAL, "max_depth must be finite and positive");
    if (s->gate_count < 0 || s->gate_count > FPV_MAX_GATES)
        return fail(FPV_EINVAL, "gate_count must be 0.." + std::to_string(FPV_MAX_GATES) + ", not " + std::to_string(s->gate_count));
    if (s->gate_count > 0) {
        if (!s->gate_descriptors) return fail(FPV_EINVAL, "gates without descriptors (gate_descriptors is null)");
        if ((uintptr_t)s->gate_descriptors & 15) return fail(FPV_EALIGN, "gate_descriptors must be 16-byte aligned");
        if (!isfinite(s->gate_frame_width) || !(s->gate_frame_width > 0.0f)) return fail(FPV_EINVAL, "gate_frame_width must be finite and positive");
    }
    if (!isfinite(s->dir_len_max) || !(s->dir_len_max >= 1.0f)) return fail(FPV_EINVAL, "dir_len_max is not what fpv_camera_derive writes");
    memset(K, 0, sizeof(*K));
    memset(T, 0, sizeof(*T));
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(s->dir0[k]) || !isfinite(s->dir_u[k]) || !isfinite(s->dir_v[k]) || !isfinite(s->offset[k]))
            return fail(FPV_EINVAL, "direction vectors and offset must be finite (they come from fpv_camera_derive)");
        K->a0[k] = s->dir0[k]; K->au[k] = s->dir_u[k]; K->av[k] = s->dir_v[k]; K->rel[k] = s->offset[k];
    }
    {   // no pixel's direction may be longer than dir_len_max says: the cull's margin rests on it
        double worst = 0.0;
        for (int c = 0; c < 4; ++c) {
            const double i = (c & 1) ? s->width - 1 : 0, j = (c & 2) ? s->height - 1 : 0;
            double l2 = 0.0;
            for (int k = 0; k < 3; ++k) { const double d = (double)s->dir0[k] + i * s->dir_u[k] + j * s->dir_v[k]; l2 += d * d; }
            worst = l2 > worst ? l2 : worst;
        }
        if (!(sqrt(worst) <= (double)s->dir_len_max * (1.0 + 1.0e-5))) return fail(FPV_EINVAL, "a pixel's direction is longer than dir_len_max (both come from fpv_camera_derive)");
    }
    K->max_depth = s->max_depth;
    K->reach = fpv_depth_reach(s->max_depth, s->dir_len_max);
    K->frame_width = s->gate_count > 0 ? s->gate_frame_width : 0.0f;
    K->width = s->width; K->height = s->height; K->gate_count = s->gate_count;
    int rc = check_object_count(s->objects, true);
    if (rc == FPV_OK) rc = check_object_types(s->objects);
    if (rc != FPV_OK) return rc;
    copy_objects(s->objects, T);
    fpv_range_bounds(*T, K->reach, K->near);
    return FPV_OK;
}

int depth_image_checks(const fpv_depth_render_t* s)
{
    if (!s->image) return fail(FPV_EINVAL, "fpv_depth_render_t.image is null");
    if ((uintptr_t)s->image & 3) return fail(FPV_EALIGN, "image must be 4-byte aligned");
    if (s->image_stride < (int64_t)s->width * s->height) return fail(FPV_EALIGN, "image_stride is smaller than width * height");
    if (s->image_stride % 4) return fail(FPV_EALIGN, "image_stride must be a multiple of 4 elements");
    return FPV_OK;
}

}  // namespace

int fpv_depth_render(fpv_handle_t h, const fpv_buffers_t* b, const fpv_depth_render_t* s, void* stream)
{
    int rc = check_sensor(h, b, s, fpv_depth_render_kernel_fn != nullptr, "depth camera", "fpv_depth");
    if (rc != FPV_OK) return rc;
    FpvDepthArgs A;
    memset(&A, 0, sizeof(A));
    rc = depth_constants(s, &A.K, &A.T);
    if (rc != FPV_OK) return rc;
    rc = depth_image_checks(s);
    if (rc != FPV_OK) return rc;
    const int64_t wpi = ((int64_t)s->width * s->height + 63) / 64, waves = wpi * h->n;
    if (waves > ((int64_t)1 << 31)) return fail(FPV_EINVAL, "more than 2^31 waves (drones x ceil(width * height / 64)): render the population in parts");
    A.state = b->state; A.ld = b->ld; A.gates = reinterpret_cast<const fpv_gate_v4*>(s->gate_descriptors);
    A.image = s->image; A.image_stride = s->image_stride; A.n = h->n; A.waves_per_image = (uint32_t)wpi;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    void* arg = &A;
    return launch_args("depth render launch", fpv_depth_render_kernel_fn(s->encoding == FPV_DEPTH_U8), blocks_for(waves, 4), dim3(256), (hipStream_t)stream, &arg);
}

int fpv_depth_eval(const fpv_depth_render_t* s, int64_t n, const float* p, const float* q)
{
    int rc = check_eval_args(s, n, p, q);
    if (rc != FPV_OK) return rc;
    FpvDepthK K;
    FpvObjects T;
    rc = depth_constants(s, &K, &T);
    if (rc != FPV_OK) return rc;
    rc = depth_image_checks(s);
    if (rc != FPV_OK) return rc;
    const fpv_gate_v4* const gates = reinterpret_cast<const fpv_gate_v4*>(s->gate_descriptors);
    for (int64_t i = 0; i < n; ++i) {
        const FpvRot R = fpv_rot(pose_quat(q, i));
        float ox, oy, oz;
        fpv_depth_origin(K, R, p[3 * i], p[3 * i + 1], p[3 * i + 2], &ox, &oy, &oz);
        uint32_t obj_mask = 0u;
        uint64_t gate_mask = 0ull;
        for (int k = 0; k < T.count; ++k) obj_mask |= fpv_depth_object_near(K, T, k, ox, oy, oz) ? 1u << k : 0u;
        for (int g = 0; g < K.gate_count; ++g)
            gate_mask |= fpv_depth_gate_near(K, gates[(size_t)g * FPV_GATE_GROUPS], gates[(size_t)g * FPV_GATE_GROUPS + 3], ox, oy, oz) ? 1ull << g : 0ull;
        for (int32_t y = 0; y < K.height; ++y)
            for (int32_t x = 0; x < K.width; ++x) {
                const float d = fpv_depth_pixel(K, T, gates, R, ox, oy, oz, obj_mask, gate_mask, (uint32_t)x, (uint32_t)y);
                const int64_t at = i * s->image_stride + (int64_t)y * K.width + x;
                if (s->encoding == FPV_DEPTH_U8) static_cast<uint8_t*>(s->image)[at] = (uint8_t)fpv_depth_u8(d, K.max_depth);
                else static_cast<float*>(s->image)[at] = d;
            }
    }
    return FPV_OK;
}

int fpv_chase_derive(const fpv_camera_t* camera, fpv_chase_t* out)
{
    if (!camera || !out) return fail(FPV_EINVAL, "null argument");
    const char* why = "";
    const int rc = fpv_chase_derive_camera(*camera, out, &why);
    return rc == FPV_OK ? FPV_OK : fail(rc, std::string("camera: ") + why);
}

namespace {

const char kChaseAbsent[] = "the target chase is not in this build (the library was linked without csrc/fpv_chase.hip)";

// the uniform constants of a call and its buffers, checked (n: the drones the buffers must hold): FPV_OK or the error
int chase_args(const fpv_chase_t* s, int64_t n, FpvChaseArgs* A)
{
    if (s->struct_size != sizeof(fpv_chase_t)) return fail(FPV_EINVAL, "fpv_chase_t.struct_size does not match this library");
    if (s->width < 1 || s->width > FPV_CHASE_MAX_SIDE || s->height < 1 || s->height > FPV_CHASE_MAX_SIDE)
        return fail(FPV_EINVAL, "width and height must be 1.." + std::to_string(FPV_CHASE_MAX_SIDE) + " pixels, not " + std::to_string(s->width) + " x " + std::to_string(s->height));
    if (s->ref_frame != FPV_CHASE_WORLD && s->ref_frame != FPV_CHASE_DRONE) return fail(FPV_EINVAL, "unknown ref_frame (0 FPV_CHASE_WORLD, 1 FPV_CHASE_DRONE)");
    if (s->mode != FPV_CHASE_LEVEL && s->mode != FPV_CHASE_FRONTARGET) return fail(FPV_EINVAL, "unknown mode (0 FPV_CHASE_LEVEL, 1 FPV_CHASE_FRONTARGET)");
    if (!isfinite(s->focal_length) || !(s->focal_length > 0.0)) return fail(FPV_EINVAL, "focal_length must be finite and positive (it comes from fpv_chase_derive)");
    for (int k = 0; k < 9; ++k)
        if (!isfinite(s->relative_rotation[k]) || !isfinite(s->relative_position[k % 3]))
            return fail(FPV_EINVAL, "relative_rotation and relative_position must be finite (they come from fpv_chase_derive)");
    if (!isfinite(s->max_depth) || !(s->max_depth > 0.0)) return fail(FPV_EINVAL, "max_depth must be finite and positive");
    if (!isfinite(s->mass) || !(s->mass > 0.0)) return fail(FPV_EPARAM, "mass must be finite and positive");
    const double five[5] = {s->virtual_drag_coefficient, s->virtual_lift_coefficient, s->tof_effective_distance, s->keep_distance, s->UWB_sensor_max_range};
    const char* const names[5] = {"virtual_drag_coefficient", "virtual_lift_coefficient", "tof_effective_distance", "keep_distance", "UWB_sensor_max_range"};
    for (int k = 0; k < 5; ++k)
        if (!isfinite(five[k])) return fail(FPV_EPARAM, std::string(names[k]) + " is not finite");
    for (int k = 0; k < 3; ++k)
        if (!isfinite(s->target[k])) return fail(FPV_EPARAM, "the target's centre is not finite");
    if (!isfinite(s->target_radius) || !(s->target_radius >= 0.0f)) return fail(FPV_EPARAM, "the target's radius must be finite and not negative");
    const fpv_pid_params_t& P = s->pid;
    if (P.struct_size != sizeof(fpv_pid_params_t)) return fail(FPV_EINVAL, "fpv_chase_t.pid.struct_size does not match this library");
    const double pid[8] = {P.kP, P.kI, P.kD, P.dt, P.integral_clip, P.min_output, P.max_output, P.derivative_transition_rate};
    for (int k = 0; k < 8; ++k)
        if (!isfinite(pid[k])) return fail(FPV_EPARAM, "a PID constant is not finite");
    if (!(P.dt > 0)) return fail(FPV_EPARAM, "dt must be positive");
    if (!(P.integral_clip >= 0) || !(P.min_output <= P.max_output) || !(P.derivative_transition_rate >= 0 && P.derivative_transition_rate <= 1))
        return fail(FPV_EPARAM, "components.PID constants: integral_clip >= 0, min_output <= max_output, derivative_transition_rate in [0, 1]");
    if (!s->pid_state) return fail(FPV_EINVAL, "fpv_chase_t.pid_state is null");
    if (!s->rotation) return fail(FPV_EINVAL, "fpv_chase_t.rotation is null");
    if (!s->thrust) return fail(FPV_EINVAL, "fpv_chase_t.thrust is null");
    if (s->pid_ld < n) return fail(FPV_EALIGN, "fpv_chase_t.pid_ld is smaller than the number of drones");
    if (((uintptr_t)s->pid_state & 3) || ((uintptr_t)s->rotation & 3) || ((uintptr_t)s->thrust & 3))
        return fail(FPV_EALIGN, "pid_state, rotation and thrust must be 4-byte aligned");
    if (((uintptr_t)s->pixel & 7) || ((uintptr_t)s->pixel_out & 7)) return fail(FPV_EALIGN, "pixel and pixel_out must be 8-byte aligned");
    memset(A, 0, sizeof(*A));
    FpvChaseK& K = A->K;
    for (int k = 0; k < 9; ++k) K.rr[k] = (float)s->relative_rotation[k];
    for (int k = 0; k < 3; ++k) { K.rel[k] = (float)s->relative_position[k]; K.tc[k] = s->target[k]; }
    K.f = (float)s->focal_length; K.cx = (float)(0.5 * s->width); K.cy = (float)(0.5 * s->height); K.w = (float)s->width; K.h = (float)s->height;
    K.max_depth = (float)s->max_depth; K.tr = s->target_radius;
    K.gz = (float)(-9.81 * s->mass);                                     // kinematics.gravity_vector(mass, g=9.81): components.py:270
    K.vdrag = (float)five[0]; K.vlift = (float)five[1]; K.tof = (float)five[2]; K.keep = (float)five[3]; K.uwb = (float)five[4];
    K.frame = s->ref_frame; K.mode = s->mode;
    K.pid.dt = (float)P.dt; K.pid.inv_dt = (float)(1.0 / P.dt);
    K.pid.gain[0][0] = (float)P.kP; K.pid.gain[0][1] = (float)P.kI; K.pid.gain[0][2] = (float)P.kD;
    K.pid.integral_clip = (float)P.integral_clip; K.pid.min_output = (float)P.min_output; K.pid.max_output = (float)P.max_output;
    K.pid.d_rate = (float)P.derivative_transition_rate; K.pid.om_d_rate = (float)(1.0 - P.derivative_transition_rate);
    A->pid_state = s->pid_state; A->pid_ld = s->pid_ld; A->pixel = s->pixel; A->rotation = s->rotation; A->thrust = s->thrust;
    A->pixel_out = s->pixel_out; A->visible = s->visible; A->n = n;
    return FPV_OK;
}

}  // namespace

int fpv_chase_guide(fpv_handle_t h, const fpv_buffers_t* b, const fpv_chase_t* s, void* stream)
{
    if (fpv_chase_kernel_fn == nullptr) return fail(FPV_EINVAL, kChaseAbsent);
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (!b || !s) return fail(FPV_EINVAL, "null argument");
    if (h->mode != FPV_MODE_DRONE) return fail(FPV_EINVAL, "the target chase is the Drone's guidance law: not for a Racer handle");
    if (h->K.flags & FPV_FLAG_FP16_STATE)
        return fail(FPV_EINVAL, "the target chase cannot read fp16 state (FPV_FLAG_FP16_STATE): a reader of the packed quaternion is the follow-up");
    if (!b->state) return fail(FPV_EINVAL, "fpv_buffers_t.state is null");
    if (b->ld < h->n) return fail(FPV_EALIGN, "fpv_buffers_t.ld is smaller than the number of drones");
    FpvChaseArgs A;
    const int rc = chase_args(s, h->n, &A);
    if (rc != FPV_OK) return rc;
    A.state = b->state; A.ld = b->ld;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    void* arg = &A;
    return launch_args("chase kernel launch", fpv_chase_kernel_fn(s->pixel != nullptr), blocks_for(h->n, kStepBlock), dim3(kStepBlock), (hipStream_t)stream, &arg);
}

int fpv_chase_eval(const fpv_chase_t* s, int64_t n, const float* p, const float* v, const float* q)
{
    if (fpv_chase_eval_host == nullptr) return fail(FPV_EINVAL, kChaseAbsent);
    if (!v) return fail(FPV_EINVAL, "null argument");
    int rc = check_eval_args(s, n, p, q);
    if (rc != FPV_OK) return rc;
    FpvChaseArgs A;
    rc = chase_args(s, n, &A);
    if (rc != FPV_OK) return rc;
    fpv_chase_eval_host(&A, p, v, q);
    return FPV_OK;
}

int fpv_pns_derive(const fpv_camera_t* camera, fpv_pns_t* out)
{
    if (!camera || !out) return fail(FPV_EINVAL, "null argument");
    fpv_chase_t c;
    const int rc = fpv_chase_derive(camera, &c);
    if (rc != FPV_OK) return rc;
    out->width = c.width; out->height = c.height; out->focal_length = c.focal_length;
    memcpy(out->relative_rotation, c.relative_rotation, sizeof c.relative_rotation);
    memcpy(out->relative_position, c.relative_position, sizeof c.relative_position);
    return FPV_OK;
}

namespace {

const char kPnsAbsent[] = "point and shoot is not in this build (the library was linked without csrc/fpv_pns.hip)";

// the uniform constants of a call and its buffers, checked (n: the drones the buffers must hold): FPV_OK or the error.  What the
// struct shares with fpv_chase_t is checked by chase_args itself, on a fpv_chase_t holding those fields.
int pns_args(const fpv_pns_t* s, int64_t n, FpvPnsArgs* A)
{
    if (s->struct_size != sizeof(fpv_pns_t)) return fail(FPV_EINVAL, "fpv_pns_t.struct_size does not match this library");
    if (!s->pid_state) return fail(FPV_EINVAL, "fpv_pns_t.pid_state is null");
    if (!s->prev_pixel) return fail(FPV_EINVAL, "fpv_pns_t.prev_pixel is null");
    if (!s->rotation) return fail(FPV_EINVAL, "fpv_pns_t.rotation is null");
    if (!s->thrust) return fail(FPV_EINVAL, "fpv_pns_t.thrust is null");
    if (s->pid.struct_size != sizeof(fpv_pid_params_t)) return fail(FPV_EINVAL, "fpv_pns_t.pid.struct_size does not match this library");
    if (s->pid_ld < n) return fail(FPV_EALIGN, "fpv_pns_t.pid_ld is smaller than the number of drones");
    if (((uintptr_t)s->pixel & 7) || ((uintptr_t)s->pixel_velocity & 7)) return fail(FPV_EALIGN, "pixel and pixel_velocity must be 8-byte aligned");
    fpv_chase_t c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.width = s->width; c.height = s->height; c.ref_frame = s->ref_frame; c.mode = s->mode; c.focal_length = s->focal_length;
    memcpy(c.relative_rotation, s->relative_rotation, sizeof c.relative_rotation);
    memcpy(c.relative_position, s->relative_position, sizeof c.relative_position);
    c.max_depth = s->max_depth; c.mass = s->mass; c.virtual_drag_coefficient = s->virtual_drag_coefficient;
    c.virtual_lift_coefficient = s->virtual_lift_coefficient; c.tof_effective_distance = s->tof_effective_distance;
    c.pid = s->pid; c.pid_state = s->pid_state; c.pid_ld = s->pid_ld; c.rotation = s->rotation; c.thrust = s->thrust;
    FpvChaseArgs C;
    const int rc = chase_args(&c, n, &C);
    if (rc != FPV_OK) return rc;
    if (!isfinite(s->max_throttle_in_force) || !(s->max_throttle_in_force > 0.0)) return fail(FPV_EPARAM, "max_throttle_in_force must be finite and positive");
    for (int k = 0; k < 4; ++k)
        if (!isfinite(s->thrust2throttle_poly[k])) return fail(FPV_EPARAM, "thrust2throttle_poly is not finite");
    if (s->target && s->target_rows) return fail(FPV_EINVAL, "both a shared target and target_rows are given: one target per call");
    if (!s->pixel && !s->target && !s->target_rows) return fail(FPV_EINVAL, "pixel is null and neither target nor target_rows is given");
    if (s->prev_pixel_ld < n) return fail(FPV_EALIGN, "fpv_pns_t.prev_pixel_ld is smaller than the number of drones");
    if (s->target_rows && s->target_ld < n) return fail(FPV_EALIGN, "fpv_pns_t.target_ld is smaller than the number of drones");
    if (((uintptr_t)s->prev_pixel & 3) || ((uintptr_t)s->target_rows & 3) || ((uintptr_t)s->throttle & 3))
        return fail(FPV_EALIGN, "prev_pixel, target_rows and throttle must be 4-byte aligned");
    if ((uintptr_t)s->action & 15) return fail(FPV_EALIGN, "action must be 16-byte aligned");
    memset(A, 0, sizeof(*A));
    FpvPnsK& K = A->K;
    K.C = C.K;
    K.fmax = (float)s->max_throttle_in_force;
    for (int k = 0; k < 4; ++k) K.inv[k] = (float)s->thrust2throttle_poly[k];
    if (s->target) {
        for (int k = 0; k < 3; ++k) {
            if (!isfinite(s->target[k])) return fail(FPV_EPARAM, "the target's centre is not finite");
            K.tc[k] = s->target[k];
        }
    }
    A->pid_state = s->pid_state; A->pid_ld = s->pid_ld; A->prev_pixel = s->prev_pixel; A->prev_ld = s->prev_pixel_ld; A->pixel = s->pixel;
    A->target_rows = s->target_rows; A->target_ld = s->target_ld; A->action = s->action; A->restart = s->restart;
    A->rotation = s->rotation; A->thrust = s->thrust; A->pixel_velocity = s->pixel_velocity; A->limited = s->limited;
    A->visible = s->visible; A->throttle = s->throttle; A->n = n;
    return FPV_OK;
}

}  // namespace

int fpv_pns_guide(fpv_handle_t h, const fpv_buffers_t* b, const fpv_pns_t* s, void* stream)
{
    if (fpv_pns_kernel_fn == nullptr) return fail(FPV_EINVAL, kPnsAbsent);
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (!b || !s) return fail(FPV_EINVAL, "null argument");
    if (h->mode != FPV_MODE_DRONE) return fail(FPV_EINVAL, "point and shoot is the Drone's guidance law: not for a Racer handle");
    if (h->K.flags & FPV_FLAG_FP16_STATE)
        return fail(FPV_EINVAL, "point and shoot cannot read fp16 state (FPV_FLAG_FP16_STATE): a reader of the packed quaternion is the follow-up");
    if (!b->state) return fail(FPV_EINVAL, "fpv_buffers_t.state is null");
    if (b->ld < h->n) return fail(FPV_EALIGN, "fpv_buffers_t.ld is smaller than the number of drones");
    FpvPnsArgs A;
    const int rc = pns_args(s, h->n, &A);
    if (rc != FPV_OK) return rc;
    A.state = b->state; A.ld = b->ld;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    void* arg = &A;
    return launch_args("point and shoot kernel launch", fpv_pns_kernel_fn(s->pixel != nullptr), blocks_for(h->n, kStepBlock), dim3(kStepBlock), (hipStream_t)stream, &arg);
}

int fpv_pns_eval(const fpv_pns_t* s, int64_t n, const float* p, const float* v, const float* q)
{
    if (fpv_pns_eval_host == nullptr) return fail(FPV_EINVAL, kPnsAbsent);
    if (!v) return fail(FPV_EINVAL, "null argument");
    int rc = check_eval_args(s, n, p, q);
    if (rc != FPV_OK) return rc;
    FpvPnsArgs A;
    rc = pns_args(s, n, &A);
    if (rc != FPV_OK) return rc;
    fpv_pns_eval_host(&A, p, v, q);
    return FPV_OK;
}

int fpv_boxes_derive(const fpv_objects_t* objects, const double* ground_size, const fpv_gate_t* gates, int gate_count, int gate_resolution,
                     fpv_boxes_t* out)
{
    if (!out) return fail(FPV_EINVAL, "null argument");
    if (gate_count < 0 || (gate_count > 0 && !gates)) return fail(FPV_EINVAL, "gates is null or gate_count negative");
    int rc = check_object_count(objects, true);
    if (rc != FPV_OK) return rc;
    if (gate_count > FPV_MAX_GATES || (objects ? objects->count : 0) + gate_count > FPV_MAX_BOXES)
        return fail(FPV_EPARAM, "a box table has at most " + std::to_string(FPV_MAX_OBJECTS) + " objects and " + std::to_string(FPV_MAX_GATES) + " gates");
    if (gate_resolution < 1 || gate_resolution > 4096) return fail(FPV_EPARAM, "gate_resolution must be 1..4096");
    int bad = -1;
    const char* why = "";
    memset(out, 0, sizeof(*out));
    rc = fpv_detect_derive_boxes(objects, ground_size, gates, gate_count, gate_resolution, out, &bad, &why);
    return rc == FPV_OK ? FPV_OK : fail(rc, "box " + std::to_string(bad) + ": " + why);
}

int fpv_detect_derive(const fpv_camera_t* camera, fpv_detect_t* out)
{
    if (!camera || !out) return fail(FPV_EINVAL, "null argument");
    fpv_chase_t c;
    const int rc = fpv_chase_derive(camera, &c);
    if (rc != FPV_OK) return rc;
    out->width = c.width; out->height = c.height; out->focal_length = c.focal_length;
    memcpy(out->relative_rotation, c.relative_rotation, sizeof c.relative_rotation);
    memcpy(out->relative_position, c.relative_position, sizeof c.relative_position);
    return FPV_OK;
}

namespace {

const char kDetectAbsent[] = "object detections are not in this build (the library was linked without csrc/fpv_detect.hip)";

// the uniform constants of a call, its box table and its buffers, checked (n: the drones the buffers must hold): FPV_OK or the error
int detect_args(const fpv_detect_t* s, int64_t n, FpvDetectArgs* A)
{
    if (s->struct_size != sizeof(fpv_detect_t)) return fail(FPV_EINVAL, "fpv_detect_t.struct_size does not match this library");
    if (s->width < 1 || s->width > FPV_CHASE_MAX_SIDE || s->height < 1 || s->height > FPV_CHASE_MAX_SIDE)
        return fail(FPV_EPARAM, "width and height must be 1..16384 pixels (the camera numbers come from fpv_detect_derive)");
    if (!isfinite(s->focal_length) || !(s->focal_length > 0.0)) return fail(FPV_EPARAM, "focal_length must be finite and positive (fpv_detect_derive)");
    for (int k = 0; k < 9; ++k)
        if (!isfinite(s->relative_rotation[k])) return fail(FPV_EPARAM, "relative_rotation is not finite");
    for (int k = 0; k < 3; ++k)
        if (!isfinite(s->relative_position[k])) return fail(FPV_EPARAM, "relative_position is not finite");
    if (s->pixel_mode != FPV_DETECT_INT && s->pixel_mode != FPV_DETECT_FLOAT) return fail(FPV_EINVAL, "unknown pixel mode");
    const int table = s->table ? s->table->count : 0;
    const int count = table + (s->target_rows ? 1 : 0);
    if (table < 0 || count < 1 || count > FPV_MAX_BOXES)
        return fail(FPV_EINVAL, "count: a detection has 1.." + std::to_string(FPV_MAX_BOXES) + " boxes, not " + std::to_string(count));
    for (int m = 0; m < table; ++m) {
        const float* b = s->table->box[m];
        for (int a = 0; a < 6; ++a)
            if (!isfinite(b[a])) return fail(FPV_EPARAM, "box " + std::to_string(m) + " is not finite");
        for (int a = 0; a < 3; ++a)
            if (b[a] > b[3 + a]) return fail(FPV_EPARAM, "box " + std::to_string(m) + " has min > max");
    }
    if (!s->boxes || !s->box_depth || !s->box_visible) return fail(FPV_EINVAL, "fpv_detect_t.boxes, box_depth or box_visible is null");
    if (((uintptr_t)s->boxes & 3) || ((uintptr_t)s->box_depth & 3)) return fail(FPV_EALIGN, "boxes and box_depth must be 4-byte aligned");
    if (s->ld < n) return fail(FPV_EALIGN, "fpv_detect_t.ld is smaller than the number of drones");
    if (s->ld % 4) return fail(FPV_EALIGN, "fpv_detect_t.ld must be a multiple of 4");
    if (s->target_rows) {
        if (((uintptr_t)s->target_rows & 3) || ((uintptr_t)s->target_radius & 3)) return fail(FPV_EALIGN, "target_rows and target_radius must be 4-byte aligned");
        if (s->target_ld < n) return fail(FPV_EALIGN, "fpv_detect_t.target_ld is smaller than the number of drones");
        if (!s->target_radius && (!isfinite(s->target_radius_all) || !(s->target_radius_all >= 0.0f)))
            return fail(FPV_EPARAM, "target_radius_all must be finite and not negative");
    }
    memset(A, 0, sizeof(*A));
    FpvDetectK& K = A->K;
    for (int k = 0; k < 9; ++k) K.rr[k] = (float)s->relative_rotation[k];
    for (int k = 0; k < 3; ++k) K.rel[k] = (float)s->relative_position[k];
    K.f = (float)s->focal_length; K.cx = (float)(s->width / 2.0); K.cy = (float)(s->height / 2.0);
    K.w = (float)s->width; K.h = (float)s->height;
    K.tr = s->target_rows && !s->target_radius ? s->target_radius_all : 0.0f;
    K.trunc = s->pixel_mode == FPV_DETECT_INT; K.clip = s->clip != 0;
    if (table) memcpy(A->box, s->table->box, sizeof(float) * 6 * (size_t)table);
    A->count = count; A->table_count = table;
    A->target_rows = s->target_rows; A->target_ld = s->target_ld; A->target_radius = s->target_rows ? s->target_radius : nullptr;
    A->boxes = s->boxes; A->depth = s->box_depth; A->visible = s->box_visible; A->out_ld = s->ld; A->n = n;
    return FPV_OK;
}

}  // namespace

int fpv_detect_boxes(fpv_handle_t h, const fpv_buffers_t* b, const fpv_detect_t* s, void* stream)
{
    if (fpv_detect_kernel_fn == nullptr) return fail(FPV_EINVAL, kDetectAbsent);
    if (!s) return fail(FPV_EINVAL, "null argument");
    FpvDetectArgs A;
    int rc = detect_args(s, h ? h->n : 1, &A);             // the struct first: what it refuses needs no device
    if (rc != FPV_OK) return rc;
    if (!h) {
        int devices = 0;
        const hipError_t e = hipGetDeviceCount(&devices);
        if (e != hipSuccess || devices < 1) return fail(FPV_ENODEV, "no HIP device: detections run on the GPU only (fpv_detect_eval is the host function)");
    }
    rc = check_sensor(h, b, s, true, "object detection", "fpv_detect");
    if (rc != FPV_OK) return rc;
    A.state = b->state; A.ld = b->ld;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    void* arg = &A;
    const dim3 grid((unsigned)((h->n + kStepBlock - 1) / kStepBlock), (unsigned)((A.count + FPV_DETECT_GROUP - 1) / FPV_DETECT_GROUP));
    return launch_args("detection kernel launch", fpv_detect_kernel_fn(s->target_rows != nullptr), grid, dim3(kStepBlock), (hipStream_t)stream, &arg);
}

int fpv_detect_eval(const fpv_detect_t* s, int64_t n, const float* p, const float* q)
{
    if (fpv_detect_eval_host == nullptr) return fail(FPV_EINVAL, kDetectAbsent);
    int rc = check_eval_args(s, n, p, q);
    if (rc != FPV_OK) return rc;
    FpvDetectArgs A;
    rc = detect_args(s, n, &A);
    if (rc != FPV_OK) return rc;
    fpv_detect_eval_host(&A, p, q);
    return FPV_OK;
}

int fpv_splat_derive(const fpv_camera_t* camera, fpv_splat_t* out)
{
    if (!camera || !out) return fail(FPV_EINVAL, "null argument");
    if (camera->width < 4 || camera->width > FPV_DEPTH_MAX_SIDE || camera->height < 4 || camera->height > FPV_DEPTH_MAX_SIDE)
        return fail(FPV_EPARAM, "width and height must be 4..128 pixels: the z-buffer of a drone is an LDS image");
    if (camera->width % 4) return fail(FPV_EPARAM, "width must be a multiple of 4");
    fpv_chase_t c;
    const int rc = fpv_chase_derive(camera, &c);
    if (rc != FPV_OK) return rc;
    out->width = c.width; out->height = c.height; out->focal_length = c.focal_length;
    memcpy(out->relative_rotation, c.relative_rotation, sizeof c.relative_rotation);
    memcpy(out->relative_position, c.relative_position, sizeof c.relative_position);
    return FPV_OK;
}

int fpv_cloud_derive(int kind, const double* numbers, const int32_t* resolutions, float* out_points, int64_t ld)
{
    if (!numbers || !resolutions) return fail(FPV_EINVAL, "null argument");
    if (kind < FPV_CLOUD_GROUND || kind > FPV_CLOUD_GATE) return fail(FPV_EINVAL, "unknown cloud kind");
    const int nn = kind == FPV_CLOUD_GROUND ? 1 : kind == FPV_CLOUD_CYLINDER ? 5 : 13;
    for (int k = 0; k < nn; ++k)
        if (!isfinite(numbers[k])) return fail(FPV_EPARAM, "the numbers of a cloud must be finite");
    if (kind == FPV_CLOUD_GATE && (resolutions[0] < FPV_GATE_RECTANGLE || resolutions[0] > FPV_GATE_HALF_CIRCLE)) return fail(FPV_EPARAM, "unknown gate shape");
    const int nr = kind == FPV_CLOUD_GROUND ? 1 : 2;
    for (int k = kind == FPV_CLOUD_GATE ? 1 : 0; k < nr; ++k)
        if (resolutions[k] < 1 || resolutions[k] > FPV_SPLAT_MAX_POINTS) return fail(FPV_EPARAM, "a resolution must be 1..2^20");
    const int64_t count = fpv_cloud_points(kind, numbers, resolutions, nullptr, 0);
    if (count > FPV_SPLAT_MAX_POINTS) return fail(FPV_EPARAM, "a cloud has at most 2^20 points");
    if (!out_points) return (int)count;
    if (ld < count) return fail(FPV_EALIGN, "ld is smaller than the number of points");
    if (ld % 4) return fail(FPV_EALIGN, "ld must be a multiple of 4");
    if ((uintptr_t)out_points & 3) return fail(FPV_EALIGN, "out_points must be 4-byte aligned");
    return (int)fpv_cloud_points(kind, numbers, resolutions, out_points, ld);
}

namespace {

const char kSplatAbsent[] = "the point-cloud camera is not in this build (the library was linked without csrc/fpv_splat.hip)";

// the uniform constants of a call, its object tables and its buffers, checked: FPV_OK or the error
int splat_args(const fpv_splat_t* s, int64_t n, FpvSplatArgs* A)
{
    if (s->struct_size != sizeof(fpv_splat_t)) return fail(FPV_EINVAL, "fpv_splat_t.struct_size does not match this library");
    if (s->width < 4 || s->width > FPV_DEPTH_MAX_SIDE || s->height < 4 || s->height > FPV_DEPTH_MAX_SIDE)
        return fail(FPV_EPARAM, "width and height must be 4..128 pixels (the camera numbers come from fpv_splat_derive)");
    if (s->width % 4) return fail(FPV_EPARAM, "width must be a multiple of 4");
    if (!isfinite(s->focal_length) || !(s->focal_length > 0.0)) return fail(FPV_EPARAM, "focal_length must be finite and positive (fpv_splat_derive)");
    for (int k = 0; k < 9; ++k)
        if (!isfinite(s->relative_rotation[k])) return fail(FPV_EPARAM, "relative_rotation is not finite");
    for (int k = 0; k < 3; ++k)
        if (!isfinite(s->relative_position[k])) return fail(FPV_EPARAM, "relative_position is not finite");
    if (s->encoding != FPV_SPLAT_METRES && s->encoding != FPV_SPLAT_U8 && s->encoding != FPV_SPLAT_MASK) return fail(FPV_EINVAL, "unknown encoding");
    if (!isfinite(s->max_depth) || !(s->max_depth > 0.0f)) return fail(FPV_EPARAM, "max_depth must be finite and positive");
    const int M = s->object_count;
    if (M < 0 || M > FPV_MAX_BOXES) return fail(FPV_EINVAL, "object_count: a cloud has 0.." + std::to_string(FPV_MAX_BOXES) + " objects, not " + std::to_string(M));
    if (s->first[0] != 0) return fail(FPV_EPARAM, "first[0] must be 0");
    for (int m = 0; m < M; ++m) {
        if (s->first[m + 1] < s->first[m]) return fail(FPV_EPARAM, "first is not non-decreasing at object " + std::to_string(m));
        if (s->first[m + 1] > FPV_SPLAT_MAX_POINTS) return fail(FPV_EPARAM, "first is past 2^20 points at object " + std::to_string(m));
        for (int a = 0; a < 6; ++a)
            if (!isfinite(s->box[m][a])) return fail(FPV_EPARAM, "box " + std::to_string(m) + " is not finite");
        for (int a = 0; a < 3; ++a) {
            if (s->box[m][a] > s->box[m][3 + a]) return fail(FPV_EPARAM, "box " + std::to_string(m) + " has min > max");
            if (!isfinite(s->offset[m][a])) return fail(FPV_EPARAM, "offset " + std::to_string(m) + " is not finite");
        }
    }
    const int32_t total = s->first[M];
    if (total > 0 && !s->points) return fail(FPV_EINVAL, "fpv_splat_t.points is null");
    if ((uintptr_t)s->points & 3) return fail(FPV_EALIGN, "points must be 4-byte aligned");
    if (s->point_ld < total) return fail(FPV_EALIGN, "point_ld is smaller than the number of points");
    if (s->point_ld % 4) return fail(FPV_EALIGN, "point_ld must be a multiple of 4");
    if (!s->image) return fail(FPV_EINVAL, "fpv_splat_t.image is null");
    if ((uintptr_t)s->image & 3) return fail(FPV_EALIGN, "image must be 4-byte aligned");
    if (s->image_ld < (int64_t)s->width * s->height) return fail(FPV_EALIGN, "image_ld is smaller than width * height");
    if (s->image_ld % 4) return fail(FPV_EALIGN, "image_ld must be a multiple of 4 elements");
    if ((s->centroid == nullptr) != (s->lit == nullptr)) return fail(FPV_EINVAL, "centroid and lit are given together or not at all");
    if (((uintptr_t)s->centroid & 3) || ((uintptr_t)s->lit & 3)) return fail(FPV_EALIGN, "centroid and lit must be 4-byte aligned");
    if (n > 0x7fffffff) return fail(FPV_EINVAL, "more than 2^31 - 1 drones (a workgroup each): render the population in parts");
    memset(A, 0, sizeof(*A));
    FpvDetectK& K = A->K;
    for (int k = 0; k < 9; ++k) K.rr[k] = (float)s->relative_rotation[k];
    for (int k = 0; k < 3; ++k) K.rel[k] = (float)s->relative_position[k];
    K.f = (float)s->focal_length; K.cx = (float)(s->width / 2.0); K.cy = (float)(s->height / 2.0);
    K.w = (float)s->width; K.h = (float)s->height;
    K.trunc = 1; K.clip = 0;
    A->max_depth = s->max_depth; A->encoding = s->encoding; A->width = s->width; A->height = s->height; A->count = M;
    memcpy(A->first, s->first, sizeof(int32_t) * (size_t)(M + 1));
    if (M) { memcpy(A->offset, s->offset, sizeof(float) * 3 * (size_t)M); memcpy(A->box, s->box, sizeof(float) * 6 * (size_t)M); }
    A->points = s->points; A->point_ld = s->point_ld; A->image = s->image; A->image_ld = s->image_ld;
    A->centroid = s->centroid; A->lit = s->lit; A->n = n;
    return FPV_OK;
}

}  // namespace

int fpv_splat_render(fpv_handle_t h, const fpv_buffers_t* b, const fpv_splat_t* s, void* stream)
{
    if (fpv_splat_kernel_fn == nullptr) return fail(FPV_EINVAL, kSplatAbsent);
    if (!s) return fail(FPV_EINVAL, "null argument");
    FpvSplatArgs A;
    int rc = splat_args(s, h ? h->n : 1, &A);              // the struct first: what it refuses needs no device
    if (rc != FPV_OK) return rc;
    if (!h) {
        int devices = 0;
        const hipError_t e = hipGetDeviceCount(&devices);
        if (e != hipSuccess || devices < 1) return fail(FPV_ENODEV, "no HIP device: the point-cloud camera renders on the GPU only (fpv_splat_eval is the host function)");
    }
    rc = check_sensor(h, b, s, true, "point-cloud camera", "fpv_splat");
    if (rc != FPV_OK) return rc;
    A.state = b->state; A.ld = b->ld;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    void* arg = &A;
    const size_t lds = sizeof(uint32_t) * (size_t)s->width * (size_t)s->height;      // the z-buffer: at most 64 KiB
    (void)hipLaunchKernel(fpv_splat_kernel_fn(), dim3((unsigned)h->n), dim3(FPV_SPLAT_BLOCK), &arg, lds, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPV_OK : hip_fail(e, "point-cloud render launch");
}

int fpv_splat_eval(const fpv_splat_t* s, int64_t n, const float* p, const float* q)
{
    if (fpv_splat_eval_host == nullptr) return fail(FPV_EINVAL, kSplatAbsent);
    int rc = check_eval_args(s, n, p, q);
    if (rc != FPV_OK) return rc;
    FpvSplatArgs A;
    rc = splat_args(s, n, &A);
    if (rc != FPV_OK) return rc;
    fpv_splat_eval_host(&A, p, q);
    return FPV_OK;
}

int fpv_pursuit_derive(int32_t resolution, float* circle_out_host)
{
    if (!circle_out_host) return fail(FPV_EINVAL, "null argument");
    if (resolution < 1 || resolution > FPV_PURSUIT_MAX_RESOLUTION)
        return fail(FPV_EPARAM, "path_resolution must be 1.." + std::to_string(FPV_PURSUIT_MAX_RESOLUTION) + ", not " + std::to_string(resolution));
    // numpy.linspace(0, 2 pi, K + 1)[:-1] (helper_functions.py:152): theta_j = j * (2 pi / K)
    const double step = 2.0 * M_PI / (double)resolution;
    for (int32_t j = 0; j < resolution; ++j) {
        circle_out_host[2 * j] = (float)cos((double)j * step);
        circle_out_host[2 * j + 1] = (float)sin((double)j * step);
    }
    return FPV_OK;
}

namespace {

const char kPursuitAbsent[] = "the pursuit task is not in this build (the library was linked without csrc/fpv_pursuit.hip)";

// the constants of the respawn draw, checked: what fpv_pursuit_sample needs and the first part of pursuit_args
int pursuit_spawn(const fpv_pursuit_t* s, FpvPursuitK* P)
{
    if (s->struct_size != sizeof(fpv_pursuit_t)) return fail(FPV_EINVAL, "fpv_pursuit_t.struct_size does not match this library");
    if (s->path_resolution < 1 || s->path_resolution > FPV_PURSUIT_MAX_RESOLUTION)
        return fail(FPV_EPARAM, "path_resolution must be 1.." + std::to_string(FPV_PURSUIT_MAX_RESOLUTION) + ", not " + std::to_string(s->path_resolution));
    memset(P, 0, sizeof(*P));
    for (int k = 0; k < 4; ++k) {
        const double lo = k < 3 ? s->spawn_lo[k] : s->radius_lo, hi = k < 3 ? s->spawn_hi[k] : s->radius_hi;
        if (!isfinite(lo) || !isfinite(hi)) return fail(FPV_EPARAM, k < 3 ? "the spawn box is not finite" : "the radius range is not finite");
        if (hi < lo) return fail(FPV_EPARAM, k < 3 ? "the spawn box has hi < lo" : "the radius range has hi < lo");
        P->lo[k] = (float)lo; P->span[k] = (float)(hi - lo);
    }
    if (s->radius_lo < 0.0) return fail(FPV_EPARAM, "a target's radius must not be negative");
    P->seed_lo = (uint32_t)s->spawn_seed; P->seed_hi = (uint32_t)(s->spawn_seed >> 32);
    P->resolution = (uint32_t)s->path_resolution;
    return FPV_OK;
}

// the uniform constants of a call and its buffers, checked (n: the drones the buffers must hold; gid: the first drone's global id;
// reward: the cells add_to_reward adds to, not read by a reset call): FPV_OK or the error
int pursuit_args(const fpv_pursuit_t* s, int64_t n, uint64_t gid, float* reward, bool reset, FpvPursuitArgs* A)
{
    FpvPursuitK P;
    int rc = pursuit_spawn(s, &P);
    if (rc != FPV_OK) return rc;
    const double four[4] = {s->dt, s->capture_distance, s->progress, s->capture};
    const char* const names[4] = {"dt", "capture_distance", "progress", "capture"};
    for (int k = 0; k < 4; ++k)
        if (!isfinite(four[k])) return fail(FPV_EPARAM, std::string(names[k]) + " is not finite");
    if (!(s->dt > 0.0)) return fail(FPV_EPARAM, "dt must be positive");
    if (s->capture_distance < 0.0) return fail(FPV_EPARAM, "capture_distance must not be negative");
    if (!s->targets) return fail(FPV_EINVAL, "fpv_pursuit_t.targets is null");
    if (!s->circle) return fail(FPV_EINVAL, "fpv_pursuit_t.circle is null");
    if (s->targets_ld < n) return fail(FPV_EALIGN, "fpv_pursuit_t.targets_ld is smaller than the number of drones");
    if ((uintptr_t)s->targets & 15) return fail(FPV_EALIGN, "targets must be 16-byte aligned");
    if ((uintptr_t)s->circle & 7) return fail(FPV_EALIGN, "circle must be 8-byte aligned");
    if (((uintptr_t)s->obs & 3) || ((uintptr_t)s->position & 3) || ((uintptr_t)s->reward_out & 3)) return fail(FPV_EALIGN, "obs, position and reward_out must be 4-byte aligned");
    if (s->obs && s->obs_ld < n) return fail(FPV_EALIGN, "fpv_pursuit_t.obs_ld is smaller than the number of drones");
    if (s->position && s->position_ld < n) return fail(FPV_EALIGN, "fpv_pursuit_t.position_ld is smaller than the number of drones");
    if (!reset && s->add_to_reward && !reward) return fail(FPV_EINVAL, "add_to_reward needs fpv_buffers_t.reward");
    memset(A, 0, sizeof(*A));
    if (s->guide) {
        FpvChaseArgs C;
        fpv_chase_t g = *s->guide;
        g.target[0] = g.target[1] = g.target[2] = 0.0f; g.target_radius = 0.0f; g.pixel = nullptr;     // ignored: not checked
        rc = chase_args(&g, n, &C);
        if (rc != FPV_OK) return rc;
        A->K = C.K; A->pid_state = C.pid_state; A->pid_ld = C.pid_ld; A->rotation = C.rotation; A->thrust = C.thrust;
        A->pixel_out = C.pixel_out; A->visible = C.visible;
    }
    P.dt = (float)s->dt; P.capture_distance = (float)s->capture_distance; P.progress = (float)s->progress; P.capture = (float)s->capture;
    P.gid_lo = (uint32_t)gid; P.gid_hi = (uint32_t)(gid >> 32);
    P.advance = s->advance != 0; P.respawn_on_done = s->respawn_on_done != 0; P.add_to_reward = s->add_to_reward != 0;
    A->P = P;
    A->targets = s->targets; A->tld = s->targets_ld; A->circle = s->circle; A->obs = s->obs; A->obs_ld = s->obs_ld;
    A->position = s->position; A->pos_ld = s->position_ld; A->event = s->event; A->reward_out = s->reward_out; A->n = n;
    return FPV_OK;
}

int pursuit_launch(fpv_handle_t h, const fpv_buffers_t* b, const fpv_pursuit_t* s, const uint8_t* flags, bool reset, void* stream)
{
    if (fpv_pursuit_kernel_fn == nullptr) return fail(FPV_EINVAL, kPursuitAbsent);
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (!b || !s) return fail(FPV_EINVAL, "null argument");
    if (h->mode != FPV_MODE_DRONE) return fail(FPV_EINVAL, "the pursuit task is the Drone's chase: not for a Racer handle");
    if (h->K.flags & FPV_FLAG_FP16_STATE)
        return fail(FPV_EINVAL, "the pursuit task cannot read fp16 state (FPV_FLAG_FP16_STATE): a reader of the packed quaternion is the follow-up");
    if (!b->state) return fail(FPV_EINVAL, "fpv_buffers_t.state is null");
    if (b->ld < h->n) return fail(FPV_EALIGN, "fpv_buffers_t.ld is smaller than the number of drones");
    FpvPursuitArgs A;
    const int rc = pursuit_args(s, h->n, ((uint64_t)h->K.noise.id_hi << 32) | h->K.noise.id_lo, b->reward, reset, &A);
    if (rc != FPV_OK) return rc;
    A.state = b->state; A.ld = b->ld; A.done = flags;
    if (!reset && s->add_to_reward) { A.reward = b->reward; A.ep_return = b->ep_return; }
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    void* arg = &A;
    return launch_args("pursuit kernel launch", fpv_pursuit_kernel_fn(s->guide != nullptr, reset), blocks_for(h->n, kStepBlock), dim3(kStepBlock),
                       (hipStream_t)stream, &arg);
}

}  // namespace

int fpv_pursuit_sample(const fpv_pursuit_t* s, uint64_t global_id, uint32_t respawn_index, float out[4], uint32_t* phase_out)
{
    if (!s || !out || !phase_out) return fail(FPV_EINVAL, "null argument");
    FpvPursuitK P;
    const int rc = pursuit_spawn(s, &P);
    if (rc != FPV_OK) return rc;
    fpv_pursuit_draw(P, global_id, respawn_index & 0xffffu, out, out[3], *phase_out);
    return FPV_OK;
}

int fpv_pursuit_step(fpv_handle_t h, const fpv_buffers_t* b, const fpv_pursuit_t* s, void* stream)
{
    return pursuit_launch(h, b, s, b ? b->done : nullptr, false, stream);
}

int fpv_pursuit_reset(fpv_handle_t h, const fpv_buffers_t* b, const fpv_pursuit_t* s, const uint8_t* mask, void* stream)
{
    return pursuit_launch(h, b, s, mask, true, stream);
}

int fpv_pursuit_eval(const fpv_pursuit_t* s, int64_t n, uint64_t drone_id_offset, const float* p, const float* v, const float* q,
                     const uint8_t* done_or_mask, float* reward, int reset)
{
    if (fpv_pursuit_eval_host == nullptr) return fail(FPV_EINVAL, kPursuitAbsent);
    if (!v) return fail(FPV_EINVAL, "null argument");
    int rc = check_eval_args(s, n, p, q);
    if (rc != FPV_OK) return rc;
    FpvPursuitArgs A;
    rc = pursuit_args(s, n, drone_id_offset, reward, reset != 0, &A);
    if (rc != FPV_OK) return rc;
    A.done = done_or_mask;
    if (!reset && s->add_to_reward) A.reward = reward;
    fpv_pursuit_eval_host(&A, p, v, q, s->guide != nullptr, reset);
    return FPV_OK;
}

int fpv_create(const fpv_params_t* params, int64_t n, int device, fpv_handle_t* out)
{
    if (!params || !out) return fail(FPV_EINVAL, "null argument");
    *out = nullptr;
    if (n <= 0) return fail(FPV_EINVAL, "n must be positive");
    if (n > FPV_MAX_DRONES) return fail(FPV_EINVAL, "n exceeds 2^28 drones per handle (32-bit lane byte offsets into 16-byte action rows); split the population over handles");
    FpvK K;
    FpvResetJitter J;
    const char* why = "";
    const int rc = derive(params, &K, &J, &why);
    if (rc != FPV_OK) return fail(rc, why);
    const int drc = check_device_index(device);
    if (drc != FPV_OK) return drc;
    fpv_env* h = new (std::nothrow) fpv_env;
    if (!h) return fail(FPV_EINVAL, "out of host memory");
    h->K = K; h->rj = J; h->P = *params; h->n = n; h->device = device; h->mode = (int)params->mode;
    h->launches = 0;
    const int mrc = device_cache_model(device, &h->cache);
    if (mrc != FPV_OK) { delete h; return mrc; }
    update_rotation(h);
    *out = h;
    return FPV_OK;
}

void fpv_destroy(fpv_handle_t h)
{
    if (!h) return;
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->graph) (void)hipGraphDestroy(h->graph);
    delete h;
}

int fpv_set_params(fpv_handle_t h, const fpv_params_t* params)
{
    if (!h || !params) return fail(FPV_EINVAL, "null argument");
    if ((int)params->mode != h->mode) return fail(FPV_EINVAL, "mode cannot change on a live handle (state layout differs)");
    if ((params->flags ^ h->P.flags) & (FPV_FLAG_FP16_STATE | FPV_FLAG_STICK_NOISE))
        return fail(FPV_EINVAL, "FPV_FLAG_FP16_STATE / FPV_FLAG_STICK_NOISE cannot change on a live handle (buffer layout differs)");
    FpvK K;
    FpvResetJitter J;
    const char* why = "";
    const int rc = derive(params, &K, &J, &why);
    if (rc != FPV_OK) return fail(rc, why);
    h->K = K; h->rj = J; h->P = *params;
    return FPV_OK;
}

int fpv_set_rotation(fpv_handle_t h, int64_t drones)
{
    if (!h) return fail(FPV_EINVAL, "null handle");
    if (drones < -1) return fail(FPV_EINVAL, "fpv_set_rotation: -1 = automatic, 0 = plain order, > 0 = drones the start moves back per launch");
    h->rot_request = drones;
    update_rotation(h);
    h->graph_shape_key.clear();         // a cached graph carries the starts of the old setting: rebuilt at its next use
    return FPV_OK;
}

int fpv_get_rotation(fpv_handle_t h, int64_t* drones)
{
    if (!h || !drones) return fail(FPV_EINVAL, "null argument");
    *drones = h->rot_blocks * kStepBlock;
    // the plain order because the device is not the model's: the reason is the call's message (the call itself succeeds)
    if (h->rot_request < 0 && !h->cache.matches) g_err = h->cache.reason;
    return FPV_OK;
}

int fpv_check_cache_model(const char* arch, int compute_units, int64_t l2_bytes_per_xcd, fpv_cache_model_t* out)
{
    if (!arch || !out) return fail(FPV_EINVAL, "null argument");
    check_cache_model(arch, compute_units, l2_bytes_per_xcd, out);
    return FPV_OK;
}

int fpv_device_cache_model(int device, fpv_cache_model_t* out)
{
    if (!out) return fail(FPV_EINVAL, "null argument");
    const int rc = check_device_index(device);
    if (rc != FPV_OK) return rc;
    return device_cache_model(device, out);
}

int fpv_get_cache_model(fpv_handle_t h, fpv_cache_model_t* out)
{
    if (!h || !out) return fail(FPV_EINVAL, "null argument");
    *out = h->cache;
    return FPV_OK;
}

int fpv_reset_pose_sample(const fpv_params_t* params, uint64_t global_id, uint64_t step, int explicit_reset,
                          const float base[10], float out[10])
{
    if (!params || !base || !out) return fail(FPV_EINVAL, "null argument");
    FpvK K;
    FpvResetJitter J;
    const char* why = "";
    const int rc = derive(params, &K, &J, &why);
    if (rc != FPV_OK) return fail(rc, why);
    for (int r = 0; r < 10; ++r) out[r] = base[r];
    if (K.flags & FPV_FLAG_RESET_JITTER) fpv_reset_jitter(J, global_id, step, explicit_reset ? 1u : 0u, out);
    return FPV_OK;
}

int fpv_set_step_counter(fpv_handle_t h, uint64_t step)
{
    if (!h) return fail(FPV_EINVAL, "null handle");
    h->launches = step;
    return FPV_OK;
}

int fpv_get_step_counter(fpv_handle_t h, uint64_t* step)
{
    if (!h || !step) return fail(FPV_EINVAL, "null argument");
    *step = h->launches;
    return FPV_OK;
}

int64_t fpv_recommended_ld_device(int64_t n, int device)
{
    if (n <= 0) return fail(FPV_EINVAL, "n must be positive");
    fpv_cache_model_t m;
    const int rc = fpv_device_cache_model(device, &m);
    if (rc != FPV_OK) return rc;
    return m.matches ? fpv_recommended_ld(n) : conservative_ld(n);
}

int64_t fpv_recommended_ld(int64_t n)
{
    if (n <= 0) return fail(FPV_EINVAL, "n must be positive");
    int64_t ld = conservative_ld(n);
    if (n <= kL2ModelFromDrones) return ld;
    // Larger populations: a stride of 1 KiB past a multiple of 2 KiB (ld = 256 mod 512 floats) is the best or within 1 % of the
    // best of the eight 256-byte classes at every size measured from 2^18 to 2^23 drones, ragged ones included (2 000 000 drones:
    // 37.3 us against 38.3 us for the stride that only keeps clear of 8 KiB; 3 000 000: 55.4 against 57.3) ...
    ld = (n + 255) / 512 * 512 + 256;
    // ... except where it makes the rows of a drone block meet in the same L2 sets (l2_set_overflow: 2^19 drones, 3 * 2^19).
    // That matters while the L2s hold a good part of the state (up to 2^21 drones); beyond, the loss of the L2 share and the
    // stride's gain on the memory side cancel (5 * 2^19 drones: 50.0 against 50.7 us).
    if (n > kL2ModelToDrones) return ld;
    const int64_t blocks = std::min<int64_t>(step_grid(n), kL2Bytes / 64 * 61 / (4 * FPV_DRONE_ROWS + 5) / kStepBlock / 8 * 8);
    double best = l2_set_overflow(4 * ld, blocks);
    if (best < kL2OverflowOk) return ld;
    int64_t best_ld = ld;
    for (int k = 1; k <= 3; ++k)
        for (int sign = 1; sign >= -1; sign -= 2) {
            const int64_t c = ld + sign * 64 * k;            // never a multiple of 512 floats (k <= 3)
            if (c < n || c % 2048 < 256) continue;        // (the 8 KiB rule above stays)
            const double o = l2_set_overflow(4 * c, blocks);
            if (o < kL2OverflowOk) return c;
            if (o < best) { best = o; best_ld = c; }
        }
    return best_ld;
}

int fpv_reset(fpv_handle_t h, const fpv_buffers_t* b, const uint8_t* mask, const float* position,
              const float* velocity, const float* ypr_deg, void* stream)
{
    int rc = check_buffers(h, b, false);
    if (rc != FPV_OK) return rc;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    FpvBufD d = to_device_view(h, b);
    d.step = h->launches;                // the jitter of an explicit reset is keyed by the handle's step counter
    rc = launch("reset kernel launch", fpv_reset_kernel, blocks_for(h->n, kBlock), dim3(kBlock), (hipStream_t)stream, h->K, d,
                h->mode, mask, position, velocity, ypr_deg, h->n);
    if (rc != FPV_OK || !h->gates) return rc;
    // a gate course: the words of the same lanes, after the state on the same stream
    return launch("gate word reset launch", reinterpret_cast<GateResetKernel>(fpv_gate_reset_kernel_fn()), blocks_for(h->n, kBlock), dim3(kBlock),
                  (hipStream_t)stream, h->ga.word, mask, h->ga.start, h->ga.K.count, h->n);
}

int fpv_step(fpv_handle_t h, const fpv_buffers_t* b, void* stream)
{
    int rc = check_buffers(h, b, true);
    if (rc != FPV_OK) return rc;
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    const FpvBufD d = to_device_view(h, b);
    return launch_step(h, plan_launch(h, d), d, (hipStream_t)stream);
}

namespace {

void drop_graph(fpv_env* h)
{
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    if (h->graph) { (void)hipGraphDestroy(h->graph); h->graph = nullptr; }
    h->graph_nodes.clear();
    h->graph_shape_key.clear();
    h->graph_ptr_key.clear();
}

// step t's device view of a k-step call (fpv_rollout's launches, fpv_rollout_graph's nodes); a null action (stick noise) stays null
FpvBufD graph_step_view(const fpv_buffers_t* b, const FpvBufD& d0, int t, int64_t action_stride, int64_t out_stride)
{
    FpvBufD d = d0;
    if (b->action) d.action = reinterpret_cast<const float4*>(b->action + (int64_t)t * action_stride);
    if (out_stride) {
        if (b->reward) d.reward = b->reward + (int64_t)t * out_stride;
        if (b->done) d.done = b->done + (int64_t)t * out_stride;
    }
    if (b->done_bits) d.done_bits = reinterpret_cast<unsigned long long*>(b->done_bits) + (int64_t)t * b->done_bits_stride;
    return d;
}

}  // namespace

int fpv_rollout(fpv_handle_t h, const fpv_buffers_t* b, int k, int64_t action_stride, int64_t out_stride,
                void* stream)
{
    int rc = check_buffers(h, b, true);
    if (rc != FPV_OK) return rc;
    if (k < 0) return fail(FPV_EINVAL, "k must be >= 0");
    if (action_stride % 4) return fail(FPV_EALIGN, "action_stride must keep 16-byte alignment");
    if (b->rotation_override) return fail(FPV_EINVAL, "the guidance override is a per-step input: use fpv_step");
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    const FpvBufD d0 = to_device_view(h, b);
    const Plan p = plan_launch(h, d0);
    for (int t = 0; t < k; ++t)
        if ((rc = launch_step(h, p, graph_step_view(b, d0, t, action_stride, out_stride), (hipStream_t)stream)) != FPV_OK) return rc;
    return FPV_OK;
}

int fpv_diag_stream_copy(float* dst, const float* src, int64_t n_floats, void* stream)
{
    if (!dst || !src || n_floats <= 0) return fail(FPV_EINVAL, "bad argument");
    return launch("diag copy launch", fpv_diag_copy_kernel, blocks_for(n_floats, kBlock), dim3(kBlock), (hipStream_t)stream, dst, src, n_floats);
}

int fpv_diag_stream_copy_wide(float* dst, const float* src, int64_t n_floats, void* stream)
{
    if (!dst || !src || n_floats <= 0) return fail(FPV_EINVAL, "bad argument");
    if (n_floats % 4 || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15)) return fail(FPV_EALIGN, "n_floats must be a multiple of 4 and both pointers 16-byte aligned");
    const int64_t n4 = n_floats / 4;
    return launch("diag wide copy launch", fpv_diag_copy4_kernel, blocks_for(n4, kBlock), dim3(kBlock), (hipStream_t)stream,
                  reinterpret_cast<fpv_v4f*>(dst), reinterpret_cast<const fpv_v4f*>(src), n4);
}

int fpv_diag_xcd_map(uint32_t* xcd_of_block, int64_t blocks, void* stream)
{
    if (!xcd_of_block || blocks <= 0 || blocks > ((int64_t)1 << 24)) return fail(FPV_EINVAL, "fpv_diag_xcd_map: need a device buffer and 0 < blocks <= 2^24");
    return launch("diag xcd-map launch", fpv_diag_xcd_kernel, dim3((unsigned)blocks), dim3(kStepBlock), (hipStream_t)stream, xcd_of_block);
}

int fpv_diag_busy(double microseconds, void* stream)
{
    if (!(microseconds > 0.0) || microseconds > 1000.0) return fail(FPV_EINVAL, "fpv_diag_busy: 0 < microseconds <= 1000");
    // wall_clock64 ticks at the device's constant wall-clock rate (hipDeviceAttributeWallClockRate, kHz): asked, not assumed
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
        khz = 100000;
    const unsigned long long ticks = (unsigned long long)(microseconds * (double)khz * 1e-3);
    // one s_sleep(32) is 32 x 64 clocks ~ 1 us at 2 GHz: the iteration cap is ~4x the requested time
    return launch("diag busy launch", fpv_diag_busy_kernel, dim3(1), dim3(64), (hipStream_t)stream, ticks, (int)(microseconds * 4.0) + 64);
}

int fpv_step_n(fpv_handle_t h, const fpv_buffers_t* b, int k, int64_t action_stride, int64_t out_stride, void* stream)
{
    int rc = check_buffers(h, b, true);
    if (rc != FPV_OK) return rc;
    if (k < 0) return fail(FPV_EINVAL, "k must be >= 0");
    if (k == 0) return FPV_OK;
    if (action_stride % 4) return fail(FPV_EALIGN, "action_stride must keep 16-byte alignment");
    if (b->obs_aos) return fail(FPV_EINVAL, "fpv_step_n does not write obs_aos rows (a per-step observation is a closed-loop need: use fpv_step)");
    if (b->action_ld) return fail(FPV_EINVAL, "fpv_step_n reads action rows [n][4] only (SoA sticks are a policy's per-step output, a closed-loop need: use fpv_step or fpv_rollout)");
    if (b->rotation_override) return fail(FPV_EINVAL, "the guidance override is a per-step input: use fpv_step");
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    const FpvBufD d = to_device_view(h, b);
    return launch_roll(h, plan_launch(h, d), d, FpvRoll{k, 0, action_stride, out_stride, b->done_bits_stride}, (hipStream_t)stream, "k-step kernel launch");
}

int fpv_rollout_graph(fpv_handle_t h, const fpv_buffers_t* b, int k, int64_t action_stride, int64_t out_stride,
                      void* stream)
{
    int rc = check_buffers(h, b, true);
    if (rc != FPV_OK) return rc;
    if (k <= 0) return fail(FPV_EINVAL, "k must be positive");
    if (action_stride % 4) return fail(FPV_EALIGN, "action_stride must keep 16-byte alignment");
    if (b->rotation_override) return fail(FPV_EINVAL, "the guidance override is a per-step input: use fpv_step");
    const FpvBufD d0 = to_device_view(h, b);
    const Plan p = plan_launch(h, d0);
    // not replayed (plan_launch says why): the call is the other entry point's, with that one's own refusals and device guard
    if (p.graph == kToStepN) return fpv_step_n(h, b, k, action_stride, out_stride, stream);
    if (p.graph == kToRollout) return fpv_rollout(h, b, k, action_stride, out_stride, stream);
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    const std::string shape = bytes_of(p.step, step_grid(h->n), h->n, p.ground, FpvRoll{k, 0, action_stride, out_stride, b->done_bits_stride}, h->K, d0.ld,
                                       d0.action_ld, d0.wx, d0.wy, d0.wz, d0.seed, d0.objs, d0.rj, h->phys, h->phys_ld, h->ga);
    const std::string ptrs = bytes_of(d0);
    // node t starts where launch_step would after t launches, counted from the first node (a replay begins where the previous one
    // began: one launch in k starts on cold rows)
    const int64_t nblk = step_grid(h->n), rot = rotation_blocks(h, &d0);
    const auto start = [&](int t) { return rot > 0 ? (int64_t)(((uint64_t)t * (uint64_t)(nblk - rot % nblk)) % (uint64_t)nblk) : 0; };
    if (!h->graph_exec || shape != h->graph_shape_key) {
        drop_graph(h);
        hipError_t e = hipGraphCreate(&h->graph, 0);
        if (e != hipSuccess) { drop_graph(h); return hip_fail(e, "hipGraphCreate"); }
        hipGraphNode_t prev = nullptr;
        for (int t = 0; t < k; ++t) {
            const StepLaunch g(h, p, graph_step_view(b, d0, t, action_stride, out_stride), start(t));
            hipGraphNode_t node;
            e = hipGraphAddKernelNode(&node, h->graph, prev ? &prev : nullptr, prev ? 1 : 0, &g.np);
            if (e != hipSuccess) { drop_graph(h); return hip_fail(e, "hipGraphAddKernelNode"); }
            h->graph_nodes.push_back(node);
            prev = node;
        }
        e = hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0);
        if (e != hipSuccess) { drop_graph(h); return hip_fail(e, "hipGraphInstantiate"); }
        h->graph_shape_key = shape;
        h->graph_ptr_key = ptrs;
    } else if (ptrs != h->graph_ptr_key) {
        // same shape, new buffers (e.g. a fresh actions tensor every call): patch the node arguments
        for (int t = 0; t < k; ++t) {
            const StepLaunch g(h, p, graph_step_view(b, d0, t, action_stride, out_stride), start(t));
            const hipError_t e = hipGraphExecKernelNodeSetParams(h->graph_exec, h->graph_nodes[(size_t)t], &g.np);
            if (e != hipSuccess) { drop_graph(h); return hip_fail(e, "hipGraphExecKernelNodeSetParams"); }
        }
        h->graph_ptr_key = ptrs;
    }
    const hipError_t e = hipGraphLaunch(h->graph_exec, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipGraphLaunch");
    launched(h, p, k);
    return FPV_OK;
}

int fpv_widen_state(fpv_handle_t h, const fpv_buffers_t* b, float* out, int64_t out_ld, void* stream)
{
    if (!h || !b || !b->state || !out) return fail(FPV_EINVAL, "null argument");
    if (h->mode != FPV_MODE_DRONE || !(h->K.flags & FPV_FLAG_FP16_STATE) || !b->state_h)
        return fail(FPV_EINVAL, "fpv_widen_state is for FPV_FLAG_FP16_STATE handles (fp32 state is already fp32 rows)");
    if (b->ld < h->n || out_ld < h->n) return fail(FPV_EALIGN, "ld / out_ld smaller than the number of drones");
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    const uint16_t* thrust = b->state_h_thrust ? b->state_h_thrust : b->state_h + (int64_t)2 * FPV_HALF_PAIR_ROWS * b->ld;
    return launch("widen kernel launch", fpv_widen_state_kernel, blocks_for(h->n, kBlock), dim3(kBlock), (hipStream_t)stream,
                  b->state, b->state_h, thrust, b->ld, out, out_ld, h->n);
}

int fpv_return_triple(fpv_handle_t h, const fpv_buffers_t* b, float* rt, float* gyro, float* acc, void* stream)
{
    if (!h || !b || !b->state || !rt || !gyro) return fail(FPV_EINVAL, "null argument");
    if (h->mode != FPV_MODE_DRONE || (h->K.flags & FPV_FLAG_FP16_STATE))
        return fail(FPV_EINVAL, "fpv_return_triple reads the fp32 drone state (Drone.step's return value)");
    if (b->ld < h->n) return fail(FPV_EALIGN, "fpv_buffers_t.ld is smaller than the number of drones");
    if (acc && !b->accel) return fail(FPV_EINVAL, "R @ acceleration needs fpv_buffers_t.accel (the step kernel writes it there)");
    const DeviceGuard dev(h->device);
    if (dev.rc != FPV_OK) return dev.rc;
    return launch("return-triple kernel launch", fpv_return_triple_kernel, blocks_for(h->n, kBlock), dim3(kBlock), (hipStream_t)stream,
                  b->state, b->ld, b->accel, rt, gyro, acc, h->n);
}

int fpv_pid_reset(float* pid_state, int64_t ld, int64_t n, const uint8_t* mask, int device, void* stream)
{
    if (!pid_state) return fail(FPV_EINVAL, "pid_state is null");
    if (n <= 0 || ld < n) return fail(FPV_EINVAL, "need 0 < n <= ld");
    const int rc = check_device_index(device);
    if (rc != FPV_OK) return rc;
    const DeviceGuard dev(device);
    if (dev.rc != FPV_OK) return dev.rc;
    return launch("pid reset kernel launch", fpv_pid_reset_kernel, blocks_for(n, kBlock), dim3(kBlock), (hipStream_t)stream, pid_state, ld, n, mask);
}

int fpv_pid_call(const fpv_pid_params_t* params, float* pid_state, int64_t ld, int64_t n, const float* current,
                 const float* target, float target_scalar, float* out, float* error_out, int device, void* stream)
{
    if (!params || !pid_state || !current || !out) return fail(FPV_EINVAL, "null argument");
    if (params->struct_size != sizeof(fpv_pid_params_t)) return fail(FPV_EINVAL, "fpv_pid_params_t.struct_size does not match this library");
    if (n <= 0 || ld < n) return fail(FPV_EINVAL, "need 0 < n <= ld");
    if (!(params->dt > 0)) return fail(FPV_EPARAM, "dt must be positive");
    if (!(params->integral_clip >= 0) || !(params->min_output <= params->max_output)
        || !(params->derivative_transition_rate >= 0 && params->derivative_transition_rate <= 1))
        return fail(FPV_EPARAM, "components.PID constants: integral_clip >= 0, min_output <= max_output, derivative_transition_rate in [0, 1]");
    const int rc = check_device_index(device);
    if (rc != FPV_OK) return rc;
    const DeviceGuard dev(device);
    if (dev.rc != FPV_OK) return dev.rc;
    FpvPidK<float> P;
    memset(&P, 0, sizeof(P));
    P.dt = (float)params->dt; P.inv_dt = (float)(1.0 / params->dt);
    P.gain[0][0] = (float)params->kP; P.gain[0][1] = (float)params->kI; P.gain[0][2] = (float)params->kD;
    P.integral_clip = (float)params->integral_clip; P.min_output = (float)params->min_output; P.max_output = (float)params->max_output;
    P.d_rate = (float)params->derivative_transition_rate; P.om_d_rate = (float)(1.0 - params->derivative_transition_rate);
    return launch("pid kernel launch", fpv_pid_kernel, blocks_for(n, kBlock), dim3(kBlock), (hipStream_t)stream,
                  P, pid_state, ld, n, current, target, target_scalar, out, error_out);
}

// ---- RCCL, opened at run time ------------------------------------------------------------------------------
namespace {
struct NcclId { char internal[FPV_COMM_ID_BYTES]; };          // = ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES 128)
typedef void* NcclComm;
enum { kNcclSuccess = 0, kNcclUint64 = 5, kNcclFloat32 = 7 };   // rccl.h: ncclResult_t / ncclDataType_t values
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(NcclId*) = nullptr;
    int (*CommInitRank)(NcclComm*, int, NcclId, int) = nullptr;
    int (*CommDestroy)(NcclComm) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, NcclComm, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int*) = nullptr;
    std::string why;
};

// Opened once per process, under std::call_once: two host threads (one per GPU) may call fpv_comm_* at the same
// time.  The table is filled in a local and published whole; a failure leaves lib == nullptr and `why` set.
Rccl* rccl()
{
    static Rccl R;
    static std::once_flag once;
    std::call_once(once, [] {
        Rccl T;
        const char* env = getenv("FPV_RCCL_PATH");
        if (env && *env) T.lib = dlopen(env, RTLD_NOW | RTLD_LOCAL);
        // reuse a copy the process already has (PyTorch links its own as "librccl.so"), else load the system one
        if (!T.lib) T.lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
        if (!T.lib) T.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!T.lib) T.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!T.lib) T.lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!T.lib) {
            const char* msg = dlerror();
            T.why = std::string("librccl not found: ") + (msg ? msg : "dlopen failed without a message");
        } else {
            T.GetUniqueId = reinterpret_cast<int (*)(NcclId*)>(dlsym(T.lib, "ncclGetUniqueId"));
            T.CommInitRank = reinterpret_cast<int (*)(NcclComm*, int, NcclId, int)>(dlsym(T.lib, "ncclCommInitRank"));
            T.CommDestroy = reinterpret_cast<int (*)(NcclComm)>(dlsym(T.lib, "ncclCommDestroy"));
            T.AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, NcclComm, hipStream_t)>(dlsym(T.lib, "ncclAllGather"));
            T.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(T.lib, "ncclGetErrorString"));
            T.GetVersion = reinterpret_cast<int (*)(int*)>(dlsym(T.lib, "ncclGetVersion"));
            if (!T.GetUniqueId || !T.CommInitRank || !T.CommDestroy || !T.AllGather) {
                T.why = "librccl lacks the ncclGetUniqueId/CommInitRank/CommDestroy/AllGather symbols";
                T.lib = nullptr;
            }
        }
        R = T;
    });
    return &R;
}

int rccl_fail(int rc, const char* what)
{
    Rccl* R = rccl();
    return fail(FPV_EHIP, std::string(what) + ": " + (R->GetErrorString ? R->GetErrorString(rc) : "RCCL error ") + " (" + std::to_string(rc) + ")");
}
}  // namespace

struct fpv_comm {
    NcclComm comm;
    int world, rank, device;
};

int fpv_comm_unique_id(uint8_t id[FPV_COMM_ID_BYTES])
{
    if (!id) return fail(FPV_EINVAL, "null id");
    Rccl* R = rccl();
    if (!R->lib) return fail(FPV_EHIP, R->why);
    NcclId u;
    const int rc = R->GetUniqueId(&u);
    if (rc != kNcclSuccess) return rccl_fail(rc, "ncclGetUniqueId");
    memcpy(id, u.internal, FPV_COMM_ID_BYTES);
    return FPV_OK;
}

int fpv_comm_create(const uint8_t id[FPV_COMM_ID_BYTES], int world_size, int rank, int device, fpv_comm_t* out)
{
    if (!id || !out) return fail(FPV_EINVAL, "null argument");
    *out = nullptr;
    if (world_size <= 0 || rank < 0 || rank >= world_size) return fail(FPV_EINVAL, "need 0 <= rank < world_size");
    Rccl* R = rccl();
    if (!R->lib) return fail(FPV_EHIP, R->why);
    int rc = check_device_index(device);
    if (rc != FPV_OK) return rc;
    const DeviceGuard dev(device);
    if (dev.rc != FPV_OK) return dev.rc;
    NcclId u;
    memcpy(u.internal, id, FPV_COMM_ID_BYTES);
    NcclComm c = nullptr;
    rc = R->CommInitRank(&c, world_size, u, rank);
    if (rc != kNcclSuccess) return rccl_fail(rc, "ncclCommInitRank");
    fpv_comm* h = new (std::nothrow) fpv_comm;
    if (!h) { (void)R->CommDestroy(c); return fail(FPV_EINVAL, "out of host memory"); }
    h->comm = c; h->world = world_size; h->rank = rank; h->device = device;
    *out = h;
    return FPV_OK;
}

int fpv_comm_info(fpv_comm_t c, int* world_size, int* rank, int* rccl_version)
{
    if (!c) return fail(FPV_EINVAL, "null communicator");
    if (world_size) *world_size = c->world;
    if (rank) *rank = c->rank;
    if (rccl_version) {
        *rccl_version = 0;
        Rccl* R = rccl();
        if (R->lib && R->GetVersion) (void)R->GetVersion(rccl_version);
    }
    return FPV_OK;
}

void fpv_comm_destroy(fpv_comm_t c)
{
    if (!c) return;
    Rccl* R = rccl();
    if (R->lib && c->comm) (void)R->CommDestroy(c->comm);
    delete c;
}

namespace {
int allgather(fpv_comm_t c, const void* send, void* recv, int64_t count, int dtype, void* stream)
{
    if (!c || !send || !recv) return fail(FPV_EINVAL, "null argument");
    if (count <= 0) return fail(FPV_EINVAL, "count per rank must be positive");
    Rccl* R = rccl();
    if (!R->lib) return fail(FPV_EHIP, R->why);
    const DeviceGuard dev(c->device);
    if (dev.rc != FPV_OK) return dev.rc;
    const int rc = R->AllGather(send, recv, (size_t)count, dtype, c->comm, (hipStream_t)stream);
    if (rc != kNcclSuccess) return rccl_fail(rc, "ncclAllGather");
    return FPV_OK;
}
}  // namespace

int fpv_allgather_done(fpv_comm_t c, const uint64_t* send_bits, uint64_t* recv_bits, int64_t words_per_rank, void* stream)
{
    return allgather(c, send_bits, recv_bits, words_per_rank, kNcclUint64, stream);
}

int fpv_allgather_f32(fpv_comm_t c, const float* send, float* recv, int64_t count_per_rank, void* stream)
{
    return allgather(c, send, recv, count_per_rank, kNcclFloat32, stream);
}

const char* fpv_last_error(void) { return g_err.c_str(); }

const char* fpv_encoding_id(int which)
{
    return which == 0 ? FPV_STATE_H_ENCODING_ID : which == 1 ? FPV_NOISE_GENERATOR_ID : nullptr;
}

const char* fpv_error_name(int code)
{
    switch (code) {
        case FPV_OK: return "FPV_OK";
        case FPV_EINVAL: return "FPV_EINVAL";
        case FPV_EHIP: return "FPV_EHIP";
        case FPV_ENODEV: return "FPV_ENODEV";
        case FPV_EALIGN: return "FPV_EALIGN";
        case FPV_EPARAM: return "FPV_EPARAM";
        default: return "FPV_E?";
    }
}

}  // extern "C"
