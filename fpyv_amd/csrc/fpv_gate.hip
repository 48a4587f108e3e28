// fpv_gate.hip - the gfx950 kernels of gate courses (include/fpv_abi.h "Gate courses").
//
// A handle with a course flies a race: every drone carries one 32-bit word (next gate, the event of the step just executed, gates
// passed) that the step kernels load with the state and store with it.  The physics is fpv_math.h's lane function, called
// unchanged; the gate function (fpv_gate.h fpv_gate_step, the one the host's fpv_gate_eval runs) follows it on the position the
// step loaded and the position it produced - three more live VGPRs and no second pass over the state.  Reward and done are the
// race's (progress towards the next gate, pass / finish bonus, miss / crash penalty; FINISH and, on request, MISS end the
// episode), and six optional write-only rows tell a policy where its next gate is in the body frame.
//
// A translation unit of its own, linked with fpv_hip.hip and fpv_phys.hip into the one libfpv_hip.so: their kernels stay exactly
// as they are, and fpv_hip.hip alone still builds (it reaches the three lookup functions at the end of this file through weak
// declarations).  Five kernels: the plain single-step kernel, the k-step kernel <NOISE, OBJ> without / with stick noise / with
// the object list, and the word reset of fpv_reset.  A handle with stick noise, an object list or a reset source runs its single
// steps on the k-step kernel (k = 1), as reset sources do without a course (fpv_hip.hip: plan_launch).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_math.h"
#include "fpv_gate.h"
#include "fpv_kernels.h"

namespace {

constexpr bool kGateLds = FPV_EXP_GATE_LDS != 0;

// the workgroup's copy of the descriptor table (FPV_EXP_GATE_LDS, the shipped form of the single-step kernel): every thread of the workgroup reaches the barrier - the lanes of a ragged last
// block too, which leave only after it.  At most FPV_MAX_GATES rows, whatever the argument says: the array holds no more.
__device__ __forceinline__ void stage_gate_table(fpv_gate_v4* lds, const fpv_gate_v4* __restrict__ tab, uint32_t count)
{
    const uint32_t groups = (count < (uint32_t)FPV_MAX_GATES ? count : (uint32_t)FPV_MAX_GATES) * FPV_GATE_GROUPS;
    for (uint32_t r = threadIdx.x; r < groups; r += kStepBlock) lds[r] = tab[r];
    __syncthreads();
}

// the six observation rows of a lane: write-only, with the streaming hint like the accel rows (they do not count among the
// written bytes of the rotation rule)
__device__ __forceinline__ void st_gate_obs(float* __restrict__ obs, int64_t ld, uint32_t j, const FpvGateCN& cn, const FpvDroneState& s)
{
    float ob[6];
    fpv_gate_obs(cn, s.q, s.px, s.py, s.pz, ob);
#pragma unroll
    for (int r = 0; r < 6; ++r) ST_OUT(row_at(ROW(obs, r, ld), j), ob[r]);
}

// the kernel-argument segment of the single-step gate kernel (FpvStepArgs, then the course) and a fresh opaque view of it: what
// fpv_step_args_again is for the sectioned kernels of fpv_hip.hip - the course's constants and the store section's uniforms are
// loaded where they are used instead of living in SGPRs across the physics
struct FpvGateStepArgs { FpvStepArgs S; FpvGateArgs G; };
__device__ __forceinline__ const FpvGateStepArgs& fpv_gate_step_args_again()
{
    typedef const __attribute__((address_space(4))) FpvGateStepArgs* P4;
    P4 p = (P4)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const FpvGateStepArgs*)p;
}

// One step with a course: fpv_drone_step_kernel<false, false> (fpv_hip.hip; read the comments above FPV_STEP_PARAMS there) with
// the word load in its load block and the gate function after the lane function.  The leading scalars are FPV_STEP_PARAMS' with
// the word base in the slot of state_h - a gate handle has no fp16 state -, so all six are preloaded into SGPRs and the word load
// goes out first, ahead of the 15 state and stick loads.  The workgroup stages the descriptor table into LDS next to those
// loads - one barrier, which the lanes of a ragged last block reach too - and each lane reads its gate's row by index (shipped:
// faster than the per-lane global gather in every measurement, profiles/exp_gate_table_access.log; -DFPV_EXP_GATE_LDS=0 builds the
// gather).  The traversal rotates like every single-step kernel's (the word row counts among the written bytes).
__global__ __launch_bounds__(kStepBlock) void fpv_drone_step_gate_kernel(float* __restrict__ a_state, const int64_t a_ld,
                                                                         const float4* __restrict__ a_action, const int64_t a_action_ld,
                                                                         uint32_t* __restrict__ a_word, const int64_t n_start,
                                                                         const FpvK K, const FpvBufD B_, const FpvGateArgs GA)
{
    const FpvBufD B = fpv_step_view(B_, a_state, a_ld, a_action, a_action_ld, nullptr);
    __shared__ fpv_gate_v4 gtab[kGateLds ? FPV_MAX_GATES * FPV_GATE_GROUPS : 1];
    FPV_STEP_INDEX;
    const bool live = i < n;
    if (!kGateLds && !live) return;
    FpvDroneState s;
    uint32_t word;
    float4 a;
    // ---- 1. every load of this lane before the first use, the word first
    const fpv_gate_v4* tab = GA.tab;
    if (kGateLds) {
        // (a lane past the end loads drone 0's rows and leaves after the barrier)
        const uint32_t il = live ? i : 0u;
        word = row_at(a_word, il);
        a = ld_action_any(B.action, B.action_ld, il);
        ld_drone(B.state, B.ld, il, s);
        stage_gate_table(gtab, GA.tab, GA.K.count);
        if (!live) return;
        tab = gtab;
    } else {
        word = row_at(a_word, i);
        a = ld_action_any(B.action, B.action_ld, i);
        ld_drone(B.state, B.ld, i, s);
    }
    __builtin_amdgcn_sched_barrier(0);       // vector loads first, the scalar loads of the uniform constants after (fpv_drone_step_kernel)
    const uint32_t g = fpv_gate_index(word, GA.K.count);
    FpvGateCN cn = fpv_gate_cn(tab + g * FPV_GATE_GROUPS);
    // ---- 2. the physics, unchanged, then the race on the position it started from (the course's constants through a view of
    // their own: they are not alive during the physics)
    const float pox = s.px, poy = s.py, poz = s.pz;
    const FpvStepOut o = fpv_drone_step_lane<false>(K, s, a.x, a.y, a.z, a.w, B.wx, B.wy, B.wz, &B_.objs);
    const FpvGateArgs& GR = fpv_gate_step_args_again().G;
    FpvGateOut go = fpv_gate_step<true>(GR.K, cn, (kGateLds ? gtab : GR.tab) + g * FPV_GATE_GROUPS, word, pox, poy, poz, s.px, s.py, s.pz, o.done);
    // ---- 3. the stores: the addresses are formed only now, and the uniforms come through a fresh view
    uint32_t j = i;
    FPV_KEEP_HERE(j);
    const FpvGateStepArgs& E = fpv_gate_step_args_again();
    const FpvGateArgs& GE = E.G;
    FpvBufD Be = E.S.B;
    Be.state = E.S.state; Be.ld = E.S.ld;
    if (Be.accel) {
        ST_OUT(row_at(ROW(Be.accel, 0, Be.ld), j), o.ax); ST_OUT(row_at(ROW(Be.accel, 1, Be.ld), j), o.ay); ST_OUT(row_at(ROW(Be.accel, 2, Be.ld), j), o.az);
    }
    if ((E.S.K.flags & FPV_FLAG_AUTO_RESET) && go.done) {
        fpv_drone_reset_lane(E.S.K, s);
        go.word = fpv_gate_word_reset(go.word, GE.start ? (uint32_t)GE.start[j] : 0u, GE.K.count);      // (the start gate: read by lanes that reset only)
    }
    if (GE.obs) {
        // the gate that is next now: the one the step tested, unless the lane passed it or was reset (rare: its c and n are read then)
        uint32_t h = fpv_gate_index(go.word, GE.K.count);
        if (FPV_WAVE_ANY(h != g)) {
            FPV_KEEP_HERE(h);
            cn = fpv_gate_cn((kGateLds ? gtab : GE.tab) + h * FPV_GATE_GROUPS);
        }
        st_gate_obs(GE.obs, GE.obs_ld, j, cn, s);
    }
    st_drone(Be.state, Be.ld, j, s);
    row_at(reinterpret_cast<uint32_t*>(E.S.state_h), j) = go.word;
    emit_outputs(Be, j, true, go.reward, go.done);
}

// a fresh, opaque view of a k-step gate kernel's arguments (fpv_args_again for FpvRollGateArgs)
__device__ __forceinline__ const FpvRollGateArgs& fpv_gate_args_again()
{
    typedef const __attribute__((address_space(4))) FpvRollGateArgs* P4;
    P4 p = (P4)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const FpvRollGateArgs*)p;
}

// k steps with a course in ONE launch: fpv_drone_rollout_kernel<NOISE, OBJ, false, false> (fpv_hip.hip) with the word loaded once
// before the loop and held in a VGPR for all k steps, and with it the centre and normal of the lane's next gate (six VGPRs, read
// again only when a lane of the wave passes its gate or resets).  The gate logic runs on every step, quiet ones included; the
// reward only on steps whose outputs are stored, the observation rows once, after the last step.  It carries the reset-source
// branch (reset-pose table, jitter), so a handle with per-drone starts AND a course runs here, its single steps included (k = 1).
// Sections and argument views as in fpv_drone_rollout_kernel: the views read FpvRollArgs at the head of the kernel-argument
// segment, which is where FpvRollGateArgs keeps it.
template <bool NOISE, bool OBJ>
__global__ __launch_bounds__(kStepBlock) void fpv_drone_rollout_gate_kernel(const FpvRollGateArgs PA)
{
    const FpvRollArgs& A = PA.A;
    __shared__ FpvNormalRow ntab[NOISE ? FPV_NTAB_ROWS : 1];
    if (NOISE) stage_normal_table(ntab);
    const uint32_t i = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;
    if (i >= A.n) return;
    FpvDroneState s;
    const int k = A.R.k;
    const bool has_action = !NOISE || A.B.action;
    float4 a_next = make_float4(0.f, 0.f, 0.f, 0.f);
    float ns[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t word = row_at(PA.G.word, i);
    if (has_action) a_next = ld_action_any(A.B.action, A.B.action_ld, i);
    ld_drone(A.B.state, A.B.ld, i, s);
    if (NOISE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ns[c] = row_at(ROW(A.B.noise_state, c, A.B.ld), i);
    }
    // the descriptor rows are gathered from global memory here (FPV_EXP_GATE_LDS is the single-step kernel's question: this
    // kernel reads a row once before the loop and again only when a lane passes its gate or resets)
    const fpv_gate_v4* tab = PA.G.tab;
    FpvGateCN cn = fpv_gate_cn(tab + fpv_gate_index(word, PA.G.K.count) * FPV_GATE_GROUPS);
    fpv_settle(s.px); fpv_settle(s.py); fpv_settle(s.pz); fpv_settle(s.vx); fpv_settle(s.vy); fpv_settle(s.vz);
    fpv_settle(s.q.w); fpv_settle(s.q.x); fpv_settle(s.q.y); fpv_settle(s.q.z);
    fpv_settle(s.rx); fpv_settle(s.ry); fpv_settle(s.rz); fpv_settle(s.thrust);
    fpv_settle(cn.cx); fpv_settle(cn.cy); fpv_settle(cn.cz); fpv_settle(cn.nx); fpv_settle(cn.ny); fpv_settle(cn.nz);
    if (NOISE) { fpv_settle(ns[0]); fpv_settle(ns[1]); fpv_settle(ns[2]); fpv_settle(ns[3]); }
    float av[4] = {0.f, 0.f, 0.f, 0.f};

    auto one_step = [&](const FpvRollGateArgs& W, const FpvObjects* objs, const float* ap_next, bool prefetch, int t, auto quiet_c) -> FpvStepOut {
        constexpr bool QUIET = decltype(quiet_c)::value;
        const FpvRollArgs& V = W.A;
        av[0] = a_next.x; av[1] = a_next.y; av[2] = a_next.z; av[3] = a_next.w;
        if ((!NOISE || has_action) && (QUIET || prefetch)) a_next = ld_action(reinterpret_cast<const float4*>(ap_next), i);
        if (NOISE) {
            const FpvRollArgs& NV = OBJ ? fpv_args_again() : V;
            FpvNoiseK N = NV.K.noise;
            asm volatile("" : "+s"(N.seed_lo), "+s"(N.seed_hi));
            fpv_stick_noise(N, NV.B.step + (uint64_t)t, (uint64_t)i, ntab, ns, av);
        }
        const float pox = s.px, poy = s.py, poz = s.pz;
        FpvStepOut o = fpv_drone_step_lane<OBJ, !QUIET, false>(V.K, s, av[0], av[1], av[2], av[3], V.B.wx, V.B.wy, V.B.wz, objs);
        // the race: the lane's next gate before the step, its c and n from registers, the rest of its row only on a crossing
        const uint32_t g = fpv_gate_index(word, W.G.K.count);
        const FpvGateOut go = fpv_gate_step<!QUIET>(W.G.K, cn, tab + g * FPV_GATE_GROUPS, word, pox, poy, poz, s.px, s.py, s.pz, o.done);
        word = go.word; o.done = go.done; o.reward = go.reward;
        if ((V.K.flags & FPV_FLAG_AUTO_RESET) && o.done) {
            // rare: the reset pose and the start gate come through views of their own, inside the branch
            const FpvRollArgs& Z = fpv_args_again();
            fpv_drone_reset_lane(Z.K, s);
            apply_reset_source_k(i, (uint64_t)t, s);
            const FpvGateArgs& ZG = fpv_gate_args_again().G;
            const uint8_t* st = ZG.start;
            word = fpv_gate_word_reset(word, st ? (uint32_t)st[i] : 0u, ZG.K.count);
        }
        uint32_t h = word & 0xffu;
        if (FPV_WAVE_ANY(h != g)) {
            // rare: a lane of the wave passed its gate or went back to its start gate
            FPV_KEEP_HERE(h);
            cn = fpv_gate_cn(tab + fpv_gate_index(h, fpv_gate_args_again().G.K.count) * FPV_GATE_GROUPS);
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
            const FpvStepOut o = one_step(PA, &A.B.objs, ap, true, t, std::true_type{});
            if (bp) {
                const unsigned long long mask = __ballot(o.done);
                if ((threadIdx.x & 63) == 0) bp[i >> 6] = mask;
                bp += bstride;
            }
            ++t;
        };
        while (t < k - 1) quiet_step();
    }
    // ---- 2. the remaining steps, with every output the caller asked for
    FpvStepOut o;
    o.done = false; o.reward = 0.0f; o.ax = o.ay = o.az = 0.0f;
    {
        const FpvRollGateArgs& GW = fpv_gate_args_again();
        const FpvRollArgs& G = GW.A;
        RollOut out(G.B, G.R, i, true);
        if (out.bp) out.bp += (int64_t)t * G.R.bits_stride;
        const float* ap = reinterpret_cast<const float*>(G.B.action) + (int64_t)t * G.R.action_stride;
        const int kk = G.R.k;
        if (out.track) { fpv_settle(out.ep_r); fpv_settle(__int_as_float(out.ep_l)); }
        for (; t < kk; ++t) {
            ap += G.R.action_stride;
            o = one_step(GW, &G.B.objs, ap, G.R.action_stride != 0 && t + 1 < kk, t, std::false_type{});
            out.template step<false>(i, t, o.reward, o.done);
        }
        out.finish(i, fpv_args_again().B);
    }
    // ---- 3. the stores
    const FpvRollGateArgs& EW = fpv_gate_args_again();
    const FpvRollArgs& E = EW.A;
    uint32_t j = i;
    asm volatile("" : "+v"(j));
    if (E.B.accel) {
        ST_OUT(row_at(ROW(E.B.accel, 0, E.B.ld), j), o.ax); ST_OUT(row_at(ROW(E.B.accel, 1, E.B.ld), j), o.ay); ST_OUT(row_at(ROW(E.B.accel, 2, E.B.ld), j), o.az);
    }
    if (EW.G.obs) st_gate_obs(EW.G.obs, EW.G.obs_ld, j, cn, s);
    st_drone(E.B.state, E.B.ld, j, s);
    row_at(EW.G.word, j) = word;
    if (NOISE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) row_at(ROW(E.B.noise_state, c, E.B.ld), j) = ns[c];
        if (E.B.action_out) E.B.action_out[j] = make_float4(av[0], av[1], av[2], av[3]);
    }
}

// fpv_reset on a gate handle: the words of the masked lanes (all without a mask) go back to "nothing passed, at the start gate";
// launched after fpv_hip.hip's reset kernel on the same stream
__global__ __launch_bounds__(kBlock) void fpv_gate_reset_kernel(uint32_t* __restrict__ word, const uint8_t* __restrict__ mask,
                                                                const uint8_t* __restrict__ start, const uint32_t count, const int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    word[i] = fpv_gate_word_reset(word[i], start ? (uint32_t)start[i] : 0u, count);
}

typedef void (*GateRollFn)(const FpvRollGateArgs);
// [stick noise][object list]; the two together have no kernel (the host refuses the combination by name)
const GateRollFn kGateRoll[2][2] = {{fpv_drone_rollout_gate_kernel<false, false>, fpv_drone_rollout_gate_kernel<false, true>},
                                    {fpv_drone_rollout_gate_kernel<true, false>, nullptr}};

}  // namespace

// what fpv_hip.hip launches (it declares these three weak)
extern "C" __attribute__((visibility("hidden"))) void* fpv_gate_step_kernel(void)
{
    return reinterpret_cast<void*>(fpv_drone_step_gate_kernel);
}

extern "C" __attribute__((visibility("hidden"))) void* fpv_gate_roll_kernel(int noise, int obj)
{
    return reinterpret_cast<void*>(kGateRoll[noise != 0][obj != 0]);
}

extern "C" __attribute__((visibility("hidden"))) void* fpv_gate_reset_kernel_fn(void)
{
    return reinterpret_cast<void*>(fpv_gate_reset_kernel);
}
