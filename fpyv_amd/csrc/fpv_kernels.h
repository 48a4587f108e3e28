// fpv_kernels.h - what the gfx950 kernels of more than one translation unit share (fpv_hip.hip, fpv_phys.hip): the device view of
// the buffers, row addressing, the state loads / stores, the output and episode bookkeeping, the stick-noise staging, the leading
// preloaded scalars of the single-step kernels and the argument views of the k-step kernels.  Everything lives in an unnamed
// namespace: each unit gets its own copy, and every function here is inlined into its kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "../../include/fpv_abi.h"
#include "fpv_addr.h"
#include "fpv_exp.h"
#include "fpv_math.h"
#include "fpv_gate.h"

namespace {

constexpr int kBlock = 256;   // reset / pid / diag kernels: 4 wave64 per workgroup
// step and k-step kernels: 128-thread workgroups (2 wave64), the fastest of 64/128/256/512/1024 in every measurement
// (profiles/archive/r01_exp10_shapes_clean.log, r02_sweep_geometry.log); fpv_exp.h: -DFPV_EXP_BLOCK=N rebuilds them all for an A/B
constexpr int kStepBlock = FPV_EXP_BLOCK;
static_assert(kStepBlock % 64 == 0 && kStepBlock >= 64 && kStepBlock <= 1024, "whole wave64s");

struct FpvBufD {
    float* state;
    int64_t ld;
    const float4* action;
    float* reward;
    uint8_t* done;
    unsigned long long* done_bits;
    float* accel;
    float* ep_return;
    int32_t* ep_length;
    float* last_return;
    int32_t* last_length;
    float wx, wy, wz;
    float* obs_aos;        // [n][16] row-major observation (p3 v3 q4 rates3 accel3) or null
    float* pos_comp;       // [6][ld] Kahan compensation of p and v, or null
    float* noise_state;    // FPV_FLAG_STICK_NOISE: [4][ld] EMA stick-noise state
    float4* action_out;    // [n] applied action or null
    uint64_t step;         // 64-bit step index of this launch (the handle's launch counter): Philox counter words 2, 3
    int64_t action_ld;     // 0: action is [n][4] rows; > 0: action is [4][action_ld] SoA (a GEMM's [4, n] output)
    FpvObjects objs;       // the step's object_list (count 0 = none); only the OBJ instantiation reads it
    uint16_t* state_h;     // FPV_FLAG_FP16_STATE: [5][ld] half2 pair rows + [ld] thrust halves
    uint32_t seed;         // stochastic-rounding base seed (fpv_buffers_t.rounding_seed); step t rounds with fpv_round_seed(seed, step + t)
    const float* rot_over;     // [n][9] guidance override of the attitude (Drone.step rotation_matrix=) or null
    const float* thrust_over;  // [n] thrust_force= of the same call (NaN = this drone is not overridden)
    uint16_t* thrust_h;        // FPV_FLAG_FP16_STATE: the row of prev_thrust halves (always set by to_device_view)
    // reset sources (fpv_abi.h, ABI 9) - last, so that no field the hot kernels read moves; read only inside the reset branch
    const float* reset_pose;   // [10][ld] per-lane base pose (p3 v3 q4) or null
    FpvResetJitter rj;         // FPV_FLAG_RESET_JITTER: the narrowed boxes and the seed (zeros without the flag)
};

// k-step launches (fpv_step_n): step t reads its action at + t*action_stride floats and writes
// reward/done at + t*out_stride elements, done_bits at + t*bits_stride words (0 = last step only)
struct FpvRoll { int32_t k; int32_t pad; int64_t action_stride, out_stride, bits_stride; };

// Row access = uniform 64-bit row base (SGPR pair) + 32-bit byte offset of the lane (fpv_addr.h):
// i * sizeof(T) < 2^32 because n <= 2^28 (fpv_create) and sizeof(T) <= 16.
template <class T>
__device__ __forceinline__ T& row_at(T* row_base, uint32_t i)
{
    static_assert(sizeof(T) <= FPV_MAX_ELEM_BYTES, "lane offsets are 32-bit: element too wide for n <= 2^28");
    return *reinterpret_cast<T*>(reinterpret_cast<char*>(const_cast<typename std::remove_const<T>::type*>(row_base)) + fpv_lane_offset(i, (uint32_t)sizeof(T)));
}
#define ROW(st, r, ld) ((st) + (int64_t)(r) * (ld))

#define LDROW(st, r, ld, i) row_at(ROW(st, r, ld), i)
#define STROW(st, r, ld, i, v) (row_at(ROW(st, r, ld), i) = (v))

__device__ __forceinline__ void ld_drone(const float* __restrict__ st, int64_t ld, uint32_t i, FpvDroneState& s)
{
    s.px = LDROW(st, FPV_PX, ld, i); s.py = LDROW(st, FPV_PY, ld, i); s.pz = LDROW(st, FPV_PZ, ld, i);
    s.vx = LDROW(st, FPV_VX, ld, i); s.vy = LDROW(st, FPV_VY, ld, i); s.vz = LDROW(st, FPV_VZ, ld, i);
    s.q.w = LDROW(st, FPV_QW, ld, i); s.q.x = LDROW(st, FPV_QX, ld, i); s.q.y = LDROW(st, FPV_QY, ld, i); s.q.z = LDROW(st, FPV_QZ, ld, i);
    s.rx = LDROW(st, FPV_RX, ld, i); s.ry = LDROW(st, FPV_RY, ld, i); s.rz = LDROW(st, FPV_RZ, ld, i);
    s.thrust = LDROW(st, FPV_THRUST, ld, i);
}

__device__ __forceinline__ void st_drone(float* __restrict__ st, int64_t ld, uint32_t i, const FpvDroneState& s)
{
    STROW(st, FPV_PX, ld, i, s.px); STROW(st, FPV_PY, ld, i, s.py); STROW(st, FPV_PZ, ld, i, s.pz);
    STROW(st, FPV_VX, ld, i, s.vx); STROW(st, FPV_VY, ld, i, s.vy); STROW(st, FPV_VZ, ld, i, s.vz);
    STROW(st, FPV_QW, ld, i, s.q.w); STROW(st, FPV_QX, ld, i, s.q.x); STROW(st, FPV_QY, ld, i, s.q.y); STROW(st, FPV_QZ, ld, i, s.q.z);
    STROW(st, FPV_RX, ld, i, s.rx); STROW(st, FPV_RY, ld, i, s.ry); STROW(st, FPV_RZ, ld, i, s.rz);
    STROW(st, FPV_THRUST, ld, i, s.thrust);
}

typedef float fpv_v4f __attribute__((ext_vector_type(4)));
// Rows that a step only WRITES (the body acceleration, the AoS observation head) leave with the streaming hint, like reward and
// done: nobody on this path reads them again before the next launch overwrites them, and stored plainly they take L2 lines away
// from the state rows that the next launch of a rotated chain comes back for (round 6, one box, 2^20 drones: accel rows 22.85 ->
// 22.35 us per launch, AoS head 32.8 -> 31.4; profiles/r06_exp_nt_output_rows.log).  rotation_blocks() does not count them either.
#define ST_OUT(ref, v) __builtin_nontemporal_store((v), &(ref))

// The action batch is read once and reward/done are written once per step: non-temporal, so they
// do not displace the state rows, which are re-read next step, from L2 / Infinity Cache.
__device__ __forceinline__ float4 ld_action(const float4* __restrict__ a, uint32_t i)
{
    const fpv_v4f v = __builtin_nontemporal_load(&row_at(reinterpret_cast<const fpv_v4f*>(a), i));
    return make_float4(v.x, v.y, v.z, v.w);
}

// either layout: rows [n][4] (one 16-byte load) or SoA [4][action_ld] (four dword loads) - the latter is
// what `W[4,13] @ obs[13,n]` produces, so a policy can feed the stepper without a transpose kernel
__device__ __forceinline__ float4 ld_action_any(const float4* __restrict__ a, int64_t action_ld, uint32_t i)
{
    if (action_ld == 0) return ld_action(a, i);
    const float* __restrict__ f = reinterpret_cast<const float*>(a);
    return make_float4(__builtin_nontemporal_load(&row_at(ROW(f, 0, action_ld), i)),
                       __builtin_nontemporal_load(&row_at(ROW(f, 1, action_ld), i)),
                       __builtin_nontemporal_load(&row_at(ROW(f, 2, action_ld), i)),
                       __builtin_nontemporal_load(&row_at(ROW(f, 3, action_ld), i)));
}

// Episode bookkeeping + done outputs shared by both modes.  `done` is wave-divergent data;
// all pointer tests are wave-uniform scalar branches.
__device__ __forceinline__ void emit_lane_outputs(const FpvBufD& B, uint32_t i, float reward, bool done);

__device__ __forceinline__ void emit_outputs(const FpvBufD& B, uint32_t i, bool live, float reward, bool done)
{
    // done_bits: one ballot per 64 consecutive drones; i - lane is a multiple of 64 by construction
    const unsigned long long mask = __ballot(live && done);
    if (B.done_bits && (threadIdx.x & 63) == 0 && live) B.done_bits[i >> 6] = mask;
    if (live) emit_lane_outputs(B, i, reward, done);
}

__device__ __forceinline__ void emit_lane_outputs(const FpvBufD& B, uint32_t i, float reward, bool done)
{
    if (B.reward) __builtin_nontemporal_store(reward, &row_at(B.reward, i));
    if (B.done) __builtin_nontemporal_store((uint8_t)(done ? 1 : 0), &row_at(B.done, i));
    if (B.ep_return) {
        const float r = B.ep_return[i] + reward;
        const int32_t l = B.ep_length[i] + 1;
        if (done) {
            if (B.last_return) B.last_return[i] = r;
            if (B.last_length) B.last_length[i] = l;
        }
        B.ep_return[i] = done ? 0.0f : r;
        B.ep_length[i] = done ? 0 : l;
    }
}

// Reset sources (fpv_abi.h): after fpv_drone_reset_lane has put init_* into `s`, a lane that resets takes its base pose from
// its row of the reset-pose table, when there is one, and adds the jitter of FPV_FLAG_RESET_JITTER.  Only the rare reset branch
// of the kernels that are not on the headline path calls this, with the view of the arguments it loads inside the branch.
// `t` = step index of the step whose done started the reset (fpv_reset: the handle's counter), `e` = 1 for fpv_reset.
__device__ __forceinline__ void apply_reset_source(const FpvK& K, const FpvBufD& B, uint32_t i, uint64_t t, uint32_t e, FpvDroneState& s)
{
    float pose[10] = {s.px, s.py, s.pz, s.vx, s.vy, s.vz, s.q.w, s.q.x, s.q.y, s.q.z};
    if (B.reset_pose) {
#pragma unroll
        for (int r = 0; r < 10; ++r) pose[r] = row_at(ROW(B.reset_pose, r, B.ld), i);
    }
    if (K.flags & FPV_FLAG_RESET_JITTER)
        fpv_reset_jitter(B.rj, (((uint64_t)K.noise.id_hi << 32) | K.noise.id_lo) + i, t, e, pose);
    s.px = pose[0]; s.py = pose[1]; s.pz = pose[2]; s.vx = pose[3]; s.vy = pose[4]; s.vz = pose[5];
    s.q.w = pose[6]; s.q.x = pose[7]; s.q.y = pose[8]; s.q.z = pose[9];
}

// "These values are used here": makes the compiler complete the loads that produced them BEFORE a k-step
// loop.  Without it the wait for the pre-loop state loads lands inside the loop, and because vmcnt retires
// in order it also waits for the action prefetch issued a few instructions earlier - every iteration then
// exposes a full memory latency (measured: 48 % VALU utilisation; PMC SQ_INSTS_VALU / time).
__device__ __forceinline__ void fpv_settle(float x) { asm volatile("" ::"v"(x)); }

// Per-step outputs of a k-step launch (fpv_step_n).  reward/done/done_bits go out every step when their
// stride is non-zero, otherwise once after the last step (= what k single-step launches leave behind);
// the episode accumulators live in registers for the k steps and touch memory once.
struct RollOut {
    float* rp; uint8_t* dp; unsigned long long* bp;
    int64_t out_stride, bits_stride;
    int last_t;
    bool track, had_done;
    float ep_r, last_r;
    int32_t ep_l, last_l;
    const FpvBufD& B;
    __device__ __forceinline__ RollOut(const FpvBufD& B_, const FpvRoll& R, uint32_t i, bool live)
        : rp(B_.reward), dp(B_.done), bp(B_.done_bits), out_stride(R.out_stride), bits_stride(R.bits_stride),
          last_t(R.k - 1), track(B_.ep_return != nullptr), had_done(false), ep_r(0.0f), last_r(0.0f), ep_l(0), last_l(0), B(B_)
    {
        if (track && live) { ep_r = B.ep_return[i]; ep_l = B.ep_length[i]; }
    }
    // called by every live lane of the wave in the same iteration (the ballot spans the wave).  QUIET = a step of a
    // launch that neither stores reward/done per step nor tracks episodes, and is not the last one: only the
    // optional per-step done_bits row is left of it
    // `live` = false: a lane that runs the step but owns no drone (fpv_drone_rollout_h_kernel's shadow lanes) - it
    // stores nothing (the mask word included: a wave is live exactly when its lane 0 is) and does not vote; the
    // per-step pointers stay wave-uniform because every lane advances them
    template <bool QUIET = false>
    __device__ __forceinline__ void step(uint32_t i, int t, float reward, bool done, bool live = true)
    {
        const bool last = !QUIET && t == last_t;
        if (bp && (bits_stride || last)) {
            const unsigned long long mask = __ballot(live && done);
            // a wave whose lane 0 owns no drone is wholly dead: no word is its own.  "Am I lane 0" is asked of an opaque copy of
            // the index on every call: as a loop-invariant lane mask the answer would sit in an SGPR pair across all k steps
            uint32_t ii = i;
            asm volatile("" : "+v"(ii));
            if ((ii & 63u) == 0 && live) bp[ii >> 6] = mask;
        }
        if (!QUIET) {
            if ((out_stride || last) && live) {
                if (rp) __builtin_nontemporal_store(reward, &row_at(rp, i));
                if (dp) __builtin_nontemporal_store((uint8_t)(done ? 1 : 0), &row_at(dp, i));
            }
            if (track) {
                ep_r += reward; ep_l += 1;
                if (done) { last_r = ep_r; last_l = ep_l; had_done = true; ep_r = 0.0f; ep_l = 0; }
            }
            if (rp) rp += out_stride;
            if (dp) dp += out_stride;
        }
        if (bp) bp += bits_stride;
    }
    // `Bf`: the buffers through a view taken AFTER the loop - "are episodes tracked" is then a fresh scalar test instead
    // of a flag carried across the k steps in an SGPR pair
    __device__ __forceinline__ void finish(uint32_t i, const FpvBufD& Bf)
    {
        if (Bf.ep_return) {
            Bf.ep_return[i] = ep_r; Bf.ep_length[i] = ep_l;
            if (had_done) {
                if (Bf.last_return) Bf.last_return[i] = last_r;
                if (Bf.last_length) Bf.last_length[i] = last_l;
            }
        }
    }
};

// The inverse-CDF table of the stick-noise generator (fpv_normal_from_word): 128 rows x 16 bytes in device memory, staged
// into LDS by every workgroup of a NOISE kernel - each lane then reads one row per normal with ONE ds_read_b128 at an
// address it computes from its random word.  (Half of all lanes read the top binade's rows: same-address reads are
// broadcast, not serialised.)  The staging runs BEFORE any lane leaves the kernel: every thread of the workgroup
// reaches the barrier.
__device__ const FpvNormalRow g_normal_table[FPV_NTAB_ROWS] = FPV_NTAB_DATA;

__device__ __forceinline__ void stage_normal_table(FpvNormalRow* lds)
{
    for (int r = threadIdx.x; r < FPV_NTAB_ROWS; r += kStepBlock) lds[r] = g_normal_table[r];
    __syncthreads();
}

// EMA stick noise: read 4 state floats, one Philox4x32-7 block -> 4 normals, write them back,
// perturb the action.  With no caller action (B.action null) the sticks are the pure noise profile.
__device__ __forceinline__ float4 apply_stick_noise(const FpvK& K, const FpvBufD& B, uint32_t i, float4 a, const FpvNormalRow* table)
{
    float ns[4], av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) ns[k] = row_at(ROW(B.noise_state, k, B.ld), i);
    fpv_stick_noise(K.noise, B.step, (uint64_t)i, table, ns, av);
#pragma unroll
    for (int k = 0; k < 4; ++k) row_at(ROW(B.noise_state, k, B.ld), i) = ns[k];
    const float4 r = make_float4(av[0], av[1], av[2], av[3]);
    if (B.action_out) B.action_out[i] = r;
    return r;
}

// OVR: the guidance call shape Drone.step(..., rotation_matrix=R, thrust_force=f) (components.py:230-232,
// simulator.py:110): nine more floats and the thrust force per drone, read with a 36-byte lane stride - the
// matrices arrive in the caller's [n][3][3] layout; this is the closed-loop guidance path, not the headline one.
// One drone per lane, kStepBlock threads per workgroup: 2 / 4 drones per lane and 256-thread workgroups lost every
// measurement of rounds 1-2 (profiles/archive/r01_exp10_shapes_clean.log, r02_sweep_geometry.log) and were removed in round 3.
// The single-step kernels take what their FIRST instructions need - the state and action bases, the row stride, n - as
// plain leading scalars, ahead of the two argument structs.  The library is built with
// -mllvm -amdgpu-kernarg-preload-count=6 (six leading 8-byte arguments = 12 dwords): on gfx950 the command processor then
// places this 12-dword prefix of the
// kernel-argument segment in SGPRs at wave launch, so a wave issues its 15 vector loads at once instead of first
// waiting for a scalar load of those pointers - a cold one at every kernel start, because the scalar cache and L2
// are invalidated at the kernel boundary.  It is the head of the per-launch floor of a chain of dependent step
// kernels (profiles/archive/r03_exp_launch_floor.log).  (Firmware without the feature runs the compiler's compatibility
// prologue, which loads the same prefix with s_load: same results either way.)  The structs that follow still carry
// the same fields; fpv_step_view() overrides them, so their kernarg copies are never loaded.
#define FPV_STEP_PARAMS float* __restrict__ a_state, const int64_t a_ld, const float4* __restrict__ a_action, \
                        const int64_t a_action_ld, uint16_t* __restrict__ a_state_h, const int64_t n_start, const FpvK K, const FpvBufD B_
// `n_start` = the number of drones (low 32 bits; n <= 2^28) and a START BLOCK (high 32 bits): workgroup b works on block
// (b + start) mod blocks - ascending addresses all the way, one wrap.  The host moves the start BACK by a cache's worth of
// drones from launch to launch (update_rotation / launch_step), so that a launch BEGINS on the state rows the previous launch wrote
// LAST - the ones the cache still holds (the eight L2s for a population inside the Infinity Cache, the 256 MiB Infinity Cache for
// a larger one) - instead of on the ones it wrote first, which a population larger than the cache has pushed out by then (every
// launch in the same order finds nothing: cyclic access is the worst case of a recency cache).  Results do not depend on the
// order in which blocks run; start = 0 is the plain order.  n and the block count come from the preloaded argument: gridDim.x
// would be a cold scalar load ahead of the first vector loads.  The block count is n's, rounded up to whole rounds of the eight
// XCDs (step_grid; up to seven blocks of a launch have no drone and leave at once): workgroups go to the XCDs round-robin, so
// with a modulus and a start that are multiples of eight every block stays on its XCD across the wrap and across launches -
// a ragged count would hand each block to another XCD's L2 every launch (1 000 000 drones: no gain from the rotation at all).
#define FPV_STEP_INDEX \
    const int64_t n = n_start & 0xffffffffll; \
    const uint32_t nblk_ = (uint32_t)((n + 8 * kStepBlock - 1) / (8 * kStepBlock)) * 8u; \
    uint32_t blk_ = blockIdx.x + (uint32_t)(n_start >> 32); \
    blk_ = blk_ >= nblk_ ? blk_ - nblk_ : blk_; \
    const uint32_t i = blk_ * (uint32_t)kStepBlock + threadIdx.x
__device__ __forceinline__ FpvBufD fpv_step_view(const FpvBufD& B_, float* st, int64_t ld, const float4* act, int64_t act_ld, uint16_t* sh)
{
    FpvBufD B = B_;
    B.state = st; B.ld = ld; B.action = act; B.action_ld = act_ld; B.state_h = sh;
    return B;
}
#define FPV_STEP_VIEW const FpvBufD B = fpv_step_view(B_, a_state, a_ld, a_action, a_action_ld, a_state_h)

// The kernel-argument segment of a single-step kernel as ONE struct (the parameters of FPV_STEP_PARAMS in order, each at
// its natural alignment: exactly how the segment is laid out), and a fresh opaque view of it - what fpv_args_again() is
// for the k-step kernels.  The instantiations that carry more uniforms than the SGPR file holds (in-kernel noise: the
// Philox keys and the table staging on top of the physics constants and a dozen buffer pointers; object list + guidance
// override) read their arguments once per SECTION - loads and sticks / physics / stores - instead of keeping every field
// alive from the first instruction to the last: 12-34 spilled SGPRs (v_readlane / v_writelane per use) in round 3,
// none now.  The plain kernel takes one view, for its constants and the wind, ahead of its row loads (fpv_drone_step_kernel).
struct FpvStepArgs { float* state; int64_t ld; const float4* action; int64_t action_ld; uint16_t* state_h; int64_t n; FpvK K; FpvBufD B; };
__device__ __forceinline__ const FpvStepArgs& fpv_step_args_again()
{
    typedef const __attribute__((address_space(4))) FpvStepArgs* P4;
    P4 p = (P4)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const FpvStepArgs*)p;
}

// ---- k-step kernels: ONE kernel parameter, so that offsets into the kernel-argument segment are offsetof() ----
struct FpvRollArgs { FpvK K; FpvBufD B; int64_t n; FpvRoll R; };
typedef const __attribute__((address_space(4))) FpvRollArgs* FpvArgsPtr;

// A fresh, opaque view of the kernel arguments.  Every field of FpvRollArgs is a scalar load from the kernarg segment;
// the compiler issues all of them at the top of the kernel and keeps the values in SGPRs for as long as anything below
// uses them - the 14 row addresses of the final state stores, the reset pose, the goal, the episode buffers ... lived
// in SGPRs ACROSS the k-step loop, the kernel sat at the 102-SGPR limit (7 waves per SIMD) and spilled 40-105 of them
// into VGPR lanes (round 2; tools/kernel_resources.py had been hiding it).  Loads through the pointer returned here
// cannot be merged with earlier loads of the same field, nor hoisted above this point: what is needed only after the
// loop (or only in the rare reset branch) is loaded there.
__device__ __forceinline__ const FpvRollArgs& fpv_args_again()
{
    FpvArgsPtr p = (FpvArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const FpvRollArgs*)p;
}

// The reset sources of a k-step kernel's reset branch (apply_reset_source for the k-step kernels).  Their SGPR files are spoken for
// by the loop: with the whole FpvResetJitter read through one view (apply_reset_source) 4-26 SGPRs spilled into VGPR lanes, and
// read through a VGPR copy of the argument pointer the plain k-step kernel went from 56 to 90+ VGPRs.  Here each block's six
// constants and key come through a view of their own that is ordered after the previous block's result: one block's uniforms are
// live at a time (no spill; VGPRs within 2 of the kernels without the branch).
__device__ __forceinline__ FpvArgsPtr fpv_args_after(float after)
{
    FpvArgsPtr p = (FpvArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p) : "v"(after));         // (ordered after `after`: one block's constants are loaded at a time)
    return p;
}

__device__ __forceinline__ void apply_reset_source_k(uint32_t i, uint64_t t, FpvDroneState& s)
{
    float pose[10] = {s.px, s.py, s.pz, s.vx, s.vy, s.vz, s.q.w, s.q.x, s.q.y, s.q.z};
    FpvArgsPtr A = fpv_args_after(s.px);
    const float* tab = A->B.reset_pose;
    if (tab) {
        const int64_t ld = A->B.ld;
#pragma unroll
        for (int r = 0; r < 10; ++r) pose[r] = row_at(ROW(tab, r, ld), i);
    }
    if (A->K.flags & FPV_FLAG_RESET_JITTER) {
#pragma unroll
        for (uint32_t b = 0; b < 3; ++b) {
            const FpvArgsPtr V = fpv_args_after(pose[3 * b]);
            const float lo[3] = {V->B.rj.lo[3 * b], V->B.rj.lo[3 * b + 1], V->B.rj.lo[3 * b + 2]};
            const float span[3] = {V->B.rj.span[3 * b], V->B.rj.span[3 * b + 1], V->B.rj.span[3 * b + 2]};
            fpv_reset_jitter_block(lo, span, V->B.rj.seed_lo, V->B.rj.seed_hi, (((uint64_t)V->K.noise.id_hi << 32) | V->K.noise.id_lo) + i,
                                   V->B.step + t, 0u, b, pose);
        }
    }
    s.px = pose[0]; s.py = pose[1]; s.pz = pose[2]; s.vx = pose[3]; s.vy = pose[4]; s.vz = pose[5];
    s.q.w = pose[6]; s.q.x = pose[7]; s.q.y = pose[8]; s.q.z = pose[9];
}

// ---- per-drone physics (csrc/fpv_phys.hip; launched from fpv_hip.hip: plan_launch picks the kernel, StepLaunch / launch_roll fill these) ----
// k-step kernels: the arguments of fpv_drone_rollout_kernel first (the views above read them at the same offsets), then the table
struct FpvRollPhysArgs { FpvRollArgs A; const float* phys; int32_t ground; int32_t pad; };
// single-step kernels: n <= 2^28, so bit 31 of n_start's low word is free - "this launch loads the two ground rows", decided on
// the host and read from a preloaded SGPR: no scalar load stands between the wave's start and its table loads
constexpr int64_t kPhysGroundBit = (int64_t)1 << 31;

// ---- gate courses (csrc/fpv_gate.hip; launched from fpv_hip.hip in the same way) ----
// what fpv_set_gates binds, as the kernels read it: the descriptor table, the word row, the optional observation rows and start
// gates, the course's uniform constants.  The single-step kernel takes FPV_STEP_PARAMS with the word base in the state_h slot - a
// gate handle has no fp16 state - and this struct as a ninth parameter; the k-step kernels take one FpvRollGateArgs, the
// arguments of fpv_drone_rollout_kernel first (the views above read them at the same offsets).
struct FpvGateArgs { const fpv_gate_v4* tab; uint32_t* word; float* obs; int64_t obs_ld; const uint8_t* start; FpvGateK K; };
struct FpvRollGateArgs { FpvRollArgs A; FpvGateArgs G; };

}  // namespace
