/* pursuit_eval.c - a plain C host of the pursuit task's host functions (include/fpv_abi.h "Pursuit task"): fpv_pursuit_derive,
 * fpv_pursuit_sample and fpv_pursuit_eval on a few drones with a target each, no GPU.  Also the program
 * tests/test_pursuit_sanitized.py builds with AddressSanitizer and UndefinedBehaviorSanitizer around the library's host code:
 *
 *   hipcc --offload-arch=gfx950 -O1 -Xarch_host -fsanitize=address,undefined -ffp-contract=off -std=c++17 \
 *         -c fpyv_amd/csrc/fpv_hip.hip -o fpv_host.o     (and the same for csrc/fpv_chase.hip and csrc/fpv_pursuit.hip)
 *   clang -O1 -fsanitize=address,undefined -Iinclude -c examples/c_host/pursuit_eval.c -o pursuit_eval.o
 *   hipcc -fsanitize=address,undefined fpv_host.o fpv_chase.o fpv_pursuit.o pursuit_eval.o -o pursuit_eval && ./pursuit_eval
 *
 * (the sanitizers instrument the host halves only; nothing here touches a device)
 * Every buffer is sized exactly (heap, so that a byte past an output is caught), the rows carry a padded stride that must stay
 * untouched, and the task runs as a reset call with a mask, as steps that capture and respawn, and with the guidance law.  Prints
 * one line per check and returns 0 when all hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fpv_abi.h"

#define N 6
#define PAD 2                      /* N + PAD = 8 cells per row */
#define K 7

static int failures = 0;

static void check(int ok, const char* what)
{
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) ++failures;
}

static float* rows_of(size_t rows, size_t ld, float fill)
{
    float* r = NULL;
    if (posix_memalign((void**)&r, 16, rows * ld * sizeof(float)) != 0) exit(2);
    for (size_t k = 0; k < rows * ld; ++k) r[k] = fill;
    return r;
}

int main(void)
{
    const size_t ld = N + PAD;
    const float guard = 1.0e30f;
    float* circle = NULL;
    if (posix_memalign((void**)&circle, 16, K * 2 * sizeof(float)) != 0) return 2;
    check(fpv_pursuit_derive(K, circle) == FPV_OK, "fpv_pursuit_derive fills a table of 7");
    check(circle[0] == 1.0f && circle[1] == 0.0f && fabsf(circle[2] - cosf(6.2831853f / K)) < 1e-6f, "the table starts at (1, 0)");
    check(fpv_pursuit_derive(0, circle) < 0, "a resolution of 0 is refused");

    float* targets = rows_of(FPV_TGT_ROWS, ld, guard);
    uint32_t* words = (uint32_t*)targets;
    for (int i = 0; i < N; ++i) {
        targets[FPV_TGT_CX * ld + i] = 2.0f + i; targets[FPV_TGT_CY * ld + i] = -1.0f; targets[FPV_TGT_CZ * ld + i] = 3.0f;
        targets[FPV_TGT_PATH_R * ld + i] = i % 2 ? 1.5f : 0.0f; targets[FPV_TGT_RADIUS * ld + i] = 0.5f; targets[FPV_TGT_PREV_DIST * ld + i] = 0.0f;
        words[FPV_TGT_COUNT * ld + i] = (uint32_t)(i % K) | FPV_TGT_FRESH; words[FPV_TGT_SPAWNS * ld + i] = 0u;
    }
    float* obs = rows_of(FPV_PURSUIT_OBS, ld, guard);
    float* position = rows_of(3, ld, guard);
    float* p = (float*)malloc(N * 3 * sizeof(float));
    float* v = (float*)malloc(N * 3 * sizeof(float));
    float* q = (float*)malloc(N * 4 * sizeof(float));
    float* reward = (float*)malloc(N * sizeof(float));
    float* paid = (float*)malloc(N * sizeof(float));
    uint8_t* event = (uint8_t*)malloc(N);
    uint8_t* flags = (uint8_t*)malloc(N);
    for (int i = 0; i < N; ++i) {
        p[3 * i] = -6.0f; p[3 * i + 1] = 0.3f * i; p[3 * i + 2] = 3.5f;
        v[3 * i] = 1.0f; v[3 * i + 1] = 0.0f; v[3 * i + 2] = -0.2f;
        q[4 * i] = 1.0f; q[4 * i + 1] = q[4 * i + 2] = q[4 * i + 3] = 0.0f;
        reward[i] = 0.25f; paid[i] = guard; event[i] = 0x5A; flags[i] = (uint8_t)(i != 4);
    }

    fpv_pursuit_t s;
    memset(&s, 0, sizeof s);
    s.struct_size = (uint32_t)fpv_sizeof(10);
    check(s.struct_size == sizeof(fpv_pursuit_t), "fpv_sizeof(10) is the struct");
    s.path_resolution = K; s.advance = 1; s.respawn_on_done = 0; s.add_to_reward = 1; s.spawn_seed = 0x1234567890ULL;
    s.dt = 0.004; s.capture_distance = 0.25; s.progress = 1.5; s.capture = 7.0;
    for (int k = 0; k < 3; ++k) { s.spawn_lo[k] = k == 2 ? 1.0 : -4.0; s.spawn_hi[k] = k == 2 ? 5.0 : 4.0; }
    s.radius_lo = 0.3; s.radius_hi = 0.8;
    s.targets = targets; s.targets_ld = (int64_t)ld; s.circle = circle;
    s.obs = obs; s.obs_ld = (int64_t)ld; s.position = position; s.position_ld = (int64_t)ld; s.event = event; s.reward_out = paid;

    float draw[4];
    uint32_t phase = 99;
    check(fpv_pursuit_sample(&s, 3, 0, draw, &phase) == FPV_OK && phase < K, "fpv_pursuit_sample draws a phase below K");
    check(draw[0] >= -4.0f && draw[0] <= 4.0f && draw[2] >= 1.0f && draw[2] <= 5.0f && draw[3] >= 0.3f && draw[3] <= 0.8f, "the draw lies in the box");

    /* the reset call with a mask: drone 4 is left alone */
    check(fpv_pursuit_eval(&s, N, 0, p, v, q, flags, reward, 1) == FPV_OK, "the reset call with a mask");
    check(obs[6 * ld + 4] == guard && paid[4] == guard && event[4] == 0x5A && (words[FPV_TGT_COUNT * ld + 4] & FPV_TGT_FRESH), "the lane outside the mask is not touched");
    check(paid[0] == 0.0f && event[0] == 0 && reward[0] == 0.25f && !(words[FPV_TGT_COUNT * ld + 0] & FPV_TGT_FRESH), "a reset lane is paid nothing and its target is advanced");
    check(targets[FPV_TGT_PREV_DIST * ld + 1] == obs[6 * ld + 1] && obs[6 * ld + 1] > 7.0f, "PREV_DIST restarts at the measured distance");

    /* steps: drones 0, 2 and 4 jump onto their targets in the second one; a capture pays, respawns and is counted */
    s.respawn_on_done = 1;
    int captured = 0;
    for (int step = 0; step < 3; ++step) {
        for (int i = 0; i < N; ++i) {
            flags[i] = (uint8_t)(step == 2 && i == 5);                                   /* drone 5 crashes in the last step */
            if (step == 1 && i % 2 == 0) { p[3 * i] = 2.0f + i; p[3 * i + 1] = -1.0f; p[3 * i + 2] = 3.0f; }   /* onto the targets that stand still */
            reward[i] = 0.25f;
        }
        check(fpv_pursuit_eval(&s, N, 0, p, v, q, flags, reward, 0) == FPV_OK, "a step call");
        for (int i = 0; i < N; ++i) captured += event[i];
    }
    check(captured >= 3, "drones that reach their target capture it");
    check((words[FPV_TGT_SPAWNS * ld + 0] >> 16) >= 1u && (words[FPV_TGT_SPAWNS * ld + 0] & 0xffffu) >= 1u, "a capture counts and respawns");
    check(paid[5] == 0.0f && reward[5] == 0.25f && (words[FPV_TGT_SPAWNS * ld + 5] >> 16) == 0u, "a done lane rebases: no payment, no captures");
    int padding = 1;
    for (size_t r = 0; r < FPV_TGT_ROWS; ++r) for (size_t k = N; k < ld; ++k) padding &= targets[r * ld + k] == guard;
    for (size_t r = 0; r < FPV_PURSUIT_OBS; ++r) for (size_t k = N; k < ld; ++k) padding &= obs[r * ld + k] == guard;
    for (size_t r = 0; r < 3; ++r) for (size_t k = N; k < ld; ++k) padding &= position[r * ld + k] == guard;
    check(padding, "the padding of every row is untouched");

    /* the guidance law against every drone's own target */
    fpv_camera_t cam;
    memset(&cam, 0, sizeof cam);
    cam.pitch_deg = 35.0; cam.fov_deg = 120.0; cam.width = 640; cam.height = 480;
    fpv_chase_t g;
    memset(&g, 0, sizeof g);
    check(fpv_chase_derive(&cam, &g) == FPV_OK, "fpv_chase_derive for the guide");
    g.struct_size = (uint32_t)fpv_sizeof(8);
    g.ref_frame = FPV_CHASE_WORLD; g.mode = FPV_CHASE_LEVEL; g.max_depth = 40.0; g.mass = 0.75;
    g.virtual_drag_coefficient = 0.5; g.virtual_lift_coefficient = 0.1; g.tof_effective_distance = 2.0;
    g.keep_distance = 6.0; g.UWB_sensor_max_range = 13.0;
    g.pid.struct_size = (uint32_t)fpv_sizeof(3);
    g.pid.kP = 0.1; g.pid.kI = 2.0; g.pid.kD = 0.05; g.pid.dt = 0.004; g.pid.integral_clip = 100.0;
    g.pid.min_output = 0.9; g.pid.max_output = 60.0; g.pid.derivative_transition_rate = 0.2;
    float* pid = rows_of(FPV_PID_ROWS, ld, guard);
    for (int i = 0; i < N; ++i) { pid[0 * ld + i] = pid[1 * ld + i] = pid[2 * ld + i] = 0.0f; pid[3 * ld + i] = 1.0f; }
    float* rotation = (float*)malloc(N * 9 * sizeof(float));
    float* thrust = (float*)malloc(N * sizeof(float));
    uint8_t* visible = (uint8_t*)malloc(N);
    g.pid_state = pid; g.pid_ld = (int64_t)ld; g.rotation = rotation; g.thrust = thrust; g.visible = visible;
    s.guide = &g;
    for (int i = 0; i < N; ++i) { flags[i] = 0; p[3 * i] = position[0 * ld + i] - 5.0f; p[3 * i + 1] = position[1 * ld + i]; p[3 * i + 2] = position[2 * ld + i]; }
    check(fpv_pursuit_eval(&s, N, 0, p, v, q, flags, reward, 0) == FPV_OK, "a step call with the guidance law");
    int seen = 0, orthonormal = 1;
    for (int i = 0; i < N; ++i) {
        seen += visible[i];
        if (!visible[i]) continue;
        const float* R = rotation + 9 * i;
        orthonormal &= fabsf(R[0] * R[0] + R[3] * R[3] + R[6] * R[6] - 1.0f) < 1e-5f && thrust[i] > 0.0f && pid[3 * ld + i] == 0.0f;
    }
    check(seen >= 3 && orthonormal, "drones that look at their target get a unit matrix column, a thrust and an advanced PID");
    for (size_t r = 0; r < FPV_PID_ROWS; ++r) for (size_t k = N; k < ld; ++k) padding &= pid[r * ld + k] == guard;
    check(padding, "the padding of the PID rows is untouched");
    g.thrust = NULL;
    check(fpv_pursuit_eval(&s, N, 0, p, v, q, flags, reward, 0) < 0 && strstr(fpv_last_error(), "thrust is null") != NULL, "a guide without thrust is refused by name");

    free(circle); free(targets); free(obs); free(position); free(p); free(v); free(q); free(reward); free(paid); free(event); free(flags);
    free(pid); free(rotation); free(thrust); free(visible);
    printf("%s\n", failures ? "pursuit_eval: FAILED" : "pursuit_eval: all checks hold");
    return failures ? 1 : 0;
}
