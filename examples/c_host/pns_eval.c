/* pns_eval.c - a plain C host of point and shoot's host functions (include/fpv_abi.h "Point and shoot"): fpv_pns_derive and
 * fpv_pns_eval on a few drones, no GPU.  Also the program tests/test_pns_sanitized.py builds with AddressSanitizer and
 * UndefinedBehaviorSanitizer around the library's host code:
 *
 *   hipcc --offload-arch=gfx950 -O1 -Xarch_host -fsanitize=address,undefined -ffp-contract=off -std=c++17 \
 *         -c fpyv_amd/csrc/fpv_hip.hip -o fpv_host.o          (and the same for fpyv_amd/csrc/fpv_pns.hip -o fpv_pns.o)
 *   clang -O1 -fsanitize=address,undefined -Iinclude -c examples/c_host/pns_eval.c -o pns_eval.o
 *   hipcc -fsanitize=address,undefined fpv_host.o fpv_pns.o pns_eval.o -o pns_eval && ./pns_eval
 *
 * (the sanitizers instrument the host halves only; nothing here touches a device)
 * Every buffer is sized exactly (heap, so that a byte past an output is caught), the PID, prev_pixel and target rows carry a padded
 * stride that must stay untouched, and the law runs with the pixel found from per-drone target rows, from one shared target, and
 * with the pixel given, twice in a row and with a restart.  Prints one line per check and returns 0 when all hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fpv_abi.h"

#define N 6
#define PAD 3
#define FMAX 81.3

static int failures = 0;

static void check(int ok, const char* what)
{
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) ++failures;
}

static int orthonormal(const float* R)
{
    int ok = 1;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = (double)R[a] * R[b] + (double)R[3 + a] * R[3 + b] + (double)R[6 + a] * R[6 + b];
            ok = ok && fabs(d - (a == b)) < 1e-5;
        }
    return ok;
}

int main(void)
{
    fpv_camera_t cam;
    memset(&cam, 0, sizeof cam);
    cam.pitch_deg = 35.0; cam.fov_deg = 120.0; cam.width = 640; cam.height = 480;       /* the reference's camera */
    cam.relative_position[0] = 0.1;
    fpv_pns_t s;
    memset(&s, 0, sizeof s);
    check(fpv_pns_derive(&cam, &s) == FPV_OK, "fpv_pns_derive accepts 640 x 480");
    check(fabs(s.focal_length - 640 / (2.0 * tan(60.0 * 3.14159265358979323846 / 180.0))) < 1e-12, "focal length");
    s.struct_size = (uint32_t)fpv_sizeof(12);
    s.ref_frame = FPV_CHASE_WORLD; s.mode = FPV_CHASE_LEVEL; s.max_depth = 15.0; s.mass = 0.75;
    s.virtual_drag_coefficient = 0.5; s.virtual_lift_coefficient = 0.1; s.tof_effective_distance = 2.0;
    s.max_throttle_in_force = FMAX;
    s.thrust2throttle_poly[0] = 2.0e-4; s.thrust2throttle_poly[1] = -3.4e-2; s.thrust2throttle_poly[2] = 2.6; s.thrust2throttle_poly[3] = 1.0;
    s.pid.struct_size = (uint32_t)fpv_sizeof(3);
    s.pid.kP = 0.1; s.pid.kI = 2.0; s.pid.kD = 0.05; s.pid.dt = 0.004; s.pid.integral_clip = 100.0;
    s.pid.min_output = 1.5; s.pid.max_output = FMAX; s.pid.derivative_transition_rate = 0.2;

    float* p = (float*)malloc(N * 3 * sizeof(float));
    float* v = (float*)malloc(N * 3 * sizeof(float));
    float* q = (float*)malloc(N * 4 * sizeof(float));
    const size_t ld = N + PAD;
    float* targets = (float*)malloc(3 * ld * sizeof(float));
    for (int i = 0; i < N; ++i) {
        p[3 * i] = -1.0f + 0.5f * i; p[3 * i + 1] = 0.2f * i; p[3 * i + 2] = 1.0f + 0.6f * i;
        v[3 * i] = i == 2 ? 0.0f : 1.0f; v[3 * i + 1] = i == 3 ? 40.0f : 0.0f; v[3 * i + 2] = i == 2 ? 0.0f : -0.3f;   /* 2 stands still, 3 is far too fast */
        const float a = i == N - 1 ? 1.5707963f : 0.1f * i;                                            /* the last one looks away */
        q[4 * i] = cosf(a); q[4 * i + 1] = 0.0f; q[4 * i + 2] = 0.0f; q[4 * i + 3] = sinf(a);
        targets[i] = p[3 * i] + 6.0f; targets[ld + i] = p[3 * i + 1] + 0.5f; targets[2 * ld + i] = p[3 * i + 2] + 3.0f;
    }
    for (size_t k = 0; k < 3 * ld; ++k) if (k % ld >= N) targets[k] = -7.0f;
    float* rows = (float*)malloc(FPV_PID_ROWS * ld * sizeof(float));
    for (size_t k = 0; k < FPV_PID_ROWS * ld; ++k) rows[k] = k % ld >= N ? -7.0f : (k / ld == FPV_PID_IS_FIRST ? 1.0f : 0.0f);
    float* prev = (float*)malloc(2 * ld * sizeof(float));
    for (size_t k = 0; k < 2 * ld; ++k) prev[k] = k % ld >= N ? -7.0f : NAN;
    float* rot = (float*)malloc(N * 9 * sizeof(float));
    float* thrust = (float*)malloc(N * sizeof(float));
    float* throttle = (float*)malloc(N * sizeof(float));
    float* vel = NULL;
    float* action = NULL;
    check(posix_memalign((void**)&vel, 8, N * 2 * sizeof(float)) == 0 && posix_memalign((void**)&action, 16, N * 4 * sizeof(float)) == 0, "aligned buffers");
    for (int i = 0; i < N; ++i) { action[4 * i] = 0.3f; action[4 * i + 1] = -0.2f; action[4 * i + 2] = 0.05f * i; action[4 * i + 3] = -0.1f; }
    uint8_t* vis = (uint8_t*)malloc(N);
    uint8_t* lim = (uint8_t*)malloc(N);
    uint8_t* restart = (uint8_t*)calloc(N, 1);
    s.pid_state = rows; s.pid_ld = (int64_t)ld; s.prev_pixel = prev; s.prev_pixel_ld = (int64_t)ld;
    s.target_rows = targets; s.target_ld = (int64_t)ld; s.action = action;
    s.rotation = rot; s.thrust = thrust; s.pixel_velocity = vel; s.limited = lim; s.visible = vis; s.throttle = throttle;

    check(fpv_pns_eval(&s, N, p, v, q) == FPV_OK, "fpv_pns_eval, the pixel found from per-drone target rows");
    int seen = 0, guided_ok = 1, unseen_ok = 1, padding = 1;
    for (int i = 0; i < N; ++i) {
        const float* R = rot + 9 * i;
        if (vis[i]) {
            ++seen;
            guided_ok = guided_ok && orthonormal(R) && isfinite(thrust[i]) && thrust[i] > 0.0f && thrust[i] <= (float)FMAX && rows[FPV_PID_IS_FIRST * ld + i] == 0.0f
                        && vel[2 * i] == 0.0f && vel[2 * i + 1] == 0.0f && isfinite(prev[i]) && throttle[i] >= -1.0f && throttle[i] <= 1.0f;
        } else {
            unseen_ok = unseen_ok && isnan(thrust[i]) && isnan(vel[2 * i]) && isnan(throttle[i]) && lim[i] == 0 && R[0] == 1.0f && R[4] == 1.0f && R[8] == 1.0f
                        && R[1] == 0.0f && rows[FPV_PID_IS_FIRST * ld + i] == 1.0f && isnan(prev[i]);
        }
    }
    check(seen >= 3 && seen < N, "some drones see their target, the one that looks away does not");
    check(guided_ok, "a guided drone gets an orthonormal matrix, a force within the limit, no pixel velocity on its first call, an advanced PID");
    check(unseen_ok, "an unguided drone gets the identity and NaNs and keeps its PID rows and prev_pixel");
    check(vis[3] && lim[3] == 2 && thrust[3] == (float)FMAX, "the limit out of reach: the limit itself, flagged 2");

    restart[0] = 1;
    s.restart = restart;
    check(fpv_pns_eval(&s, N, p, v, q) == FPV_OK, "a second call, drone 0 restarted");
    check(vel[0] == 0.0f && rows[FPV_PID_IS_FIRST * ld] == 0.0f && rows[FPV_PID_PREV_DERIVATIVE * ld] == 0.0f, "the restarted drone makes its first call again");
    check(vis[1] && vel[2] == 0.0f && vel[3] == 0.0f && rows[FPV_PID_PREV_DERIVATIVE * ld + 1] == 0.0f, "an unmoved pixel has no velocity and no derivative");
    for (size_t k = 0; k < FPV_PID_ROWS * ld; ++k)
        if (k % ld >= N) padding = padding && rows[k] == -7.0f;
    for (size_t k = 0; k < 2 * ld; ++k)
        if (k % ld >= N) padding = padding && prev[k] == -7.0f;
    check(padding, "the padding of the PID and prev_pixel rows is untouched");

    const float centre[3] = {6.0f, 0.5f, 4.0f};
    s.target_rows = NULL; s.target = centre; s.restart = NULL; s.action = NULL;
    check(fpv_pns_eval(&s, N, p, v, q) == FPV_OK, "one shared target, no commands");

    float* given = NULL;
    check(posix_memalign((void**)&given, 8, N * 2 * sizeof(float)) == 0, "aligned pixels");
    for (int i = 0; i < N; ++i) { given[2 * i] = 300.0f + 10.0f * i; given[2 * i + 1] = i == 1 ? NAN : 200.0f; }
    s.target = NULL; s.pixel = given; s.action = action; s.ref_frame = FPV_CHASE_DRONE; s.mode = FPV_CHASE_FRONTARGET;
    s.pixel_velocity = NULL; s.limited = NULL; s.throttle = NULL;
    check(fpv_pns_eval(&s, N, p, v, q) == FPV_OK, "fpv_pns_eval, the pixel given, drone frame, frontarget, no optional output but visible");
    int given_ok = 1;
    for (int i = 0; i < N; ++i) given_ok = given_ok && vis[i] == (i != 1) && (i == 1 ? isnan(thrust[i]) : isfinite(thrust[i]) && prev[i] == given[2 * i] + action[4 * i + 2] * 320.0f);
    check(given_ok, "a NaN pixel is an unseen target; the others are used as given, the offset added");

    s.target = centre; s.target_rows = targets;
    check(fpv_pns_eval(&s, N, p, v, q) == FPV_EINVAL && strstr(fpv_last_error(), "both a shared target and target_rows") != NULL, "a refusal names its reason");

    free(given); free(restart); free(lim); free(vis); free(action); free(vel); free(throttle); free(thrust); free(rot); free(prev); free(rows);
    free(targets); free(q); free(v); free(p);
    return failures ? 1 : 0;
}
