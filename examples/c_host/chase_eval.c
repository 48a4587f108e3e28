/* chase_eval.c - a plain C host of the target chase's host functions (include/fpv_abi.h "Target chase"): fpv_chase_derive and
 * fpv_chase_eval on a few drones around one target, no GPU.  Also the program tests/test_chase_sanitized.py builds with
 * AddressSanitizer and UndefinedBehaviorSanitizer around the library's host code:
 *
 *   hipcc --offload-arch=gfx950 -O1 -Xarch_host -fsanitize=address,undefined -ffp-contract=off -std=c++17 \
 *         -c fpyv_amd/csrc/fpv_hip.hip -o fpv_host.o          (and the same for fpyv_amd/csrc/fpv_chase.hip -o fpv_chase.o)
 *   clang -O1 -fsanitize=address,undefined -Iinclude -c examples/c_host/chase_eval.c -o chase_eval.o
 *   hipcc -fsanitize=address,undefined fpv_host.o fpv_chase.o chase_eval.o -o chase_eval && ./chase_eval
 *
 * (the sanitizers instrument the host halves only; nothing here touches a device)
 * Every buffer is sized exactly (heap, so that a byte past an output is caught), the PID rows carry a padded stride that must stay
 * untouched, and the law runs with the pixel found and with the pixel given.  Prints one line per check and returns 0 when all
 * hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fpv_abi.h"

#define N 6
#define PAD 3

static int failures = 0;

static void check(int ok, const char* what)
{
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) ++failures;
}

int main(void)
{
    fpv_camera_t cam;
    memset(&cam, 0, sizeof cam);
    cam.pitch_deg = 35.0; cam.fov_deg = 120.0; cam.width = 640; cam.height = 480;       /* the reference's camera */
    cam.relative_position[0] = 0.1;
    fpv_chase_t s;
    memset(&s, 0, sizeof s);
    check(fpv_chase_derive(&cam, &s) == FPV_OK, "fpv_chase_derive accepts 640 x 480");
    check(fabs(s.focal_length - 640 / (2.0 * tan(60.0 * 3.14159265358979323846 / 180.0))) < 1e-12, "focal length");
    s.struct_size = (uint32_t)fpv_sizeof(8);
    s.ref_frame = FPV_CHASE_WORLD; s.mode = FPV_CHASE_LEVEL; s.max_depth = 15.0; s.mass = 0.75;
    s.virtual_drag_coefficient = 0.5; s.virtual_lift_coefficient = 0.1; s.tof_effective_distance = 2.0;
    s.keep_distance = 6.0; s.UWB_sensor_max_range = 13.0;
    s.target[0] = 6.0f; s.target[1] = 0.5f; s.target[2] = 4.0f; s.target_radius = 0.5f;
    s.pid.struct_size = (uint32_t)fpv_sizeof(3);
    s.pid.kP = 0.1; s.pid.kI = 2.0; s.pid.kD = 0.05; s.pid.dt = 0.004; s.pid.integral_clip = 100.0;
    s.pid.min_output = 0.9; s.pid.max_output = 60.0; s.pid.derivative_transition_rate = 0.2;

    float* p = (float*)malloc(N * 3 * sizeof(float));
    float* v = (float*)malloc(N * 3 * sizeof(float));
    float* q = (float*)malloc(N * 4 * sizeof(float));
    for (int i = 0; i < N; ++i) {
        p[3 * i] = -1.0f + 0.5f * i; p[3 * i + 1] = 0.2f * i; p[3 * i + 2] = 1.0f + 0.6f * i;
        v[3 * i] = i == 2 ? 0.0f : 1.0f; v[3 * i + 1] = 0.0f; v[3 * i + 2] = i == 2 ? 0.0f : -0.3f;      /* drone 2 stands still */
        const float a = i == N - 1 ? 1.5707963f : 0.1f * i;                                            /* the last one looks away */
        q[4 * i] = cosf(a); q[4 * i + 1] = 0.0f; q[4 * i + 2] = 0.0f; q[4 * i + 3] = sinf(a);
    }
    const size_t ld = N + PAD;
    float* rows = (float*)malloc(FPV_PID_ROWS * ld * sizeof(float));
    for (size_t k = 0; k < FPV_PID_ROWS * ld; ++k) rows[k] = k % ld >= N ? -7.0f : (k / ld == FPV_PID_IS_FIRST ? 1.0f : 0.0f);
    float* rot = (float*)malloc(N * 9 * sizeof(float));
    float* thrust = (float*)malloc(N * sizeof(float));
    float* pix = (float*)malloc(N * 2 * sizeof(float));
    uint8_t* vis = (uint8_t*)malloc(N);
    s.pid_state = rows; s.pid_ld = (int64_t)ld; s.rotation = rot; s.thrust = thrust; s.pixel_out = pix; s.visible = vis;

    check(fpv_chase_eval(&s, N, p, v, q) == FPV_OK, "fpv_chase_eval, the pixel found");
    int seen = 0, ortho = 1, unseen_ok = 1, padding = 1;
    for (int i = 0; i < N; ++i) {
        const float* R = rot + 9 * i;
        if (vis[i]) {
            ++seen;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const double d = (double)R[a] * R[b] + (double)R[3 + a] * R[3 + b] + (double)R[6 + a] * R[6 + b];
                    ortho = ortho && fabs(d - (a == b)) < 1e-5;
                }
            ortho = ortho && isfinite(thrust[i]) && thrust[i] > 0.0f && rows[FPV_PID_IS_FIRST * ld + i] == 0.0f;
        } else {
            unseen_ok = unseen_ok && isnan(thrust[i]) && isnan(pix[2 * i]) && R[0] == 1.0f && R[4] == 1.0f && R[8] == 1.0f && R[1] == 0.0f
                        && rows[FPV_PID_IS_FIRST * ld + i] == 1.0f;
        }
    }
    for (size_t k = 0; k < FPV_PID_ROWS * ld; ++k)
        if (k % ld >= N) padding = padding && rows[k] == -7.0f;
    check(seen >= 3 && seen < N, "some drones see the target, the one that looks away does not");
    check(ortho, "a guided drone gets an orthonormal matrix, a positive force and an advanced PID");
    check(unseen_ok, "an unguided drone gets the identity, NaN force and pixel, and keeps its PID rows");
    check(padding, "the padding of the PID rows is untouched");

    float* given = NULL;
    check(posix_memalign((void**)&given, 8, N * 2 * sizeof(float)) == 0, "aligned pixels");
    for (int i = 0; i < N; ++i) { given[2 * i] = 300.0f + 10.0f * i; given[2 * i + 1] = i == 1 ? NAN : 200.0f; }
    s.pixel = given; s.ref_frame = FPV_CHASE_DRONE; s.mode = FPV_CHASE_FRONTARGET;
    check(fpv_chase_eval(&s, N, p, v, q) == FPV_OK, "fpv_chase_eval, the pixel given, drone frame, frontarget");
    int given_ok = 1;
    for (int i = 0; i < N; ++i) given_ok = given_ok && vis[i] == (i != 1) && (i == 1 ? isnan(thrust[i]) : isfinite(thrust[i]) && pix[2 * i] == given[2 * i]);
    check(given_ok, "a NaN pixel is an unseen target; the others are used as given");

    s.mode = 7;
    check(fpv_chase_eval(&s, N, p, v, q) == FPV_EINVAL && strstr(fpv_last_error(), "unknown mode") != NULL, "a refusal names its reason");

    free(given); free(vis); free(pix); free(thrust); free(rot); free(rows); free(q); free(v); free(p);
    return failures ? 1 : 0;
}
