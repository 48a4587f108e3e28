/* depth_eval.c - a plain C host of the depth camera's host functions (include/fpv_abi.h "Depth camera"): fpv_camera_derive and
 * fpv_depth_eval on a small scene, no GPU.  Also the program tests/test_depth_sanitized.py builds with AddressSanitizer and
 * UndefinedBehaviorSanitizer around the library's host code:
 *
 *   hipcc --offload-arch=gfx950 -O1 -Xarch_host -fsanitize=address,undefined -ffp-contract=off -std=c++17 \
 *         -c fpyv_amd/csrc/fpv_hip.hip -o fpv_host.o
 *   clang -O1 -fsanitize=address,undefined -Iinclude -c examples/c_host/depth_eval.c -o depth_eval.o
 *   hipcc -fsanitize=address,undefined fpv_host.o depth_eval.o -o depth_eval && ./depth_eval
 *
 * (the sanitizers instrument the host half of fpv_hip.hip only; nothing here touches a device)
 * Every buffer is sized exactly (heap, so that a byte past an image or a descriptor row is caught), the image stride carries
 * padding that must stay untouched, and both encodings run.  Prints one line per check and returns 0 when all hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fpv_abi.h"

#define W 12
#define H 8
#define N 5
#define PAD 4

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
    cam.pitch_deg = 35.0; cam.fov_deg = 120.0; cam.width = W; cam.height = H;
    cam.relative_position[0] = 0.1;
    fpv_depth_render_t r;
    memset(&r, 0, sizeof r);
    check(fpv_camera_derive(&cam, &r) == FPV_OK, "fpv_camera_derive");
    check(fabs(r.focal_length - W / (2.0 * tan(60.0 * 3.14159265358979323846 / 180.0))) < 1e-12, "focal length");
    r.struct_size = (uint32_t)fpv_sizeof(7);
    r.max_depth = 25.0f; r.gate_frame_width = 0.15f;

    fpv_objects_t* objs = (fpv_objects_t*)calloc(1, sizeof *objs);
    objs->count = 3;
    objs->obj[0].type = FPV_OBJ_GROUND;
    objs->obj[1].type = FPV_OBJ_CYLINDER; objs->obj[1].x = 3.0f; objs->obj[1].radius = 1.0f; objs->obj[1].height = 5.0f;
    objs->obj[2].type = FPV_OBJ_SPHERE; objs->obj[2].x = 1.5f; objs->obj[2].y = -2.0f; objs->obj[2].z = 3.0f; objs->obj[2].radius = 0.8f;
    r.objects = objs;

    enum { GATES = 3 };
    fpv_gate_t* gates = (fpv_gate_t*)calloc(GATES, sizeof *gates);
    for (int g = 0; g < GATES; ++g) {
        gates[g].position[0] = 2.0 + g; gates[g].position[1] = 0.5 * g; gates[g].position[2] = 2.5;
        gates[g].rotation[0] = gates[g].rotation[4] = gates[g].rotation[8] = 1.0;
        gates[g].size = 1.5; gates[g].shape = g;
    }
    float* rows = NULL;
    check(posix_memalign((void**)&rows, 16, GATES * FPV_GATE_FLOATS * sizeof(float)) == 0, "aligned descriptor rows");
    check(fpv_gates_derive(GATES, gates, rows) == FPV_OK, "fpv_gates_derive");
    r.gate_descriptors = rows; r.gate_count = GATES;

    float* p = (float*)malloc(N * 3 * sizeof(float));
    float* q = (float*)malloc(N * 4 * sizeof(float));
    for (int i = 0; i < N; ++i) {
        p[3 * i] = -1.0f + 0.7f * i; p[3 * i + 1] = 0.3f * i; p[3 * i + 2] = i == 4 ? -0.5f : 1.0f + 0.5f * i;   /* the last one below the ground */
        const float a = 0.2f * i;
        q[4 * i] = cosf(a); q[4 * i + 1] = 0.0f; q[4 * i + 2] = 0.0f; q[4 * i + 3] = sinf(a);
    }

    const size_t stride = W * H + PAD;
    float* metres = (float*)malloc(N * stride * sizeof(float));
    for (size_t k = 0; k < N * stride; ++k) metres[k] = -1.0f;
    r.encoding = FPV_DEPTH_METRES; r.image = metres; r.image_stride = (int64_t)stride;
    check(fpv_depth_eval(&r, N, p, q) == FPV_OK, "fpv_depth_eval, metres");
    int in_range = 1, padding = 1, hit = 0;
    for (int i = 0; i < N; ++i)
        for (size_t k = 0; k < stride; ++k) {
            const float d = metres[i * stride + k];
            if (k >= (size_t)(W * H)) padding = padding && d == -1.0f;
            else { in_range = in_range && d >= 0.0f && d <= 25.0f; hit += d < 25.0f; }
        }
    check(in_range, "every depth is in [0, max_depth]");
    check(padding, "the padding of the stride is untouched");
    check(hit > 0, "something is seen");
    int inside = 1;
    for (int k = 0; k < W * H; ++k) inside = inside && metres[4 * stride + k] == 0.0f;
    check(inside, "a camera below the ground reports 0 everywhere");

    uint8_t* bytes = (uint8_t*)malloc(N * stride);
    memset(bytes, 7, N * stride);
    r.encoding = FPV_DEPTH_U8; r.image = bytes;
    check(fpv_depth_eval(&r, N, p, q) == FPV_OK, "fpv_depth_eval, bytes");
    int agree = 1;
    padding = 1;
    for (int i = 0; i < N; ++i)
        for (size_t k = 0; k < stride; ++k) {
            if (k >= (size_t)(W * H)) { padding = padding && bytes[i * stride + k] == 7; continue; }
            const float v = 255.0f * (1.0f - metres[i * stride + k] / 25.0f);
            agree = agree && bytes[i * stride + k] == (uint8_t)v;
        }
    check(agree, "the byte is (uint8)(255 (1 - depth / max_depth)) in fp32");
    check(padding, "the padding of the byte stride is untouched");

    r.gate_count = FPV_MAX_GATES + 1;
    check(fpv_depth_eval(&r, N, p, q) == FPV_EINVAL && strstr(fpv_last_error(), "gate_count") != NULL, "a refusal names its reason");

    free(bytes); free(metres); free(q); free(p); free(rows); free(gates); free(objs);
    return failures ? 1 : 0;
}
