/* detect_eval.c - a plain C host of the object detections' host functions (include/fpv_abi.h "Object detections"):
 * fpv_boxes_derive, fpv_detect_derive and fpv_detect_eval on a few drones, no GPU.  Also the program tests/test_detect_sanitized.py
 * builds with AddressSanitizer and UndefinedBehaviorSanitizer around the library's host code:
 *
 *   hipcc --offload-arch=gfx950 -O1 -Xarch_host -fsanitize=address,undefined -ffp-contract=off -std=c++17 \
 *         -c fpyv_amd/csrc/fpv_hip.hip -o fpv_host.o          (and the same for fpyv_amd/csrc/fpv_detect.hip -o fpv_detect.o)
 *   clang -O1 -fsanitize=address,undefined -Iinclude -c examples/c_host/detect_eval.c -o detect_eval.o
 *   hipcc -fsanitize=address,undefined fpv_host.o fpv_detect.o detect_eval.o -o detect_eval && ./detect_eval
 *
 * (the sanitizers instrument the host halves only; nothing here touches a device)
 * Every output is sized exactly (heap, so that a byte past it is caught) and carries a padded stride that must stay untouched; the
 * detection runs with 1 slot, with the full 72, with the own-target slot alone and after a table.  Prints one line per check and
 * returns 0 when all hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fpv_abi.h"

#define N 5
#define LD 8            /* padded: columns N..LD-1 stay as they were */
#define SENTINEL (-7.0f)

static int failures = 0;

static void check(int ok, const char* what)
{
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) ++failures;
}

/* exactly sized outputs for m slots, filled with the sentinel */
static void outputs(fpv_detect_t* s, int m)
{
    float* b = (float*)malloc((size_t)m * 4 * LD * sizeof(float));
    float* d = (float*)malloc((size_t)m * LD * sizeof(float));
    uint8_t* v = (uint8_t*)malloc((size_t)m * LD);
    for (int k = 0; k < m * 4 * LD; ++k) b[k] = SENTINEL;
    for (int k = 0; k < m * LD; ++k) { d[k] = SENTINEL; v[k] = 9; }
    s->boxes = b; s->box_depth = d; s->box_visible = v; s->ld = LD;
}

static int padding_untouched(const fpv_detect_t* s, int m)
{
    int ok = 1;
    for (int r = 0; r < m; ++r)
        for (int i = N; i < LD; ++i) {
            for (int k = 0; k < 4; ++k) ok = ok && s->boxes[((size_t)r * 4 + k) * LD + i] == SENTINEL;
            ok = ok && s->box_depth[(size_t)r * LD + i] == SENTINEL && s->box_visible[(size_t)r * LD + i] == 9;
        }
    return ok;
}

static int written(const fpv_detect_t* s, int m)
{
    int ok = 1;
    for (int r = 0; r < m; ++r)
        for (int i = 0; i < N; ++i) {
            for (int k = 0; k < 4; ++k) ok = ok && s->boxes[((size_t)r * 4 + k) * LD + i] != SENTINEL;
            ok = ok && s->box_depth[(size_t)r * LD + i] >= 0.0f && s->box_visible[(size_t)r * LD + i] <= 1;
        }
    return ok;
}

static void release(fpv_detect_t* s)
{
    free(s->boxes); free(s->box_depth); free(s->box_visible);
    s->boxes = NULL; s->box_depth = NULL; s->box_visible = NULL;
}

int main(void)
{
    fpv_camera_t cam;
    memset(&cam, 0, sizeof cam);
    cam.pitch_deg = 35.0; cam.fov_deg = 120.0; cam.width = 640; cam.height = 480;       /* the reference's camera */
    cam.relative_position[0] = 0.1;
    fpv_detect_t s;
    memset(&s, 0, sizeof s);
    check(fpv_detect_derive(&cam, &s) == FPV_OK, "fpv_detect_derive accepts 640 x 480");
    check(fabs(s.focal_length - 640 / (2.0 * tan(60.0 * 3.14159265358979323846 / 180.0))) < 1e-12, "focal length");
    s.struct_size = (uint32_t)fpv_sizeof(14);
    s.pixel_mode = FPV_DETECT_INT;

    /* the world: a ground, two cylinders, a sphere; 64 gates of the three shapes on a circle */
    fpv_objects_t objs;
    memset(&objs, 0, sizeof objs);
    objs.count = 4;
    objs.obj[0].type = FPV_OBJ_GROUND;
    objs.obj[1].type = FPV_OBJ_CYLINDER; objs.obj[1].x = 6.0f; objs.obj[1].y = 1.0f; objs.obj[1].radius = 0.5f; objs.obj[1].height = 3.0f;
    objs.obj[2].type = FPV_OBJ_CYLINDER; objs.obj[2].x = 9.0f; objs.obj[2].y = -2.0f; objs.obj[2].radius = 1.0f; objs.obj[2].height = 5.0f;
    objs.obj[3].type = FPV_OBJ_SPHERE; objs.obj[3].x = 7.0f; objs.obj[3].z = 3.0f; objs.obj[3].radius = 0.8f;
    double ground[4] = {60.0, 0.0, 0.0, 0.0};
    fpv_gate_t* gates = (fpv_gate_t*)calloc(FPV_MAX_GATES, sizeof(fpv_gate_t));
    for (int g = 0; g < FPV_MAX_GATES; ++g) {
        const double th = 2.0 * 3.14159265358979323846 * g / FPV_MAX_GATES, c = cos(th + 1.5707963267948966), sn = sin(th + 1.5707963267948966);
        gates[g].position[0] = 12.0 * cos(th); gates[g].position[1] = 12.0 * sin(th); gates[g].position[2] = 2.0;
        const double R[9] = {c, -sn, 0.0, sn, c, 0.0, 0.0, 0.0, 1.0};
        memcpy(gates[g].rotation, R, sizeof R);
        gates[g].size = 2.0; gates[g].shape = g % 3;
    }
    fpv_boxes_t* table = (fpv_boxes_t*)malloc(sizeof(fpv_boxes_t));
    check(fpv_sizeof(16) == (int)sizeof(fpv_boxes_t), "fpv_sizeof(16) is fpv_boxes_t");
    check(fpv_boxes_derive(&objs, ground, gates, FPV_MAX_GATES, 17, table) == FPV_OK && table->count == 68, "fpv_boxes_derive: 4 objects and 64 gates");
    check(table->box[0][0] == -30.0f && table->box[0][3] == 30.0f && table->box[0][2] == 0.0f && table->box[0][5] == 0.0f, "the ground's box");
    check(table->box[1][0] == 5.5f && table->box[1][4] == 1.5f && table->box[1][5] == 3.0f, "a cylinder's box");
    check(fabsf(table->box[4][2] - 1.0f) < 1e-6f && fabsf(table->box[4][5] - 3.0f) < 1e-6f, "gate 0 (rectangle): z from 1 to 3");
    check(fabsf(table->box[6][2] - 1.0f) < 1e-6f && fabsf(table->box[6][5] - 3.0f) < 1e-6f, "gate 2 (half circle, radius = size, shifted down by size / 2): z from 1 to 3");

    float* p = (float*)malloc(N * 3 * sizeof(float));
    float* q = (float*)malloc(N * 4 * sizeof(float));
    for (int i = 0; i < N; ++i) {
        p[3 * i] = -1.0f + 0.5f * i; p[3 * i + 1] = 0.2f * i; p[3 * i + 2] = 1.0f + 0.6f * i;
        const float h = 0.3f * i;                                   /* a yaw of 0.6 i radians */
        q[4 * i] = cosf(h); q[4 * i + 1] = 0.0f; q[4 * i + 2] = 0.0f; q[4 * i + 3] = sinf(h);
    }

    /* 1 slot */
    fpv_boxes_t* one = (fpv_boxes_t*)calloc(1, sizeof(fpv_boxes_t));
    one->count = 1;
    memcpy(one->box[0], table->box[2], sizeof one->box[0]);
    s.table = one;
    outputs(&s, 1);
    check(fpv_detect_eval(&s, N, p, q) == FPV_OK, "fpv_detect_eval: 1 slot");
    check(written(&s, 1) && padding_untouched(&s, 1), "1 slot: every drone written, the padding untouched");
    /* its nearest corner (8, -3, 0) is 8.9 m ahead of and 1 m below the camera, which looks up by 35 degrees: 8.9 cos 35 - sin 35 */
    check(s.box_visible[0] == 1 && fabsf(s.box_depth[0] - 6.717f) < 0.01f, "drone 0 sees the cylinder ahead of it, 6.72 m deep");
    float first[4];
    for (int k = 0; k < 4; ++k) first[k] = s.boxes[(size_t)k * LD];
    check(first[0] <= first[2] && first[1] <= first[3] && first[0] == truncf(first[0]), "its box is ordered, in whole pixels");
    release(&s);

    /* 72 slots: the table filled up with copies */
    fpv_boxes_t* full = (fpv_boxes_t*)malloc(sizeof(fpv_boxes_t));
    memcpy(full, table, sizeof *full);
    for (int m = 68; m < FPV_MAX_BOXES; ++m) memcpy(full->box[m], table->box[m - 66], sizeof full->box[m]);
    full->count = FPV_MAX_BOXES;
    s.table = full;
    outputs(&s, FPV_MAX_BOXES);
    check(fpv_detect_eval(&s, N, p, q) == FPV_OK, "fpv_detect_eval: 72 slots");
    check(written(&s, FPV_MAX_BOXES) && padding_untouched(&s, FPV_MAX_BOXES), "72 slots: every drone written, the padding untouched");
    int same = 1;
    for (int k = 0; k < 4; ++k) same = same && s.boxes[((size_t)2 * 4 + k) * LD] == first[k] && s.boxes[((size_t)68 * 4 + k) * LD] == first[k];
    check(same, "slot 2 and its copy in slot 68 equal the 1-slot result");
    int seen = 0;
    for (int m = 0; m < FPV_MAX_BOXES; ++m) seen += s.box_visible[(size_t)m * LD];
    check(seen > 4 && seen < FPV_MAX_BOXES, "drone 0 sees some of the gates, not all");
    release(&s);

    /* the own-target slot: alone, and after the table, with a radius row and with one radius */
    const size_t tld = N + 3;
    float* target = (float*)malloc(3 * tld * sizeof(float));
    float* radius = (float*)malloc(N * sizeof(float));
    for (size_t k = 0; k < 3 * tld; ++k) target[k] = SENTINEL;
    for (int i = 0; i < N; ++i) {
        target[i] = p[3 * i] + 5.0f; target[tld + i] = p[3 * i + 1]; target[2 * tld + i] = p[3 * i + 2] + 2.0f;
        radius[i] = 0.3f + 0.1f * i;
    }
    s.table = NULL; s.target_rows = target; s.target_ld = (int64_t)tld; s.target_radius = radius; s.pixel_mode = FPV_DETECT_FLOAT;
    outputs(&s, 1);
    check(fpv_detect_eval(&s, N, p, q) == FPV_OK, "fpv_detect_eval: the own-target slot alone");
    check(written(&s, 1) && padding_untouched(&s, 1) && s.box_visible[0] == 1, "own slot: written, the padding untouched, drone 0 sees its target");
    float own[4];
    for (int k = 0; k < 4; ++k) own[k] = s.boxes[(size_t)k * LD + 1];
    release(&s);
    s.table = table; s.clip = 1;
    outputs(&s, 69);
    check(fpv_detect_eval(&s, N, p, q) == FPV_OK, "fpv_detect_eval: 68 slots and the own target, clipped");
    check(written(&s, 69) && padding_untouched(&s, 69), "69 slots: every drone written, the padding untouched");
    int clipped = 1;
    for (int k = 0; k < 4; ++k) {
        const float hi = (k & 1) ? 480.0f : 640.0f, raw = own[k] < 0.0f ? 0.0f : own[k] > hi ? hi : own[k];
        clipped = clipped && s.boxes[((size_t)68 * 4 + k) * LD + 1] == (s.box_visible[(size_t)68 * LD + 1] ? raw : own[k]);
    }
    check(clipped, "the last slot is the own target's box, clamped to the image where visible");
    release(&s);
    s.target_radius = NULL; s.target_radius_all = 0.5f; s.clip = 0;
    outputs(&s, 69);
    check(fpv_detect_eval(&s, N, p, q) == FPV_OK && written(&s, 69), "one radius for all");
    release(&s);

    /* refusals */
    s.target_rows = NULL; s.table = full; full->count = 73;
    outputs(&s, 1);
    check(fpv_detect_eval(&s, N, p, q) < 0 && strstr(fpv_last_error(), "not 73") != NULL, "73 boxes are refused by name");
    full->count = 72; full->box[7][1] = NAN;
    check(fpv_detect_eval(&s, N, p, q) < 0 && strstr(fpv_last_error(), "box 7 is not finite") != NULL, "a NaN box is refused by name");
    full->box[7][1] = 9.0f; full->box[7][4] = 8.0f;
    check(fpv_detect_eval(&s, N, p, q) < 0 && strstr(fpv_last_error(), "box 7 has min > max") != NULL, "min > max is refused by name");
    s.table = one; s.ld = 6;
    check(fpv_detect_eval(&s, N, p, q) < 0 && strstr(fpv_last_error(), "multiple of 4") != NULL, "a stride that is no multiple of 4 is refused");
    s.ld = 4;
    check(fpv_detect_eval(&s, N, p, q) < 0 && strstr(fpv_last_error(), "smaller than the number of drones") != NULL, "a stride below n is refused");
    release(&s);

    free(p); free(q); free(target); free(radius); free(gates); free(table); free(one); free(full);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
