/* splat_eval.c - a plain C host of the point-cloud camera's host functions (include/fpv_abi.h "Point-cloud camera"):
 * fpv_splat_derive, fpv_cloud_derive and fpv_splat_eval on a few drones, no GPU.  Also the program tests/test_splat_sanitized.py
 * builds with AddressSanitizer and UndefinedBehaviorSanitizer around the library's host code:
 *
 *   hipcc --offload-arch=gfx950 -O1 -Xarch_host -fsanitize=address,undefined -ffp-contract=off -std=c++17 \
 *         -c fpyv_amd/csrc/fpv_hip.hip -o fpv_host.o     (and the same for fpv_detect.hip -o fpv_detect.o, fpv_splat.hip -o fpv_splat.o)
 *   clang -O1 -fsanitize=address,undefined -Iinclude -c examples/c_host/splat_eval.c -o splat_eval.o
 *   hipcc -fsanitize=address,undefined fpv_host.o fpv_detect.o fpv_splat.o splat_eval.o -o splat_eval && ./splat_eval
 *
 * (the sanitizers instrument the host halves only; nothing here touches a device)
 * Every buffer is sized exactly (heap, so that a byte past it is caught); the image and the points carry a padded stride that must
 * stay untouched or unread (the points' padding holds NaN); the render runs with one object, with the full 72, with an object
 * without points and in all three encodings.  Prints one line per check and returns 0 when all hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fpv_abi.h"

#define N 3
#define W 16
#define H 12
#define IMAGE_LD (W * H + 8)      /* padded: elements W * H .. IMAGE_LD - 1 of every drone stay as they were */

static int failures = 0;

static void check(int ok, const char* what)
{
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) ++failures;
}

/* one drone above the origin looking along +x, one turned about z, one upside down */
static const float P[N][3] = {{0.0f, 0.0f, 2.0f}, {-3.0f, 1.0f, 1.5f}, {2.0f, -2.0f, 3.0f}};
static const float Q[N][4] = {{1.0f, 0.0f, 0.0f, 0.0f}, {0.9238795f, 0.0f, 0.0f, 0.3826834f}, {0.0f, 1.0f, 0.0f, 0.0f}};

/* the local box of object m of a cloud: min and max of its points */
static void box_of(fpv_splat_t* s, const float* pts, int64_t ld, int m)
{
    float* b = s->box[m];
    for (int a = 0; a < 3; ++a) { b[a] = 0.0f; b[3 + a] = 0.0f; }
    for (int j = s->first[m]; j < s->first[m + 1]; ++j)
        for (int a = 0; a < 3; ++a) {
            const float x = pts[a * ld + j];
            if (j == s->first[m] || x < b[a]) b[a] = x;
            if (j == s->first[m] || x > b[3 + a]) b[3 + a] = x;
        }
}

static int render_bytes(fpv_splat_t* s, const char* what, int expect_some)
{
    uint8_t* img = (uint8_t*)malloc((size_t)N * IMAGE_LD);
    float* cen = (float*)malloc(sizeof(float) * 2 * N);
    int32_t* lit = (int32_t*)malloc(sizeof(int32_t) * N);
    memset(img, 0xAB, (size_t)N * IMAGE_LD);
    s->image = img; s->image_ld = IMAGE_LD; s->centroid = cen; s->lit = lit;
    const int rc = fpv_splat_eval(s, N, &P[0][0], &Q[0][0]);
    int ok = rc == FPV_OK, some = 0;
    if (rc != FPV_OK) printf("  %s\n", fpv_last_error());
    for (int i = 0; ok && i < N; ++i) {
        int count = 0;
        for (int k = 0; k < W * H; ++k) {
            const uint8_t v = img[(size_t)i * IMAGE_LD + k];
            if (s->encoding == FPV_SPLAT_MASK) ok = ok && v <= 1;
            count += s->encoding == FPV_SPLAT_MASK ? 0 : v > 0;
            some += v > 0;
        }
        for (int k = W * H; k < IMAGE_LD; ++k) ok = ok && img[(size_t)i * IMAGE_LD + k] == 0xAB;
        if (s->encoding == FPV_SPLAT_U8) ok = ok && lit[i] == count;
        ok = ok && (lit[i] > 0 ? (cen[2 * i] >= 0.0f && cen[2 * i] <= W - 1 && cen[2 * i + 1] >= 0.0f && cen[2 * i + 1] <= H - 1)
                               : (isnan(cen[2 * i]) && isnan(cen[2 * i + 1])));
    }
    ok = ok && (expect_some ? some > 0 : some == 0);
    check(ok, what);
    free(img); free(cen); free(lit);
    s->image = NULL; s->centroid = NULL; s->lit = NULL;
    return ok;
}

int main(void)
{
    fpv_camera_t cam;
    memset(&cam, 0, sizeof cam);
    cam.pitch_deg = 35.0; cam.fov_deg = 120.0; cam.width = W; cam.height = H;
    cam.relative_position[0] = 0.1;
    fpv_splat_t s;
    memset(&s, 0, sizeof s);
    check(fpv_sizeof(18) == (int)sizeof(fpv_splat_t) && fpv_sizeof(17) < 0, "fpv_sizeof(18) is this struct, 17 is none");
    check(fpv_splat_derive(&cam, &s) == FPV_OK && s.width == W && s.height == H && s.focal_length > 0.0, "fpv_splat_derive fills the camera numbers");
    cam.width = 640; cam.height = 480;
    check(fpv_splat_derive(&cam, &s) == FPV_EPARAM, "fpv_splat_derive refuses 640 x 480");
    s.struct_size = sizeof s; s.max_depth = 25.0f; s.encoding = FPV_SPLAT_U8;

    /* ---- one object: a ground grid, exactly sized */
    const double ground[1] = {40.0};
    const int32_t gres[1] = {21};
    const int count = fpv_cloud_derive(FPV_CLOUD_GROUND, ground, gres, NULL, 0);
    check(count == 21 * 21, "fpv_cloud_derive counts the grid");
    int64_t ld = (count + 3) / 4 * 4 + 4;                                     /* padded */
    float* pts = (float*)malloc(sizeof(float) * 3 * (size_t)ld);
    for (int64_t k = 0; k < 3 * ld; ++k) pts[k] = NAN;                        /* the padding is never read: a NaN there changes nothing */
    check(fpv_cloud_derive(FPV_CLOUD_GROUND, ground, gres, pts, ld) == count && pts[0] == -20.0f && pts[ld + count - 1] == 20.0f &&
          pts[2 * ld + 7] == 0.0f && isnan(pts[count]), "fpv_cloud_derive writes the grid SoA and leaves the padding");
    check(fpv_cloud_derive(FPV_CLOUD_GROUND, ground, gres, pts, 8) == FPV_EALIGN, "fpv_cloud_derive refuses a short ld");
    s.object_count = 1; s.first[0] = 0; s.first[1] = count; s.points = pts; s.point_ld = ld;
    box_of(&s, pts, ld, 0);
    render_bytes(&s, "one object, u8, padded image_ld and point_ld", 1);
    s.encoding = FPV_SPLAT_MASK;
    render_bytes(&s, "one object, mask", 1);
    s.encoding = FPV_SPLAT_METRES;
    {
        float* img = (float*)malloc(sizeof(float) * (size_t)N * IMAGE_LD);
        for (int k = 0; k < N * IMAGE_LD; ++k) img[k] = -7.0f;
        s.image = img; s.image_ld = IMAGE_LD;
        int ok = fpv_splat_eval(&s, N, &P[0][0], &Q[0][0]) == FPV_OK;
        for (int i = 0; i < N; ++i) {
            for (int k = 0; k < W * H; ++k) ok = ok && img[i * IMAGE_LD + k] > 0.0f;
            for (int k = W * H; k < IMAGE_LD; ++k) ok = ok && img[i * IMAGE_LD + k] == -7.0f;
        }
        check(ok, "one object, metres, without centroid");
        free(img); s.image = NULL;
    }
    s.encoding = FPV_SPLAT_U8;
    /* the object moved beyond max_depth by its offset: whatever still lands encodes to 0 */
    s.offset[0][2] = -1000.0f; s.offset[0][0] = 5000.0f;
    render_bytes(&s, "the object beyond max_depth: dark images, NaN centroids", 0);
    s.offset[0][2] = 0.0f; s.offset[0][0] = 0.0f;
    free(pts);

    /* ---- 72 objects: 70 cylinders, an object without points, a gate; points exactly sized */
    int total = 0;
    int32_t cres[2] = {9, 4};
    const int32_t gate_res[2] = {FPV_GATE_CIRCLE, 17};
    ld = 70 * 36 + 18;
    ld = (ld + 3) / 4 * 4;
    pts = (float*)malloc(sizeof(float) * 3 * (size_t)ld);
    for (int64_t k = 0; k < 3 * ld; ++k) pts[k] = NAN;
    float* tmp = (float*)malloc(sizeof(float) * 3 * 36);
    int ok = 1;
    s.object_count = 72;
    for (int m = 0; m < 72; ++m) {
        s.first[m] = total;
        int got = 0;
        if (m < 70) {
            const double th = 6.283185307179586 * m / 70.0;
            const double cyl[5] = {8.0 * cos(th), 8.0 * sin(th), 0.0, 0.4, 3.0};
            got = fpv_cloud_derive(FPV_CLOUD_CYLINDER, cyl, cres, tmp, 36);
            ok = ok && got == 36;
        } else if (m == 71) {
            const double gate[13] = {4.0, 0.0, 2.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 2.0};
            got = fpv_cloud_derive(FPV_CLOUD_GATE, gate, gate_res, tmp, 36);
            ok = ok && got == 18;
        }
        for (int j = 0; j < got; ++j)
            for (int a = 0; a < 3; ++a) pts[a * ld + total + j] = tmp[a * 36 + j];
        total += got;
        s.first[m + 1] = total;
        box_of(&s, pts, ld, m);
    }
    free(tmp);
    check(ok && total == 70 * 36 + 18 && s.first[71] == s.first[70], "72 clouds derived, object 70 has no points");
    s.points = pts; s.point_ld = ld;
    render_bytes(&s, "72 objects, u8", 1);
    s.encoding = FPV_SPLAT_MASK;
    render_bytes(&s, "72 objects, mask", 1);
    s.encoding = FPV_SPLAT_U8;

    /* ---- refusals, by name */
    s.object_count = 73;
    check(fpv_splat_eval(&s, N, &P[0][0], &Q[0][0]) == FPV_EINVAL && strstr(fpv_last_error(), "not 73"), "73 objects are refused before anything is read");
    s.object_count = 72; s.first[5] = s.first[4] - 1;
    {
        uint8_t* img = (uint8_t*)malloc((size_t)N * IMAGE_LD);
        s.image = img; s.image_ld = IMAGE_LD;
        check(fpv_splat_eval(&s, N, &P[0][0], &Q[0][0]) == FPV_EPARAM && strstr(fpv_last_error(), "non-decreasing"), "a decreasing first is refused");
        s.first[5] = s.first[4] + 36; s.box[3][4] = NAN;
        check(fpv_splat_eval(&s, N, &P[0][0], &Q[0][0]) == FPV_EPARAM && strstr(fpv_last_error(), "box 3 is not finite"), "a NaN box is refused");
        box_of(&s, pts, ld, 3);
        s.point_ld = ld - 4;
        check(fpv_splat_eval(&s, N, &P[0][0], &Q[0][0]) == FPV_EALIGN, "a point_ld below first[M] is refused");
        s.point_ld = ld;
        free(img); s.image = NULL;
    }
    free(pts);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
