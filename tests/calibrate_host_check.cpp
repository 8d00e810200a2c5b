// Stand-alone check of the host side of ltg_hist_groups and ltg_topk_calibrate under a sanitizer: argument validation and the host read
// of list_class, i.e. only the paths that return before any HIP call (no GPU is needed, no kernel is launched).  Not part of the pytest
// suite (it recompiles the library's translation unit); build and run by hand from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -o /tmp/calibrate_host_check tests/calibrate_host_check.cpp long-tail-gan_amd/csrc/ltg_kernels.hip && /tmp/calibrate_host_check
//
// Prints "calibrate host check: ok" and exits 0; any sanitizer report or failed expectation makes the exit status non-zero.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ltg.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "line %d: expectation failed: %s\n", __LINE__, #cond); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// list_class in a heap block of exactly n entries: a host read past the end is the sanitizer's to find
static int cal(int32_t n_rows, int32_t n_lists, int32_t m_in, const int32_t* cls, int n_cls, int32_t n_groups, float lambda, int32_t k,
               const float* sg, const int32_t* ig, const int32_t* hist, float* so, int32_t* io, float* st) {
    int32_t* lc = NULL;
    if (cls) {
        lc = (int32_t*)malloc((n_cls > 0 ? n_cls : 1) * sizeof(int32_t));
        memcpy(lc, cls, n_cls * sizeof(int32_t));
    }
    const int rc = ltg_topk_calibrate(n_rows, n_lists, m_in, sg, ig, lc, n_groups, hist, lambda, k, so, io, st, NULL);
    free(lc);
    return rc;
}

int main(void) {
    float* f = (float*)malloc(2 * 2 * 8 * sizeof(float));
    int32_t* ids = (int32_t*)malloc(2 * 2 * 8 * sizeof(int32_t));
    int32_t* hist = (int32_t*)malloc(2 * 3 * sizeof(int32_t));
    float* so = (float*)malloc(2 * 4 * sizeof(float));
    int32_t* io = (int32_t*)malloc(2 * 4 * sizeof(int32_t));
    float* st = (float*)malloc(2 * 2 * sizeof(float));
    int32_t* ptr = (int32_t*)malloc(3 * sizeof(int32_t));
    uint8_t* lab = (uint8_t*)malloc(16);
    memset(ids, 0, 2 * 2 * 8 * sizeof(int32_t));
    memset(hist, 0, 2 * 3 * sizeof(int32_t));
    memset(ptr, 0, 3 * sizeof(int32_t));
    memset(lab, 0, 16);
    const int32_t c02[] = {0, 2};

    // ---- ltg_topk_calibrate
    EXPECT(cal(0, 2, 8, c02, 2, 2, 0.5f, 4, f, ids, hist, so, io, NULL) == LTG_OK);
    EXPECT(cal(0, 2, 8, c02, 2, 2, 0.5f, 4, f, ids, hist, so, io, st) == LTG_OK);
    EXPECT(cal(2, 2, 8, c02, 2, 2, 0.5f, 4, NULL, ids, hist, so, io, st) == LTG_EINVAL);
    EXPECT(cal(2, 2, 8, c02, 2, 2, 0.5f, 4, f, NULL, hist, so, io, st) == LTG_EINVAL);
    EXPECT(cal(2, 2, 8, NULL, 0, 2, 0.5f, 4, f, ids, hist, so, io, st) == LTG_EINVAL);
    EXPECT(cal(2, 2, 8, c02, 2, 2, 0.5f, 4, f, ids, NULL, so, io, st) == LTG_EINVAL);
    EXPECT(cal(2, 2, 8, c02, 2, 2, 0.5f, 4, f, ids, hist, NULL, io, st) == LTG_EINVAL);
    EXPECT(cal(2, 2, 8, c02, 2, 2, 0.5f, 4, f, ids, hist, so, NULL, st) == LTG_EINVAL);
    const int32_t bad_g[] = {0, -1, 9, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_g / sizeof bad_g[0]; ++i) EXPECT(cal(2, 1, 8, c02, 1, bad_g[i], 0.5f, 4, f, ids, hist, so, io, st) == LTG_EINVAL);
    // n_lists is refused before list_class is read: the block holds two entries only
    const int32_t bad_l[] = {0, -1, 4, 10, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_l / sizeof bad_l[0]; ++i) EXPECT(cal(2, bad_l[i], 8, c02, 2, 2, 0.5f, 4, f, ids, hist, so, io, st) == LTG_EINVAL);
    const int32_t bad_m[] = {0, -1, 1025, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_m / sizeof bad_m[0]; ++i) EXPECT(cal(2, 2, bad_m[i], c02, 2, 2, 0.5f, 1, f, ids, hist, so, io, st) == LTG_EINVAL);
    const int32_t bad_k[] = {0, -1, 9, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_k / sizeof bad_k[0]; ++i) EXPECT(cal(2, 2, 8, c02, 2, 2, 0.5f, bad_k[i], f, ids, hist, so, io, st) == LTG_EINVAL);
    const float bad_lam[] = {-1e-6f, 1.0f + 1e-6f, NAN, INFINITY, -INFINITY};
    for (size_t i = 0; i < sizeof bad_lam / sizeof bad_lam[0]; ++i) EXPECT(cal(2, 2, 8, c02, 2, 2, bad_lam[i], 4, f, ids, hist, so, io, st) == LTG_EINVAL);
    const int32_t bad_c[][2] = {{1, 1}, {2, 0}, {-1, 0}, {0, 3}, {0, INT32_MAX}, {INT32_MIN, 0}};
    for (size_t i = 0; i < sizeof bad_c / sizeof bad_c[0]; ++i) EXPECT(cal(2, 2, 8, bad_c[i], 2, 2, 0.5f, 4, f, ids, hist, so, io, st) == LTG_EINVAL);
    EXPECT(cal(-1, 2, 8, c02, 2, 2, 0.5f, 4, f, ids, hist, so, io, st) == LTG_EINVAL);
    // zero rows: nothing is launched, but the arguments are still checked
    const int32_t all9[] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    EXPECT(cal(0, 9, 1024, all9, 9, 8, 1.0f, 1024, f, ids, hist, so, io, st) == LTG_OK);
    EXPECT(cal(0, 2, 8, c02, 2, 2, 0.0f, 8, f, ids, hist, so, io, st) == LTG_OK);
    EXPECT(cal(0, 2, 8, c02, 2, 2, 0.5f, 9, f, ids, hist, so, io, st) == LTG_EINVAL);
    EXPECT(cal(0, 2, 8, bad_c[1], 2, 2, 0.5f, 4, f, ids, hist, so, io, st) == LTG_EINVAL);

    // ---- ltg_hist_groups
    ltg_batch tr;
    memset(&tr, 0, sizeof tr);
    tr.n_rows = 2;
    tr.indptr = ptr;
    tr.indices = ptr;
    ltg_batch none = tr;
    none.n_rows = 0;
    EXPECT(ltg_hist_groups(&none, 0, 0, lab, 16, 2, hist, NULL) == LTG_OK);
    EXPECT(ltg_hist_groups(&none, INT32_MAX, 0, lab, INT32_MAX, 8, hist, NULL) == LTG_OK);
    EXPECT(ltg_hist_groups(NULL, 0, 2, lab, 16, 2, hist, NULL) == LTG_EINVAL);
    EXPECT(ltg_hist_groups(&tr, 0, 2, NULL, 16, 2, hist, NULL) == LTG_EINVAL);
    EXPECT(ltg_hist_groups(&tr, 0, 2, lab, 16, 2, NULL, NULL) == LTG_EINVAL);
    ltg_batch t2 = tr;
    t2.indptr = NULL;
    EXPECT(ltg_hist_groups(&t2, 0, 2, lab, 16, 2, hist, NULL) == LTG_EINVAL);
    t2 = tr;
    t2.indices = NULL;
    EXPECT(ltg_hist_groups(&t2, 0, 2, lab, 16, 2, hist, NULL) == LTG_EINVAL);
    t2 = tr;
    t2.n_rows = 3;
    EXPECT(ltg_hist_groups(&t2, 0, 2, lab, 16, 2, hist, NULL) == LTG_EINVAL);
    EXPECT(ltg_hist_groups(&tr, 0, 3, lab, 16, 2, hist, NULL) == LTG_EINVAL);
    t2.n_rows = -1;
    EXPECT(ltg_hist_groups(&t2, 0, -1, lab, 16, 2, hist, NULL) == LTG_EINVAL);
    EXPECT(ltg_hist_groups(&tr, -1, 2, lab, 16, 2, hist, NULL) == LTG_EINVAL);
    EXPECT(ltg_hist_groups(&tr, 0, 2, lab, 0, 2, hist, NULL) == LTG_EINVAL);
    EXPECT(ltg_hist_groups(&tr, 0, 2, lab, -16, 2, hist, NULL) == LTG_EINVAL);
    for (size_t i = 0; i < sizeof bad_g / sizeof bad_g[0]; ++i) EXPECT(ltg_hist_groups(&tr, 0, 2, lab, 16, bad_g[i], hist, NULL) == LTG_EINVAL);
    EXPECT(ltg_hist_groups(&none, 0, 0, lab, 16, 9, hist, NULL) == LTG_EINVAL);
    free(lab);
    free(ptr);
    free(st);
    free(io);
    free(so);
    free(hist);
    free(ids);
    free(f);
    if (failures) {
        fprintf(stderr, "calibrate host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("calibrate host check: ok\n");
    return 0;
}
