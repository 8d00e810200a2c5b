// Stand-alone check of the host side of ltg_topk_explain under a sanitizer: argument validation, i.e. only the paths that return before
// any HIP call (no GPU is needed, no kernel is launched).  Not part of the pytest suite (it recompiles the library's translation unit);
// build and run by hand from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -o /tmp/explain_host_check tests/explain_host_check.cpp long-tail-gan_amd/csrc/ltg_kernels.hip && /tmp/explain_host_check
//
// Prints "explain host check: ok" and exits 0; any sanitizer report or failed expectation makes the exit status non-zero.
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

int main(void) {
    // heap buffers of exactly the size a caller would pass: a host-side read or write of them past the end is the sanitizer's to find
    uint16_t* img = (uint16_t*)aligned_alloc(16, 4 * 608 * sizeof(uint16_t));
    float* f = (float*)malloc(2 * 4 * 3 * sizeof(float));
    int32_t* ids = (int32_t*)malloc(2 * 8 * sizeof(int32_t));
    int32_t* out = (int32_t*)malloc(2 * 4 * 3 * sizeof(int32_t));
    int32_t* ptr = (int32_t*)malloc(3 * sizeof(int32_t));
    memset(img, 0, 4 * 608 * sizeof(uint16_t));
    memset(ids, 0, 2 * 8 * sizeof(int32_t));
    memset(ptr, 0, 3 * sizeof(int32_t));
    ltg_batch tr;
    memset(&tr, 0, sizeof tr);
    tr.n_rows = 2;
    tr.indptr = ptr;
    tr.indices = ptr;
    ltg_batch none = tr;
    none.n_rows = 0;

    // NULL pointers
    EXPECT(ltg_topk_explain(NULL, 0, 4, &tr, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, NULL, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 2, 8, NULL, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 2, 8, ids, 4, 3, NULL, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 2, 8, ids, 4, 3, f, NULL, NULL) == LTG_EINVAL);
    ltg_batch t2 = tr;
    t2.indptr = NULL;
    EXPECT(ltg_topk_explain(img, 0, 4, &t2, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    t2 = tr;
    t2.indices = NULL;
    EXPECT(ltg_topk_explain(img, 0, 4, &t2, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    // rows
    t2 = tr;
    t2.n_rows = 3;
    EXPECT(ltg_topk_explain(img, 0, 4, &t2, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 3, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    t2.n_rows = -1;
    EXPECT(ltg_topk_explain(img, 0, 4, &t2, 0, -1, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    // k_in, top, r
    const int32_t bad_k[] = {0, -1, 1025, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_k / sizeof bad_k[0]; ++i)
        EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 2, bad_k[i], ids, 1, 3, f, out, NULL) == LTG_EINVAL);
    const int32_t bad_top[] = {0, -1, 9, LTG_WHY_MAX_TOP + 1, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_top / sizeof bad_top[0]; ++i)
        EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 2, 8, ids, bad_top[i], 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 2, 1024, ids, LTG_WHY_MAX_TOP + 1, 3, f, out, NULL) == LTG_EINVAL);
    const int32_t bad_r[] = {0, -1, LTG_WHY_MAX_R + 1, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_r / sizeof bad_r[0]; ++i)
        EXPECT(ltg_topk_explain(img, 0, 4, &tr, 0, 2, 8, ids, 4, bad_r[i], f, out, NULL) == LTG_EINVAL);
    // the image
    EXPECT(ltg_topk_explain(img, 0, 0, &tr, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, -4, &tr, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, -1, 4, &tr, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, &tr, -1, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img + 1, 0, 3, &tr, 0, 2, 8, ids, 4, 3, f, out, NULL) == LTG_EINVAL);     // not 16-byte aligned
    // zero rows: nothing is launched, but the arguments are still checked
    EXPECT(ltg_topk_explain(img, 0, 4, &none, 0, 0, 8, ids, 4, 3, f, out, NULL) == LTG_OK);
    EXPECT(ltg_topk_explain(img, INT32_MAX, INT32_MAX, &none, INT32_MAX, 0, 1024, ids, 256, 8, f, out, NULL) == LTG_OK);
    EXPECT(ltg_topk_explain(img, 0, 4, &none, 0, 0, 8, ids, 9, 3, f, out, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_explain(img, 0, 4, &none, 0, 0, 8, ids, 4, 9, f, out, NULL) == LTG_EINVAL);
    free(ptr);
    free(out);
    free(ids);
    free(f);
    free(img);
    if (failures) {
        fprintf(stderr, "explain host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("explain host check: ok\n");
    return 0;
}
