// Stand-alone check of the host side of ltg_item_audience / ltg_item_audience_ws_bytes under a sanitizer: argument validation and
// workspace sizing, i.e. only the paths that return before any HIP call (no GPU is needed, no kernel is launched).  Not part of the
// pytest suite (it recompiles the library's translation unit); build and run by hand from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -o /tmp/audience_host_check tests/audience_host_check.cpp long-tail-gan_amd/csrc/ltg_kernels.hip && /tmp/audience_host_check
//
// Prints "audience host check: ok" and exits 0; any sanitizer report or failed expectation makes the exit status non-zero.
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
    ltg_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_items = 20000;
    // heap buffers of exactly the size a caller would pass: a host-side read or write of them past the end is the sanitizer's to find
    float* f = (float*)malloc(16 * sizeof(float));
    int32_t* q = (int32_t*)malloc(4 * sizeof(int32_t));
    int32_t* ptr = (int32_t*)malloc(5 * sizeof(int32_t));
    memset(f, 0, 16 * sizeof(float));
    memset(q, 0, 4 * sizeof(int32_t));
    memset(ptr, 0, 5 * sizeof(int32_t));
    void* ws = malloc(64);
    const size_t big = (size_t)1 << 40;
    ltg_batch tr;
    memset(&tr, 0, sizeof tr);
    tr.n_rows = 4;
    tr.indptr = ptr;
    tr.indices = ptr;

    // refusals
    EXPECT(ltg_item_audience(NULL, f, f, NULL, 4, 0, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, NULL, f, NULL, 4, 0, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 4, 0, NULL, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 4, 0, q, 3, 8, NULL, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 4, 0, q, 3, 8, f, NULL, ws, big, NULL) == LTG_EINVAL);
    const int32_t bad_k[] = {0, -1, LTG_AUD_MAX_K + 1, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_k / sizeof bad_k[0]; ++i) {
        EXPECT(ltg_item_audience(&cfg, f, f, NULL, 4, 0, q, 3, bad_k[i], f, q, ws, big, NULL) == LTG_EINVAL);
        EXPECT(ltg_item_audience_ws_bytes(&cfg, 20000, 4, bad_k[i]) == 0);
    }
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, -1, 0, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 4, 0, q, -1, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 4, -1, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 2, INT32_MAX - 1, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, INT32_MAX, INT32_MAX, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    ltg_batch t2 = tr;
    t2.n_rows = 5;
    EXPECT(ltg_item_audience(&cfg, f, f, &t2, 4, 0, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    t2 = tr;
    t2.indptr = NULL;
    EXPECT(ltg_item_audience(&cfg, f, f, &t2, 4, 0, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    t2 = tr;
    t2.indices = NULL;
    EXPECT(ltg_item_audience(&cfg, f, f, &t2, 4, 0, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    ltg_config empty = cfg;
    empty.n_items = 0;
    EXPECT(ltg_item_audience(&empty, f, f, NULL, 4, 0, q, 3, 8, f, q, ws, big, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience_ws_bytes(&empty, 20000, 4, 8) == 0 && ltg_item_audience_ws_bytes(NULL, 20000, 4, 8) == 0);
    EXPECT(ltg_item_audience_ws_bytes(&cfg, -1, 4, 8) == 0 && ltg_item_audience_ws_bytes(&cfg, 20000, -1, 8) == 0);

    // the workspace: too small, or absent when one is needed
    const size_t need = ltg_item_audience_ws_bytes(&cfg, 20000, 4, 8);
    EXPECT(need >= (size_t)2 * 4 * 8 * 8);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 20000, 0, q, 4, 8, f, q, ws, need - 1, NULL) == LTG_EINVAL);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 20000, 0, q, 4, 8, f, q, NULL, big, NULL) == LTG_EINVAL);

    // the zero-size calls
    EXPECT(ltg_item_audience(&cfg, f, NULL, NULL, 0, 0, q, 3, 8, f, q, NULL, 0, NULL) == LTG_OK);
    EXPECT(ltg_item_audience(&cfg, f, f, &tr, 4, 0, q, 0, 8, f, q, NULL, 0, NULL) == LTG_OK);
    EXPECT(ltg_item_audience(&cfg, f, f, NULL, 0, INT32_MAX, q, 3, 8, f, q, NULL, 0, NULL) == LTG_OK);

    // the sizing over its whole argument range: lists of at most 32 row segments, no overflow on the way
    const int32_t rows[] = {1, 127, 128, 1024, 1025, 4095, 20000, 1 << 20, INT32_MAX};
    const int32_t nqs[] = {1, 7, 16, 17, 4096, 20000, 1 << 20, INT32_MAX};
    const int32_t ks[] = {1, 100, 128, 129, 256};
    for (size_t a = 0; a < sizeof rows / sizeof rows[0]; ++a)
        for (size_t b = 0; b < sizeof nqs / sizeof nqs[0]; ++b)
            for (size_t c = 0; c < sizeof ks / sizeof ks[0]; ++c) {
                const size_t w = ltg_item_audience_ws_bytes(&cfg, rows[a], nqs[b], ks[c]);
                const size_t per_list = (size_t)nqs[b] * (size_t)ks[c] * 8;
                EXPECT(w <= 32 * per_list + 256);
                EXPECT(w == 0 || w >= 2 * per_list);
                if (rows[a] <= 1024) EXPECT(w == 0);
            }
    free(ws);
    free(ptr);
    free(q);
    free(f);
    if (failures) {
        fprintf(stderr, "audience host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("audience host check: ok\n");
    return 0;
}
