// Stand-alone check of the host side of ltg_list_mass and ltg_replay_rows under a sanitizer: argument validation and the read of the HOST
// array of temperatures (exactly n_pol floats, never one more), i.e. only the paths that return before any HIP call (no GPU is needed, no
// kernel is launched).  Not part of the pytest suite (it recompiles the library's translation unit); build and run by hand from the
// repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -o /tmp/replay_host_check tests/replay_host_check.cpp long-tail-gan_amd/csrc/ltg_kernels.hip && /tmp/replay_host_check
//
// Prints "replay host check: ok" and exits 0; any sanitizer report or failed expectation makes the exit status non-zero.
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

int main(void) {
    // heap blocks: the host reads the temperatures and the configuration and only compares the other pointers with NULL
    ltg_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_items = 1000;
    float* logits = (float*)malloc(16);
    int32_t* ids = (int32_t*)malloc(16);
    int32_t* head = (int32_t*)malloc(16);
    float* f = (float*)malloc(16);
    int32_t* st = (int32_t*)malloc(16);
    double* d = (double*)malloc(16);
    uint8_t* lab = (uint8_t*)malloc(16);

    for (int n_pol = 1; n_pol <= LTG_REPLAY_MAX_POLICIES; ++n_pol) {
        float* it = (float*)malloc(n_pol * sizeof(float));        // exactly n_pol values: a read of it[n_pol] is a report
        for (int p = 0; p < n_pol; ++p) it[p] = 0.5f + (float)p;
        EXPECT(ltg_list_mass(&cfg, logits, NULL, 0, 4, ids, 0, NULL, n_pol, it, f, st, f, f, NULL) == LTG_OK);
        EXPECT(ltg_replay_rows(0, 4, n_pol, it, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_OK);
        const float bad[] = {0.f, -1.f, INFINITY, -INFINITY, NAN};
        for (size_t b = 0; b < sizeof bad / sizeof bad[0]; ++b) {
            it[n_pol - 1] = bad[b];                                // the last value that is read
            EXPECT(ltg_list_mass(&cfg, logits, NULL, 0, 4, ids, 0, NULL, n_pol, it, f, st, f, f, NULL) == LTG_EINVAL);
            EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, 4, ids, 0, NULL, n_pol, it, f, st, f, f, NULL) == LTG_EINVAL);
            EXPECT(ltg_replay_rows(2, 4, n_pol, it, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
            if (n_pol > 1) {                                       // one value fewer: the bad one is not read
                EXPECT(ltg_list_mass(&cfg, logits, NULL, 0, 4, ids, 0, NULL, n_pol - 1, it, f, st, f, f, NULL) == LTG_OK);
                EXPECT(ltg_replay_rows(0, 4, n_pol - 1, it, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_OK);
            }
        }
        free(it);
    }
    float one[1] = {1.f};
    const int32_t bad_pol[] = {0, -1, 9, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_pol / sizeof bad_pol[0]; ++i) {   // n_pol is refused before the array is read
        EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, 4, ids, 0, NULL, bad_pol[i], one, f, st, f, f, NULL) == LTG_EINVAL);
        EXPECT(ltg_replay_rows(2, 4, bad_pol[i], one, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    }
    EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, 4, ids, 0, NULL, 1, NULL, f, st, f, f, NULL) == LTG_EINVAL);
    EXPECT(ltg_replay_rows(2, 4, 1, NULL, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    const int32_t bad_k[] = {0, -1, 1025, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_k / sizeof bad_k[0]; ++i) {
        EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, bad_k[i], ids, 0, NULL, 1, one, f, st, f, f, NULL) == LTG_EINVAL);
        EXPECT(ltg_replay_rows(2, bad_k[i], 1, one, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    }
    const int32_t bad_f[] = {-1, 4, 5, INT32_MAX, INT32_MIN};           // 0 <= f_in < k = 4
    for (size_t i = 0; i < sizeof bad_f / sizeof bad_f[0]; ++i) {
        EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, 4, ids, bad_f[i], head, 1, one, f, st, f, f, NULL) == LTG_EINVAL);
        EXPECT(ltg_replay_rows(2, 4, 1, one, bad_f[i], head, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    }
    EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, 4, ids, 3, NULL, 1, one, f, st, f, f, NULL) == LTG_EINVAL);       // a head without its ids
    EXPECT(ltg_replay_rows(2, 4, 1, one, 3, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_list_mass(&cfg, logits, NULL, 0, 4, ids, 3, head, 1, one, f, st, f, f, NULL) == LTG_OK);
    EXPECT(ltg_replay_rows(0, 4, 1, one, 3, head, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, f, NULL) == LTG_OK);
    const double bad_clip[] = {0.0, -1.0, (double)INFINITY, (double)NAN};
    for (size_t i = 0; i < sizeof bad_clip / sizeof bad_clip[0]; ++i)
        EXPECT(ltg_replay_rows(2, 4, 1, one, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, bad_clip[i], d, d, st, NULL, NULL) == LTG_EINVAL);
    const int32_t bad_g[] = {0, -1, 9, INT32_MAX};
    for (size_t i = 0; i < sizeof bad_g / sizeof bad_g[0]; ++i)
        EXPECT(ltg_replay_rows(2, 4, 1, one, 0, NULL, ids, f, f, f, st, f, f, lab, bad_g[i], 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_replay_rows(2, 4, 1, one, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 0, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_replay_rows(-1, 4, 1, one, 0, NULL, ids, f, f, f, st, f, f, lab, 2, 50, 100.0, d, d, st, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_list_mass(&cfg, logits, NULL, -1, 4, ids, 0, NULL, 1, one, f, st, f, f, NULL) == LTG_EINVAL);
    EXPECT(ltg_list_mass(NULL, logits, NULL, 2, 4, ids, 0, NULL, 1, one, f, st, f, f, NULL) == LTG_EINVAL);
    cfg.n_items = 425985;                                               // a slab beyond the LDS bitset
    EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, 4, ids, 0, NULL, 1, one, f, st, f, f, NULL) == LTG_EINVAL);
    cfg.n_items = 0;
    EXPECT(ltg_list_mass(&cfg, logits, NULL, 2, 4, ids, 0, NULL, 1, one, f, st, f, f, NULL) == LTG_EINVAL);
    free(lab);
    free(d);
    free(st);
    free(f);
    free(head);
    free(ids);
    free(logits);
    if (failures) {
        fprintf(stderr, "replay host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("replay host check: ok\n");
    return 0;
}
