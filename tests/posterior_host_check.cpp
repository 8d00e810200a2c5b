// Stand-alone check of the host side of ltg_posterior_ld / _image_bytes / _h2 / _scores / _entries and ltg_row_lse under a sanitizer:
// argument validation only, i.e. the paths that return before any HIP call (no GPU is needed, no kernel is launched).  Not part of the
// pytest suite (it recompiles the library's translation unit); build and run by hand from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -o /tmp/posterior_host_check tests/posterior_host_check.cpp long-tail-gan_amd/csrc/ltg_kernels.hip && /tmp/posterior_host_check
//
// Prints "posterior host check: ok" and exits 0; any sanitizer report or failed expectation makes the exit status non-zero.
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

static ltg_config good_cfg(void) {
    ltg_config c;
    memset(&c, 0, sizeof c);
    c.n_items = 1000;
    c.h_enc = 600;
    c.z_dim = 200;
    c.d_feat = 1000;
    c.d_h0 = 100, c.d_h1 = 150, c.d_h2 = 250, c.d_h3 = 300;
    c.precision = LTG_PREC_BF16;
    c.d_precision = LTG_PREC_FP32;
    return c;
}

int main(void) {
    // heap blocks: the host reads the configuration and the generator struct and only compares the other pointers with NULL (the image
    // pointer also for its alignment)
    ltg_config cfg = good_cfg();
    float* f = (float*)malloc(16);
    int32_t* ids = (int32_t*)malloc(16);
    uint16_t* img = (uint16_t*)aligned_alloc(16, 32);
    ltg_gen_state gen;
    memset(&gen, 0, sizeof gen);
    gen.p[2] = gen.p[3] = gen.p[6] = gen.p[7] = f;

    EXPECT(ltg_posterior_ld(&cfg) == 608);
    EXPECT(ltg_posterior_ld(NULL) == 0);
    EXPECT(ltg_posterior_image_bytes(&cfg, 37, 16) == (size_t)37 * 16 * 608 * 2);
    EXPECT(ltg_posterior_image_bytes(&cfg, 37, 3) == 0 && ltg_posterior_image_bytes(&cfg, -1, 4) == 0 && ltg_posterior_image_bytes(NULL, 1, 4) == 0);
    EXPECT(ltg_posterior_image_bytes(&cfg, INT32_MAX, 32) == 0);

    const int32_t good_s[] = {1, 4, 8, 16, 32};
    for (size_t i = 0; i < sizeof good_s / sizeof good_s[0]; ++i) {      // zero rows: checked, nothing launched
        const int32_t s = good_s[i];
        EXPECT(ltg_posterior_h2(&cfg, &gen, f, 0, 0, s, 7, NULL, img, NULL, NULL) == LTG_OK);
        EXPECT(ltg_posterior_scores(&cfg, &gen, img, 0, s, 0.f, f, NULL, NULL) == LTG_OK);
        EXPECT(ltg_posterior_entries(&cfg, &gen, img, 0, s, ids, 4, f, f, NULL) == LTG_OK);
    }
    EXPECT(ltg_row_lse(&cfg, f, 0, f, NULL) == LTG_OK);
    const int32_t bad_s[] = {0, -1, 2, 3, 5, 12, 33, 64, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_s / sizeof bad_s[0]; ++i) {
        for (int32_t n = 0; n <= 2; n += 2) {
            EXPECT(ltg_posterior_h2(&cfg, &gen, f, n, 0, bad_s[i], 0, NULL, img, NULL, NULL) == LTG_EINVAL);
            EXPECT(ltg_posterior_scores(&cfg, &gen, img, n, bad_s[i], 0.f, f, NULL, NULL) == LTG_EINVAL);
            EXPECT(ltg_posterior_entries(&cfg, &gen, img, n, bad_s[i], ids, 4, f, f, NULL) == LTG_EINVAL);
        }
    }
    const float bad_beta[] = {INFINITY, -INFINITY, NAN};
    for (size_t i = 0; i < sizeof bad_beta / sizeof bad_beta[0]; ++i) {
        EXPECT(ltg_posterior_scores(&cfg, &gen, img, 2, 16, bad_beta[i], f, NULL, NULL) == LTG_EINVAL);
        EXPECT(ltg_posterior_scores(&cfg, &gen, img, 0, 16, bad_beta[i], f, NULL, NULL) == LTG_EINVAL);
    }
    EXPECT(ltg_posterior_scores(&cfg, &gen, img, 2, 1, 0.5f, f, NULL, NULL) == LTG_EINVAL);      // one sample has no std
    EXPECT(ltg_posterior_scores(&cfg, &gen, img, 0, 1, -1.f, f, NULL, NULL) == LTG_EINVAL);
    // NULL required pointers
    EXPECT(ltg_posterior_h2(NULL, &gen, f, 2, 0, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_h2(&cfg, NULL, f, 2, 0, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_h2(&cfg, &gen, NULL, 2, 0, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_h2(&cfg, &gen, f, 2, 0, 4, 0, NULL, NULL, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_h2(&cfg, &gen, f, 2, -1, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_h2(&cfg, &gen, f, 0, -1, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_h2(&cfg, &gen, f, -1, 0, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_scores(NULL, &gen, img, 2, 4, 0.f, f, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_scores(&cfg, NULL, img, 2, 4, 0.f, f, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_scores(&cfg, &gen, NULL, 2, 4, 0.f, f, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_scores(&cfg, &gen, img, 2, 4, 0.f, NULL, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_scores(&cfg, &gen, img + 1, 2, 4, 0.f, f, NULL, NULL) == LTG_EINVAL);   // not 16-byte aligned
    EXPECT(ltg_posterior_scores(&cfg, &gen, img, -1, 4, 0.f, f, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_entries(&cfg, &gen, img, 2, 4, NULL, 4, f, f, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_entries(&cfg, &gen, img, 2, 4, ids, 4, NULL, f, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_entries(&cfg, &gen, img, 2, 4, ids, 4, f, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_entries(&cfg, &gen, NULL, 2, 4, ids, 4, f, f, NULL) == LTG_EINVAL);
    const int32_t bad_k[] = {0, -1, 1025, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_k / sizeof bad_k[0]; ++i) {
        EXPECT(ltg_posterior_entries(&cfg, &gen, img, 2, 4, ids, bad_k[i], f, f, NULL) == LTG_EINVAL);
        EXPECT(ltg_posterior_entries(&cfg, &gen, img, 0, 4, ids, bad_k[i], f, f, NULL) == LTG_EINVAL);
    }
    EXPECT(ltg_row_lse(NULL, f, 2, f, NULL) == LTG_EINVAL);
    EXPECT(ltg_row_lse(&cfg, NULL, 2, f, NULL) == LTG_EINVAL);
    EXPECT(ltg_row_lse(&cfg, f, 2, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_row_lse(&cfg, f, -1, f, NULL) == LTG_EINVAL);
    // a generator without the tables a call reads
    ltg_gen_state empty;
    memset(&empty, 0, sizeof empty);
    EXPECT(ltg_posterior_h2(&cfg, &empty, f, 2, 0, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_scores(&cfg, &empty, img, 2, 4, 0.f, f, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_entries(&cfg, &empty, img, 2, 4, ids, 4, f, f, NULL) == LTG_EINVAL);
    // bad configurations
    ltg_config bad = good_cfg();
    bad.n_items = 0;
    EXPECT(ltg_posterior_scores(&bad, &gen, img, 2, 4, 0.f, f, NULL, NULL) == LTG_EINVAL && ltg_row_lse(&bad, f, 2, f, NULL) == LTG_EINVAL);
    bad = good_cfg();
    bad.h_enc = 602;
    EXPECT(ltg_posterior_h2(&bad, &gen, f, 2, 0, 4, 0, NULL, img, NULL, NULL) == LTG_EINVAL && ltg_posterior_ld(&bad) == 0);
    bad = good_cfg();
    bad.item_lo = -1;
    EXPECT(ltg_posterior_scores(&bad, &gen, img, 2, 4, 0.f, f, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_entries(&bad, &gen, img, 2, 4, ids, 4, f, f, NULL) == LTG_EINVAL);
    bad = good_cfg();
    bad.z_dim = 4096;                                                   // 8 x 4096 floats of z do not fit the LDS
    EXPECT(ltg_posterior_h2(&bad, &gen, f, 2, 0, 8, 0, NULL, img, NULL, NULL) == LTG_EINVAL);
    EXPECT(ltg_posterior_h2(&bad, &gen, f, 0, 0, 4, 0, NULL, img, NULL, NULL) == LTG_OK);
    free(img);
    free(ids);
    free(f);
    if (failures) {
        fprintf(stderr, "posterior host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("posterior host check: ok\n");
    return 0;
}
