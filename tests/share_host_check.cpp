// Stand-alone check of the host side of ltg_share_ws_bytes and ltg_topk_share under a sanitizer: argument validation, the overlap test of
// the outputs against the inputs and the size arithmetic of the workspace, i.e. only the paths that return before any HIP call (no GPU is
// needed, no kernel is launched).  Not part of the pytest suite (it recompiles the library's translation unit); build and run by hand
// from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -o /tmp/share_host_check tests/share_host_check.cpp long-tail-gan_amd/csrc/ltg_kernels.hip && /tmp/share_host_check
//
// Prints "share host check: ok" and exits 0; any sanitizer report or failed expectation makes the exit status non-zero.
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
    // heap blocks of exactly the sizes a 2 x 8 -> 2 x 4 call names (the host reads none of them: the pointers are only compared)
    float* ps = (float*)malloc(2 * 8 * sizeof(float));
    int32_t* pi = (int32_t*)malloc(2 * 8 * sizeof(int32_t));
    float* rs = (float*)malloc(2 * 8 * sizeof(float));
    int32_t* ri = (int32_t*)malloc(2 * 8 * sizeof(int32_t));
    float* so = (float*)malloc(2 * 4 * sizeof(float));
    int32_t* io = (int32_t*)malloc(2 * 4 * sizeof(int32_t));
    int32_t* state = (int32_t*)malloc(LTG_SHARE_STATE * sizeof(int32_t));
    void* ws = malloc(16);
    for (int i = 0; i < LTG_SHARE_STATE; ++i) state[i] = -9;
    const size_t need = ltg_share_ws_bytes(2, 4), need0 = ltg_share_ws_bytes(0, 4);

    // ---- ltg_share_ws_bytes: grows with both sizes, 0 for what the call refuses, no overflow at the largest sizes it takes
    EXPECT(need >= 2 * 4 * 8 + 2 * 2 * 4 + 8 * 256 * 4 && need0 > 0 && need0 <= need);
    EXPECT(ltg_share_ws_bytes(3000, 4) > ltg_share_ws_bytes(2000, 4) && ltg_share_ws_bytes(2000, 5) > ltg_share_ws_bytes(2000, 4));
    EXPECT(ltg_share_ws_bytes((1 << 21) - 1, 1024) > (size_t)((1 << 21) - 1) * 1024 * 8);
    EXPECT(ltg_share_ws_bytes(INT32_MAX, 1) > (size_t)INT32_MAX * 16);
    const int32_t bad_ws[][2] = {{-1, 4}, {INT32_MIN, 4}, {2, 0}, {2, -1}, {2, 1025}, {2, INT32_MAX}, {2, INT32_MIN}, {1 << 21, 1024},
                                 {1 << 30, 2}, {INT32_MAX, 2}, {INT32_MAX, 1024}};
    for (size_t i = 0; i < sizeof bad_ws / sizeof bad_ws[0]; ++i) {
        const int32_t n = bad_ws[i][0], k = bad_ws[i][1];
        EXPECT(ltg_share_ws_bytes(n, k) == 0);
        EXPECT(ltg_topk_share(n, 1024, ps, pi, rs, ri, k, 3, so, io, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
    }

    // ---- ltg_topk_share
    EXPECT(ltg_topk_share(0, 8, ps, pi, rs, ri, 4, 3, so, io, state, ws, need0, NULL) == LTG_OK);
    EXPECT(ltg_topk_share(0, 1024, ps, pi, rs, ri, 1024, INT64_MAX, so, io, state, ws, SIZE_MAX, NULL) == LTG_OK);
    EXPECT(ltg_topk_share(0, 8, ps, pi, rs, ri, 8, 0, so, io, state, ws, ltg_share_ws_bytes(0, 8), NULL) == LTG_OK);
    EXPECT(ltg_topk_share(2, 8, NULL, pi, rs, ri, 4, 3, so, io, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, NULL, rs, ri, 4, 3, so, io, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, NULL, ri, 4, 3, so, io, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, NULL, 4, 3, so, io, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, NULL, io, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, NULL, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, io, NULL, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, io, state, NULL, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, io, state, ws, need - 1, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, io, state, ws, 0, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(0, 8, ps, pi, rs, ri, 4, 3, so, NULL, state, ws, need0, NULL) == LTG_EINVAL);    // zero rows: the arguments are still checked
    EXPECT(ltg_topk_share(0, 8, ps, pi, rs, ri, 4, 3, so, io, state, ws, need0 - 1, NULL) == LTG_EINVAL);
    const int32_t bad_m[] = {0, -1, 1025, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_m / sizeof bad_m[0]; ++i) {
        EXPECT(ltg_topk_share(2, bad_m[i], ps, pi, rs, ri, 1, 3, so, io, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
        EXPECT(ltg_topk_share(0, bad_m[i], ps, pi, rs, ri, 1, 3, so, io, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
    }
    const int32_t bad_k[] = {0, -1, 9, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_k / sizeof bad_k[0]; ++i) {
        EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, bad_k[i], 3, so, io, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
        EXPECT(ltg_topk_share(0, 8, ps, pi, rs, ri, bad_k[i], 3, so, io, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
    }
    const int64_t bad_want[] = {-1, INT64_MIN, -((int64_t)1 << 40)};
    for (size_t i = 0; i < sizeof bad_want / sizeof bad_want[0]; ++i) {
        EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, bad_want[i], so, io, state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_topk_share(0, 8, ps, pi, rs, ri, 4, bad_want[i], so, io, state, ws, need, NULL) == LTG_EINVAL);
    }
    // an output that is an input, or reaches into one
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, ps, io, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, rs, io, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, pi, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, ri, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(0, 8, ps, pi, rs, ri, 4, 3, so, ri, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, ps + 12, io, state, ws, need, NULL) == LTG_EINVAL);      // the last 4 of its 8 reach into ps
    EXPECT(ltg_topk_share(2, 8, ps, pi, rs, ri, 4, 3, so, ri + 15, state, ws, need, NULL) == LTG_EINVAL);
    for (int i = 0; i < LTG_SHARE_STATE; ++i) EXPECT(state[i] == -9);       // no path above wrote the state
    free(ws);
    free(state);
    free(io);
    free(so);
    free(ri);
    free(rs);
    free(pi);
    free(ps);
    if (failures) {
        fprintf(stderr, "share host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("share host check: ok\n");
    return 0;
}
