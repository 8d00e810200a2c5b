// Stand-alone check of the host side of ltg_floor_ws_bytes, ltg_floor_index, ltg_floor_rounds and ltg_floor_finish under a sanitizer:
// argument validation and the size arithmetic of the workspace, i.e. only the paths that return before any HIP call (no GPU is needed, no
// kernel is launched).  Not part of the pytest suite (it recompiles the library's translation unit); build and run by hand from the
// repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -o /tmp/floor_host_check tests/floor_host_check.cpp long-tail-gan_amd/csrc/ltg_kernels.hip && /tmp/floor_host_check
//
// Prints "floor host check: ok" and exits 0; any sanitizer report or failed expectation makes the exit status non-zero.
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
    // heap blocks of exactly the sizes a 2 x 8 matching over 16 items reads on the host (nothing: the pointers are only compared with NULL)
    float* cs = (float*)malloc(2 * 8 * sizeof(float));
    int32_t* ci = (int32_t*)malloc(2 * 8 * sizeof(int32_t));
    float* lse = (float*)malloc(2 * sizeof(float));
    int32_t* nd = (int32_t*)malloc(16 * sizeof(int32_t));
    int32_t* state = (int32_t*)malloc(LTG_FLOOR_STATE * sizeof(int32_t));
    float* so = (float*)malloc(2 * 4 * sizeof(float));
    int32_t* io = (int32_t*)malloc(2 * 4 * sizeof(int32_t));
    uint8_t* ao = (uint8_t*)malloc(2 * 8);
    int32_t* ho = (int32_t*)malloc(16 * sizeof(int32_t));
    void* ws = malloc(16);
    const size_t need = ltg_floor_ws_bytes(2, 8, 16), need0 = ltg_floor_ws_bytes(0, 8, 16);

    // ---- ltg_floor_ws_bytes: grows with every size, 0 for what the calls refuse, no overflow at the largest sizes it takes
    EXPECT(need >= 16 * 8 + 17 * 4 + 16 * 4 + 16 * 4 + 2 * 4 + 2 * 4 + 16 * 4 && need0 > 0 && need0 <= need);
    EXPECT(ltg_floor_ws_bytes(3, 8, 16) >= need && ltg_floor_ws_bytes(2, 9, 16) >= need && ltg_floor_ws_bytes(2, 8, 17000) > need);
    EXPECT(ltg_floor_ws_bytes((1 << 21) - 1, 1024, INT32_MAX) > (size_t)INT32_MAX * 20 + (size_t)((1 << 21) - 1) * 1024 * 4);
    EXPECT(ltg_floor_ws_bytes(INT32_MAX, 1, 1) > (size_t)INT32_MAX * 12);
    const int32_t bad_ws[][3] = {{-1, 8, 16}, {INT32_MIN, 8, 16}, {2, 0, 16}, {2, -1, 16}, {2, 1025, 16}, {2, INT32_MAX, 16}, {2, 8, 0},
                                 {2, 8, -1}, {2, 8, INT32_MIN}, {1 << 21, 1024, 16}, {1 << 30, 2, 16}, {INT32_MAX, 2, 16}, {INT32_MAX, 1024, 16}};
    for (size_t i = 0; i < sizeof bad_ws / sizeof bad_ws[0]; ++i) EXPECT(ltg_floor_ws_bytes(bad_ws[i][0], bad_ws[i][1], bad_ws[i][2]) == 0);

    // ---- the sizes all three entry points refuse, with rows and without
    for (size_t i = 0; i < sizeof bad_ws / sizeof bad_ws[0]; ++i) {
        const int32_t n = bad_ws[i][0], c = bad_ws[i][1], I = bad_ws[i][2];
        EXPECT(ltg_floor_index(n, c, ci, I, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_rounds(n, c, cs, ci, lse, nd, I, 1, 1, 1, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_finish(n, c, cs, ci, lse, nd, I, 1, 1, so, io, ao, ho, state, ws, SIZE_MAX, NULL) == LTG_EINVAL);
        if (n > 0) {
            EXPECT(ltg_floor_index(0, c, ci, I, state, ws, SIZE_MAX, NULL) == (ltg_floor_ws_bytes(0, c, I) ? LTG_OK : LTG_EINVAL));
        }
    }
    // ---- ltg_floor_index
    EXPECT(ltg_floor_index(0, 8, ci, 16, state, ws, need0, NULL) == LTG_OK);
    EXPECT(ltg_floor_index(0, 1024, ci, INT32_MAX, state, ws, SIZE_MAX, NULL) == LTG_OK);
    EXPECT(ltg_floor_index(2, 8, NULL, 16, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_index(2, 8, ci, 16, NULL, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_index(2, 8, ci, 16, state, NULL, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_index(2, 8, ci, 16, state, ws, need - 1, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_index(2, 8, ci, 16, state, ws, 0, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_index(0, 8, NULL, 16, state, ws, need0, NULL) == LTG_EINVAL);     // zero rows: the arguments are still checked
    EXPECT(ltg_floor_index(0, 8, ci, 16, state, ws, need0 - 1, NULL) == LTG_EINVAL);
    // ---- ltg_floor_rounds
    EXPECT(ltg_floor_rounds(0, 8, cs, ci, lse, nd, 16, 4, 2, 1, state, ws, need0, NULL) == LTG_OK);
    EXPECT(ltg_floor_rounds(0, 8, cs, ci, NULL, nd, 16, 8, 8, LTG_FLOOR_MAX_ROUNDS, state, ws, need0, NULL) == LTG_OK);    // lse is optional
    EXPECT(ltg_floor_rounds(2, 8, NULL, ci, lse, nd, 16, 4, 2, 1, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_rounds(2, 8, cs, NULL, lse, nd, 16, 4, 2, 1, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_rounds(2, 8, cs, ci, lse, NULL, 16, 4, 2, 1, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_rounds(2, 8, cs, ci, lse, nd, 16, 4, 2, 1, NULL, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_rounds(2, 8, cs, ci, lse, nd, 16, 4, 2, 1, state, NULL, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_rounds(2, 8, cs, ci, lse, nd, 16, 4, 2, 1, state, ws, need - 1, NULL) == LTG_EINVAL);
    const int32_t bad_k[] = {0, -1, 9, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_k / sizeof bad_k[0]; ++i) {
        EXPECT(ltg_floor_rounds(2, 8, cs, ci, lse, nd, 16, bad_k[i], 0, 1, state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_rounds(0, 8, cs, ci, lse, nd, 16, bad_k[i], 0, 1, state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, nd, 16, bad_k[i], 0, so, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_finish(0, 8, cs, ci, lse, nd, 16, bad_k[i], 0, so, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
    }
    const int32_t bad_res[] = {-1, 5, INT32_MAX, INT32_MIN};      // the reserve lies in [0, k], k = 4
    for (size_t i = 0; i < sizeof bad_res / sizeof bad_res[0]; ++i) {
        EXPECT(ltg_floor_rounds(2, 8, cs, ci, lse, nd, 16, 4, bad_res[i], 1, state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_rounds(0, 8, cs, ci, lse, nd, 16, 4, bad_res[i], 1, state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, nd, 16, 4, bad_res[i], so, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_finish(0, 8, cs, ci, lse, nd, 16, 4, bad_res[i], so, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
    }
    EXPECT(ltg_floor_rounds(0, 8, cs, ci, lse, nd, 16, 4, 0, 1, state, ws, need0, NULL) == LTG_OK);
    EXPECT(ltg_floor_rounds(0, 8, cs, ci, lse, nd, 16, 4, 4, 1, state, ws, need0, NULL) == LTG_OK);
    const int32_t bad_r[] = {0, -1, LTG_FLOOR_MAX_ROUNDS + 1, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_r / sizeof bad_r[0]; ++i) {
        EXPECT(ltg_floor_rounds(2, 8, cs, ci, lse, nd, 16, 4, 2, bad_r[i], state, ws, need, NULL) == LTG_EINVAL);
        EXPECT(ltg_floor_rounds(0, 8, cs, ci, lse, nd, 16, 4, 2, bad_r[i], state, ws, need, NULL) == LTG_EINVAL);
    }
    // ---- ltg_floor_finish
    EXPECT(ltg_floor_finish(0, 8, cs, ci, lse, nd, 16, 4, 2, so, io, ao, ho, state, ws, need0, NULL) == LTG_OK);
    EXPECT(ltg_floor_finish(0, 8, cs, ci, NULL, nd, 16, 4, 2, so, io, NULL, NULL, state, ws, need0, NULL) == LTG_OK);       // lse and the tables are optional
    EXPECT(ltg_floor_finish(0, 1024, cs, ci, lse, nd, 16, 1024, 1024, so, io, ao, ho, state, ws, SIZE_MAX, NULL) == LTG_OK);
    EXPECT(ltg_floor_finish(2, 8, NULL, ci, lse, nd, 16, 4, 2, so, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(2, 8, cs, NULL, lse, nd, 16, 4, 2, so, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, NULL, 16, 4, 2, so, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, nd, 16, 4, 2, NULL, io, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, nd, 16, 4, 2, so, NULL, ao, ho, state, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, nd, 16, 4, 2, so, io, ao, ho, NULL, ws, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, nd, 16, 4, 2, so, io, ao, ho, state, NULL, need, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(2, 8, cs, ci, lse, nd, 16, 4, 2, so, io, ao, ho, state, ws, need - 1, NULL) == LTG_EINVAL);
    EXPECT(ltg_floor_finish(0, 8, cs, ci, lse, nd, 16, 4, 2, so, NULL, ao, ho, state, ws, need0, NULL) == LTG_EINVAL);
    free(ws);
    free(ho);
    free(ao);
    free(io);
    free(so);
    free(state);
    free(nd);
    free(lse);
    free(ci);
    free(cs);
    if (failures) {
        fprintf(stderr, "floor host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("floor host check: ok\n");
    return 0;
}
