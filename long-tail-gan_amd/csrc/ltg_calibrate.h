// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_explain.h): calibrated top-K lists
// (ltg_hist_groups, ltg_topk_calibrate).  Every user's list follows the class mix of that user's fold-in history: greedily, the
// next entry is the head of a class list with the largest  (1 - lambda) * rel(score) - lambda * tv(list so far + that class),  tv = the
// total-variation distance between the history's class shares and the list's.  Integers, one fp64 division and fp32 products: no
// transcendental, no MFMA, so the kernels are held to numpy bit for bit.
//
// k_hist_groups: one wave per row, the lanes stride the row's history, nine per-lane counters, one wave reduction per class.
// k_topk_calibrate: a row is 16 lanes, lane c = class c (C <= 9), four rows per wave, one wave per workgroup.  A class's cursor, head, history
//   count and list count live in its lane; everything a round needs from the other classes comes through DPP exchanges inside a row of
//   16 lanes.  (One row per wave would leave 55 of 64 lanes idle through 2 k rounds of ~100 instructions.)
//   1. the plain merge: min(k, n) rounds of a 64-bit argmax over the heads' (key, ~id) words -> s_hi, s_lo, the plain list's class counts.
//   2. the greedy rounds: x_c = h_c m - n_c H per lane, D0 = the row's sum of |x_c|, D_c = D0 - |x_c| + |x_c - H| for a candidate, tv_c, the
//      objective, a 32-bit argmax of its key, then the 64-bit argmax of the heads' words among the lanes that hold it (the tie rule).
//   3. the winner writes its head in pick order with the original score and takes its list's next entry.
// STAGE: the wave first copies its rows' lists into LDS with coalesced loads ([list][row of the wave][m_in] mirrors global memory, where the
// rows of a wave are adjacent), and the heads are read from there; otherwise the heads come from global memory.  No global workspace, no
// atomics, ids never index anything, the loops' trip counts are wave-uniform and every exchange is executed by all 64 lanes.
#pragma once

constexpr int CAL_C = 9;             // == LTG_CAL_MAX_CLASSES
constexpr int CAL_ROWS = 4;          // rows per wave: 16 lanes each

struct cal_map { int32_t list_of[CAL_C]; };      // class -> its list, or -1

__global__ __launch_bounds__(NT) void k_hist_groups(int n_rows, const int32_t* __restrict__ h_ptr, const int32_t* __restrict__ h_idx, int hist_lo,
                                                    const uint8_t* __restrict__ labels, int n_items_global, int n_groups,
                                                    int32_t* __restrict__ count_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                       // (whole waves: nothing below meets another wave)
    int cnt[CAL_C];
#pragma unroll
    for (int c = 0; c < CAL_C; ++c) cnt[c] = 0;
    const int e1 = h_ptr[row + 1];
    for (int e = h_ptr[row] + lane; e < e1; e += 64) {
        const int64_t g = (int64_t)hist_lo + (int64_t)h_idx[e];
        if (g < 0 || g >= (int64_t)n_items_global) continue;
        const int cls = min((int)labels[g], n_groups);
#pragma unroll
        for (int c = 0; c < CAL_C; ++c) cnt[c] += cls == c ? 1 : 0;
    }
    int mine = 0;
#pragma unroll
    for (int c = 0; c < CAL_C; ++c) {
        int v = cnt[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        mine = lane == c ? v : mine;
    }
    if (lane <= n_groups) count_out[(size_t)row * (n_groups + 1) + lane] = mine;
}

// the maximum / the sum over the 16 lanes of a row, in every one of them: four DPP exchanges (lane ^ 1, lane ^ 2, then the other quad of the
// half row and the other half of the row by the two mirrors -- after two steps a quad's lanes agree, so a mirror is as good as an xor),
// ltg_diversify.h's dv_wave_umax without its last step across the rows.  A DPP operand costs a few cycles where a shuffle through the LDS
// crossbar costs about a hundred, and a round is a chain of a dozen of them.
template <int CTRL>
__device__ __forceinline__ uint32_t cal_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ uint64_t cal_dpp64(uint64_t v) {
    return ((uint64_t)cal_dpp<CTRL>((uint32_t)(v >> 32)) << 32) | (uint64_t)cal_dpp<CTRL>((uint32_t)v);
}
__device__ __forceinline__ uint32_t cal_row_umax(uint32_t v) {
    v = max(v, cal_dpp<0xB1>(v));                    // quad_perm [1, 0, 3, 2]
    v = max(v, cal_dpp<0x4E>(v));                    // quad_perm [2, 3, 0, 1]
    v = max(v, cal_dpp<0x141>(v));                   // row_half_mirror
    return max(v, cal_dpp<0x140>(v));                // row_mirror
}
__device__ __forceinline__ uint64_t cal_row_umax64(uint64_t v) {
    v = max(v, cal_dpp64<0xB1>(v));
    v = max(v, cal_dpp64<0x4E>(v));
    v = max(v, cal_dpp64<0x141>(v));
    return max(v, cal_dpp64<0x140>(v));
}
__device__ __forceinline__ int64_t cal_row_sum64(int64_t x) {
    uint64_t v = (uint64_t)x;                        // (two's complement: the unsigned sum is the signed one)
    v += cal_dpp64<0xB1>(v);
    v += cal_dpp64<0x4E>(v);
    v += cal_dpp64<0x141>(v);
    return (int64_t)(v + cal_dpp64<0x140>(v));
}
// fp32 product, difference and quotient that stay what they are: the translation unit is built with contraction on, and x * y - z written
// in the open (or through __fmul_rn / __fsub_rn, which are plain operators) becomes one fused multiply-add with a single rounding
__device__ __forceinline__ float cal_mul(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ float cal_sub(float x, float y) {
#pragma clang fp contract(off)
    return x - y;
}
__device__ __forceinline__ float cal_div(float x, float y) {
#pragma clang fp contract(off)
    return x / y;
}
__device__ __forceinline__ int64_t cal_abs64(int64_t v) { return v < 0 ? -v : v; }
// the miscalibration of a list of m entries from D = sum_c |h_c m - n_c H|
__device__ __forceinline__ float cal_tv(int64_t D, int64_t H, int m) {
    return H > 0 ? (float)((double)D / (double)(2 * H * (int64_t)m)) : 0.f;
}

template <bool STAGE>
__global__ __launch_bounds__(64) void k_topk_calibrate(int n_rows, int n_lists, int m_in, const float* __restrict__ score_grp,
                                                       const int32_t* __restrict__ id_grp, cal_map map, int n_groups,
                                                       const int32_t* __restrict__ hist, float lambda, int k, float* __restrict__ score_out,
                                                       int32_t* __restrict__ id_out, float* __restrict__ stat_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned cal_lds[];     // STAGE: scores [n_lists][CAL_ROWS][m_in] | ids the same
    const int lane = threadIdx.x, r = lane >> 4, c = lane & 15, C = n_groups + 1;
    const int row0 = blockIdx.x * CAL_ROWS, row = row0 + r;
    const bool live = row < n_rows;
    int j = -1;                                      // the list of this lane's class
#pragma unroll
    for (int q = 0; q < CAL_C; ++q) j = q == c ? map.list_of[q] : j;
    const bool listed = live && c < C && j >= 0;
    const float* ls;
    const int32_t* li;
    if (STAGE) {
        float* st_s = reinterpret_cast<float*>(cal_lds);
        int32_t* st_i = reinterpret_cast<int32_t*>(cal_lds) + n_lists * CAL_ROWS * m_in;
        const int n_here = min(CAL_ROWS, n_rows - row0) * m_in;          // the wave's rows of one list are adjacent in global memory
        for (int q = 0; q < n_lists; ++q) {
            const size_t src = ((size_t)q * n_rows + row0) * m_in;
            for (int e = lane; e < n_here; e += 64) {
                st_s[q * CAL_ROWS * m_in + e] = score_grp[src + e];
                st_i[q * CAL_ROWS * m_in + e] = id_grp[src + e];
            }
        }
        __syncthreads();
        ls = st_s + (listed ? (j * CAL_ROWS + r) * m_in : 0);
        li = st_i + (listed ? (j * CAL_ROWS + r) * m_in : 0);
    } else {
        const size_t off = listed ? ((size_t)j * n_rows + row) * m_in : 0;
        ls = score_grp + off;
        li = id_grp + off;
    }
    const int64_t h = live && c < C ? (int64_t)hist[(size_t)row * C + c] : 0;
    const int64_t H = cal_row_sum64(h);
    float* so = score_out + (size_t)(live ? row : 0) * k;
    int32_t* io = id_out + (size_t)(live ? row : 0) * k;

    // 1. the plain merge
    int p = 0, hid = -1;
    float hs = -INFINITY;
    if (listed) {
        hid = li[0];
        hs = ls[0];
    }
    bool has = listed && hid >= 0;
    uint64_t word = has ? tk_comp(tk_key(hs), hid) : 0ull;
    const int id0 = hid;                             // the list's first entry: the greedy rounds start from it again
    const float s0 = hs;
    float s_hi = 0.f, s_lo = 0.f;
    int kk = 0, pc = 0;                              // the row's plain list length; this class's entries in it
    for (int t = 0; t < k; ++t) {
        if (__ballot(has) == 0ull) break;
        const uint64_t best = cal_row_umax64(word);
        if (best != 0ull) {                          // (a row without a candidate left sits the round out)
            const uint32_t key = (uint32_t)(best >> 32);
            s_lo = __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
            s_hi = t == 0 ? s_lo : s_hi;
            ++kk;
            if (has && word == best) {
                ++pc;
                ++p;
                has = false;
                if (p < m_in) {
                    hid = li[p];
                    hs = ls[p];
                    has = hid >= 0;
                }
                word = has ? tk_comp(tk_key(hs), hid) : 0ull;
            }
        }
    }
    const float tv_plain = cal_tv(cal_row_sum64(cal_abs64(h * kk - (int64_t)pc * H)), H, max(kk, 1));

    // 2. the greedy rounds
    const float a = cal_sub(1.f, lambda);
    const bool flat = s_hi == s_lo;
    const float span = cal_sub(s_hi, s_lo);
    p = 0;
    hid = id0;
    hs = s0;
    has = listed && hid >= 0;
    word = has ? tk_comp(tk_key(hs), hid) : 0ull;
    float lrel = has ? cal_mul(a, flat ? 0.f : cal_div(cal_sub(hs, s_lo), span)) : 0.f;
    int nc = 0;                                      // this class's entries in the list so far
    for (int t = 0; t < k; ++t) {
        const bool cand = has && t < kk;
        if (__ballot(cand) == 0ull) break;
        const int m = t + 1;
        const int64_t x = h * m - (int64_t)nc * H, ax = cal_abs64(x);
        const int64_t D0 = cal_row_sum64(ax);
        const float tv = cal_tv(D0 - ax + cal_abs64(x - H), H, m);
        const float obj = cal_sub(lrel, cal_mul(lambda, tv));
        const uint32_t okey = cand ? tk_key(obj) : 0u;
        const uint32_t omax = cal_row_umax(okey);
        const bool top = cand && okey == omax;
        const uint64_t best = cal_row_umax64(top ? word : 0ull);
        if (top && word == best) {
            io[t] = hid;
            so[t] = hs;
            ++nc;
            ++p;
            has = false;
            if (p < m_in) {
                hid = li[p];
                hs = ls[p];
                has = hid >= 0;
            }
            word = has ? tk_comp(tk_key(hs), hid) : 0ull;
            lrel = has ? cal_mul(a, flat ? 0.f : cal_div(cal_sub(hs, s_lo), span)) : 0.f;
        }
    }
    const float tv_list = cal_tv(cal_row_sum64(cal_abs64(h * kk - (int64_t)nc * H)), H, max(kk, 1));
    if (!live) return;
    for (int t = kk + c; t < k; t += 16) {
        io[t] = -1;
        so[t] = -INFINITY;
    }
    if (stat_out && c < 2) stat_out[(size_t)row * 2 + c] = kk == 0 ? 0.f : (c == 0 ? tv_plain : tv_list);
}
