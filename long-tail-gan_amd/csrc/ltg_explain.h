// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_diversify.h): why a user got a
// list entry (ltg_topk_explain).  Per (user row, list entry g) the r history items of that user whose image rows have the
// largest product with g's -- ltg_item_neighbors' score and ltg_topk's list format -- fused per user: the top x history scores never
// leave the chip.
//
// One workgroup (4 waves) per user row, one thread per list entry for the bookkeeping (CT tiles of 16 entries, CT = 4 / 8 / 16).
//   1. the first `top` ids of the row; an id outside the image keeps no image row (its entry is written as r paddings).
//   2. the history is walked in blocks of EX_HB rows.  Per block and K step the list rows' and the block's 64-byte slices are gathered into
//      LDS in fragment order (k_topk_diversify's loader and stage layout) while the next step's loads are in flight; the (history tile,
//      list tile) pairs of the block are dealt round-robin to the waves, every pair one chain of 19 v_mfma_f32_16x16x32_bf16 with the history
//      tile as A and the list tile as B -- the operand roles and the K order of k_item_neighbors, so the accumulator is its score bit for bit.
//   3. the block's scores go to LDS in fp32, [history row][list entry] with a row pitch of 16 CT + 4 floats: the four accumulators of a
//      lane are four rows, and the two 16-lane groups of a half wave then write 16 banks apart (ds_write: 32 banks per half wave), while the
//      fold below reads consecutive floats.
//   4. thread e folds the block's scores of entry e into its sorted running list of (key, ~global id) words (tk_comp): eight words in
//      registers, strict `>`; words are distinct, so the result does not depend on the order of the visits.
//   5. after the last block the first r words of every entry are written as a list.
// No global workspace, no atomics at all, every id -- of the list or of the history -- is checked against [image_lo, image_lo + image_rows)
// before it indexes the image.  The list rows are read again from L2 for every history block (accepted: DESIGN 5.14).
#pragma once

constexpr int EX_HB = 64;            // history rows per block (four 16-row tiles)
constexpr int EX_NT = 256;           // 4 waves
constexpr int EX_R = 8;              // == LTG_WHY_MAX_R: the running list of an entry

template <int CT>
__global__ __launch_bounds__(EX_NT) void k_topk_explain(const unsigned short* __restrict__ image, int image_lo, int image_rows,
                                                        const int32_t* __restrict__ h_ptr, const int32_t* __restrict__ h_idx, int hist_lo,
                                                        int k_in, const int32_t* __restrict__ id_in, int top, int r_out,
                                                        float* __restrict__ score_out, int32_t* __restrict__ id_out) {
    constexpr int HT = EX_HB / 16, NW = EX_NT / 64, PW = CT * HT / NW, NU = CT / 4, LEP = CT * 16 + 4;
    static_assert(EX_NT / 4 == EX_HB && CT * 16 <= EX_NT && CT % 4 == 0, "the loader serves 64 rows per pass; one thread per list entry");
    extern __shared__ __attribute__((aligned(16))) ltg_u32x4 ex_lds[];      // stage [CT + HT][64] x 16 B | scores [EX_HB][LEP] fp32
    __shared__ int s_gid[CT * 16], s_hid[EX_HB];
    ltg_u32x4* stage = ex_lds;
    float* Sc = reinterpret_cast<float*>(ex_lds + (CT + HT) * 64);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
    const size_t row = blockIdx.x;
    const int64_t ilo = image_lo, ihi = (int64_t)image_lo + (int64_t)image_rows;

    // 1. the row's entries; -1 = no image row (outside the image, padding, or past `top`)
    int g = -1;
    if (tid < top) {
        g = id_in[row * k_in + tid];
        if ((int64_t)g < ilo || (int64_t)g >= ihi) g = -1;
    }
    if (tid < CT * 16) s_gid[tid] = g;
    __syncthreads();
    const int LT = (top + 15) >> 4;                 // list tiles in use
    const int q = tid & 3, lrow = tid >> 2;         // loader: four consecutive lanes take the four chunks of one row's K step
    const ltg_u32x4* rp[NU + 1];
    bool rv[NU + 1];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int gg = s_gid[lrow + 64 * u];        // (>= 0: inside the image)
        rv[u] = gg >= 0;
        rp[u] = reinterpret_cast<const ltg_u32x4*>(image) + (size_t)(rv[u] ? gg - image_lo : 0) * ST_C16 + q;
    }
    uint64_t best[EX_R];
#pragma unroll
    for (int j = 0; j < EX_R; ++j) best[j] = 0ull;

    // 2. the history, a block at a time
    const int h0 = h_ptr[row], nh = h_ptr[row + 1] - h0;
#pragma unroll 1
    for (int b0 = 0; b0 < nh; b0 += EX_HB) {
        const int nb = min(EX_HB, nh - b0), nht = (nb + 15) >> 4, np = LT * nht;
        if (tid < EX_HB) {
            int hg = -1;
            if (tid < nb) {
                const int64_t x = (int64_t)hist_lo + (int64_t)h_idx[h0 + b0 + tid];
                hg = x >= ilo && x < ihi ? (int)x : -1;
            }
            s_hid[tid] = hg;
        }
        __syncthreads();
        {
            const int hg = s_hid[lrow];
            rv[NU] = hg >= 0;
            rp[NU] = reinterpret_cast<const ltg_u32x4*>(image) + (size_t)(rv[NU] ? hg - image_lo : 0) * ST_C16 + q;
        }
        ltg_u32x4 reg[NU + 1];
#pragma unroll
        for (int u = 0; u <= NU; ++u) reg[u] = rv[u] ? rp[u][0] : ltg_u32x4{0u, 0u, 0u, 0u};
        int tt[PW];                                  // pair p = w + NW u -> (history tile p % nht) << 8 | (list tile p / nht); -1: none
        ltg_f32x4 acc[PW];
#pragma unroll
        for (int u = 0; u < PW; ++u) {
            const int p = w + NW * u;
            tt[u] = p < np ? (((p % nht) << 8) | (p / nht)) : -1;
            acc[u] = ltg_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll 1
        for (int ks = 0; ks < ST_KS; ++ks) {
#pragma unroll
            for (int u = 0; u <= NU; ++u) {          // rows lrow + 64 u: tile (4 u + lrow / 16); u == NU: the history tiles behind the CT list tiles
                const int rr = lrow + 64 * u;
                stage[(rr >> 4) * 64 + q * 16 + (rr & 15)] = reg[u];
            }
            __syncthreads();
            if (ks + 1 < ST_KS) {
#pragma unroll
                for (int u = 0; u <= NU; ++u)
                    if (rv[u]) reg[u] = rp[u][4 * (ks + 1)];
            }
#pragma unroll
            for (int u = 0; u < PW; ++u) {
                if (tt[u] >= 0) {
                    const ltg_bf16x8 a = __builtin_bit_cast(ltg_bf16x8, stage[(CT + (tt[u] >> 8)) * 64 + lane]);
                    const ltg_bf16x8 bb = __builtin_bit_cast(ltg_bf16x8, stage[(tt[u] & 255) * 64 + lane]);
                    acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[u], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // 3. acc[j] = score(history row 16 ht + 4 lq + j, list entry 16 lt + lr)
#pragma unroll
        for (int u = 0; u < PW; ++u) {
            if (tt[u] >= 0) {
                float* o = Sc + (16 * (tt[u] >> 8) + 4 * lq) * LEP + 16 * (tt[u] & 255) + lr;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j * LEP] = acc[u][j];
            }
        }
        __syncthreads();
        // 4. the fold of entry tid
        if (g >= 0) {
            for (int h = 0; h < nb; ++h) {
                const int hg = s_hid[h];
                if (hg < 0 || hg == g) continue;
                const uint64_t c = tk_comp(tk_key(Sc[h * LEP + tid]), hg);
                if (c > best[EX_R - 1]) {
#pragma unroll
                    for (int j = EX_R - 1; j >= 1; --j) best[j] = c > best[j - 1] ? best[j - 1] : (c > best[j] ? c : best[j]);
                    best[0] = c > best[0] ? c : best[0];
                }
            }
        }
        __syncthreads();                             // s_hid, the stage and the scores are free for the next block
    }

    // 5. the lists
    if (tid < top) {
        const size_t o = (row * top + tid) * (size_t)r_out;
#pragma unroll
        for (int j = 0; j < EX_R; ++j) {
            if (j < r_out) {
                const uint64_t c = best[j];
                const uint32_t key = (uint32_t)(c >> 32);
                id_out[o + j] = c != 0ull ? (int)~(uint32_t)c : -1;
                score_out[o + j] = c != 0ull ? __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key) : -INFINITY;
            }
        }
    }
}
