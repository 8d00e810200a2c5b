// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_neighbors.h): diversified top-K
// lists (ltg_topk_diversify).  Greedy maximal marginal relevance over a row's sorted candidate list: the next entry is the
// candidate with the largest  lambda * rel_i - (1 - lambda) * max_{p picked} S[i][p],  S = the products of the candidates' image rows.
//
// One workgroup per user row, one thread per candidate position (CT tiles of 16 candidates, CT = 4 / 8 / 16).
//   1. n = the number of candidates in front of the first id outside the image (padding included); NT = ceil(n / 16) tiles.
//   2. S: the candidates' image rows are gathered one K step (64 B per row) at a time into LDS in fragment order -- a row's 16-byte chunks
//      are A- and B-fragment order already -- while the next step's loads are in flight; the NT (NT + 1) / 2 tile pairs (ti >= tj) are dealt
//      round-robin to the waves, every pair one chain of 19 v_mfma_f32_16x16x32_bf16 in a wave's accumulators (ltg_item_neighbors' score).
//      The lower triangle of tiles is then written to LDS in fp32, 1 KB per tile: S never leaves the chip and is never rounded.
//   3. min(k, n) greedy rounds: every lane keeps m_i and its objective, a wave takes the 32-bit maximum of the keys by DPP and the lowest
//      lane holding it, the waves meet through one LDS word each and one barrier per round.
//   4. the picks are written in pick order with their original scores; stat_out = the mean S over the pairs of the first min(k, n)
//      candidates and over the pairs of the picks.
// No global workspace, no atomics outside LDS (one integer min), every image row index is checked against [0, image_rows) first.
#pragma once

// where S[i][j] lives (floats from the start of S).  Tile (th, tl), th >= tl, is tile th (th + 1) / 2 + tl; inside it element (a in th,
// b in tl) sits at b * 16 + a with a's group of four xor-ed by b's, so that a column read (16 b of one a) and a row read (16 a of one b)
// both touch 16 banks, and a lane's four accumulators stay one aligned 16-byte store.
__device__ __forceinline__ int dv_saddr(int i, int j) {
    const int hi = max(i, j), lo = min(i, j), th = hi >> 4, tl = lo >> 4, a = hi & 15, b = lo & 15;
    return (((th * (th + 1)) >> 1) + tl) * 256 + b * 16 + ((((a >> 2) ^ (b >> 2)) << 2) | (a & 3));
}

// the wave's maximum in every lane: quads and rows by DPP, the four rows by lane reads
__device__ __forceinline__ uint32_t dv_wave_umax(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));     // quad_perm [1, 0, 3, 2]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));     // quad_perm [2, 3, 0, 1]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));    // row_half_mirror
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true));    // row_mirror
    const uint32_t a = __builtin_amdgcn_readlane((int)v, 0), b = __builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = __builtin_amdgcn_readlane((int)v, 32), d = __builtin_amdgcn_readlane((int)v, 48);
    return max(max(a, b), max(c, d));
}

// the sum of v over the workgroup in every thread (order fixed: deterministic).  Ends with a barrier.
template <int NW>
__device__ __forceinline__ float dv_block_sum(float v, float* s_sum) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();              // the last use of s_sum is over
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int x = 0; x < NW; ++x) t += s_sum[x];
    return t;
}

template <int CT>
__global__ __launch_bounds__(CT * 16) void k_topk_diversify(const unsigned short* __restrict__ image, int image_lo, int image_rows, int c_in,
                                                            const float* __restrict__ score_in, const int32_t* __restrict__ id_in, float lambda,
                                                            int k, float* __restrict__ score_out, int32_t* __restrict__ id_out,
                                                            float* __restrict__ stat_out) {
    constexpr int NTHR = CT * 16, NW = NTHR / 64, NPMAX = CT * (CT + 1) / 2, PW = (NPMAX + NW - 1) / NW;
    extern __shared__ __attribute__((aligned(16))) ltg_u32x4 dv_lds[];      // stage [CT][64] x 16 B | S: NPMAX tiles x 1 KB
    __shared__ float s_sc[NTHR];
    __shared__ int s_id[NTHR], s_pick[NTHR], s_tab[NPMAX], s_n;
    __shared__ uint64_t s_red[2][NW];
    __shared__ float s_sum[NW];
    ltg_u32x4* stage = dv_lds;
    float* Sl = reinterpret_cast<float*>(dv_lds + CT * 64);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const size_t row = blockIdx.x;

    // 1. the row's candidates; n = the first position whose id is outside the image
    int id = -1;
    float sc = -INFINITY;
    if (tid < c_in) {
        id = id_in[row * c_in + tid];
        sc = score_in[row * c_in + tid];
    }
    const bool inside = (int64_t)id >= (int64_t)image_lo && (int64_t)id < (int64_t)image_lo + (int64_t)image_rows;
    if (tid == 0) s_n = c_in;
    for (int p = tid; p < NPMAX; p += NTHR) {       // pair p -> (ti, tj), ti >= tj, in the order of S's tiles
        int ti = 0;
        while (((ti + 1) * (ti + 2)) / 2 <= p) ++ti;
        s_tab[p] = (ti << 8) | (p - (ti * (ti + 1)) / 2);
    }
    s_id[tid] = id;
    s_sc[tid] = sc;
    __syncthreads();
    if (tid < c_in && !inside) atomicMin(&s_n, tid);
    __syncthreads();
    const int n = s_n, kk = min(k, n);
    float* so = score_out + row * k;
    int32_t* io = id_out + row * k;
    if (n == 0) {
        for (int r = tid; r < k; r += NTHR) {
            io[r] = -1;
            so[r] = -INFINITY;
        }
        if (stat_out && tid < 2) stat_out[row * 2 + tid] = 0.f;
        return;
    }

    // 2. S.  Loader: four consecutive lanes take the four chunks of one row's K step; a thread serves rows (tid >> 2) + (NTHR / 4) u.
    const int NT_ = (n + 15) >> 4, NP = (NT_ * (NT_ + 1)) >> 1;
    const int q = tid & 3;
    const ltg_u32x4* rp[4];
    bool rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = (tid >> 2) + (NTHR / 4) * u;
        rv[u] = r < n;                              // (r < n: s_id[r] is inside the image)
        rp[u] = reinterpret_cast<const ltg_u32x4*>(image) + (size_t)(rv[u] ? s_id[r] - image_lo : 0) * ST_C16 + q;
    }
    ltg_u32x4 reg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) reg[u] = rv[u] ? rp[u][0] : ltg_u32x4{0u, 0u, 0u, 0u};
    int tt[PW];
    ltg_f32x4 acc[PW];
#pragma unroll
    for (int u = 0; u < PW; ++u) {
        const int p = w + NW * u;
        tt[u] = p < NP ? __builtin_amdgcn_readfirstlane(s_tab[min(p, NPMAX - 1)]) : -1;
        acc[u] = ltg_f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int ks = 0; ks < ST_KS; ++ks) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = (tid >> 2) + (NTHR / 4) * u;
            stage[(r >> 4) * 64 + q * 16 + (r & 15)] = reg[u];
        }
        __syncthreads();
        if (ks + 1 < ST_KS) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (rv[u]) reg[u] = rp[u][4 * (ks + 1)];
        }
#pragma unroll
        for (int u = 0; u < PW; ++u) {
            if (tt[u] >= 0) {
                const ltg_bf16x8 a = __builtin_bit_cast(ltg_bf16x8, stage[(tt[u] >> 8) * 64 + lane]);
                const ltg_bf16x8 b = __builtin_bit_cast(ltg_bf16x8, stage[(tt[u] & 255) * 64 + lane]);
                acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[u], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // acc[j] = S[16 ti + 4 lq + j][16 tj + lr]
#pragma unroll
    for (int u = 0; u < PW; ++u)
        if (tt[u] >= 0) *reinterpret_cast<ltg_f32x4*>(Sl + (w + NW * u) * 256 + lr * 16 + 4 * (lq ^ (lr >> 2))) = acc[u];
    __syncthreads();

    // 3. the greedy rounds
    const float oml = __fsub_rn(1.f, lambda);
    const float s0 = s_sc[0], sl = s_sc[n - 1];
    const float rel = tid < n && s0 != sl ? __fdiv_rn(__fsub_rn(sc, sl), __fsub_rn(s0, sl)) : 0.f;
    const float lrel = __fmul_rn(lambda, rel);
    bool alive = tid < n;
    float m = 0.f, obj = 0.f;
    int p = 0;
    for (int r = 0; r < kk; ++r) {
        if (r > 0) {
            const uint32_t key = alive ? tk_key(obj) : 0u;        // (0 is below the key of every non-NaN objective)
            const uint32_t wm = dv_wave_umax(key);
            uint64_t word = 0ull;                                  // (objective key, 0xFFFF - position): one max gives the tie rule
            if (wm != 0u) word = ((uint64_t)wm << 32) | (uint64_t)(0xFFFF - (w * 64 + (int)__builtin_ctzll(__ballot(key == wm))));
            if (NW > 1) {
                if (lane == 0) s_red[r & 1][w] = word;
                __syncthreads();
#pragma unroll
                for (int x = 0; x < NW; ++x) word = max(word, s_red[r & 1][x]);
            }
            p = __builtin_amdgcn_readfirstlane(0xFFFF - (int)(word & 0xFFFFull));
        }
        if (tid == 0) s_pick[r] = p;
        if (tid == p) alive = false;
        const float s = Sl[dv_saddr(tid, p)];
        m = r == 0 ? s : fmaxf(m, s);
        obj = __fsub_rn(lrel, __fmul_rn(oml, m));
    }
    __syncthreads();

    // 4. the list in pick order, the picks' own scores
    for (int r = tid; r < k; r += NTHR) {
        const int pr = r < kk ? s_pick[r] : -1;
        io[r] = pr >= 0 ? s_id[pr] : -1;
        so[r] = pr >= 0 ? s_sc[pr] : -INFINITY;
    }
    if (!stat_out) return;
    // the mean S over the unordered pairs: column j of the first kk positions (before) / of the picks (after), split over NTHR / kk threads
    float before = 0.f, after = 0.f;
    const int g = tid / kk, j = tid - g * kk, G = NTHR / kk;
    if (g < G) {
        const int pj = s_pick[j];
        for (int i = g; i < j; i += G) {
            before += Sl[dv_saddr(i, j)];
            after += Sl[dv_saddr(s_pick[i], pj)];
        }
    }
    before = dv_block_sum<NW>(before, s_sum);
    after = dv_block_sum<NW>(after, s_sum);
    if (tid == 0) {
        const float pairs = (float)((kk * (kk - 1)) >> 1);
        stat_out[row * 2] = kk > 1 ? __fdiv_rn(before, pairs) : 0.f;
        stat_out[row * 2 + 1] = kk > 1 ? __fdiv_rn(after, pairs) : 0.f;
    }
}
