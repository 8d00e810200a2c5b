// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_calibrate.h): critic-checked lists --
// the discriminator scores and gates each user's niche entries.
//   k_pair_critic     per user row: anchors (popular history items with features) x scored entries (niche list entries with features) pair
//                     logits on chip, reduced per entry to a fixed-point sum and the best anchor
//   k_critic_finish   sum / count -> the mean logit per entry, the scored entries per row
//   k_topk_gate       candidates + critic -> the first k entries that are unscored or reach tau
//
// k_pair_critic is k_pair_companions with the epilogue turned from "select over candidates" into "reduce over queries": the pair chain is
// that kernel's, acc <- fma(w4[j], rcp(fma(Ea[j], Eb[j], 1)), acc) over j = 0 .. h3 - 1 ascending from 0, then fma(-2, acc, c0), c0 summed
// in fp64 -- the same bits for the same two image rows (the anchor's row is the wave-uniform operand there and here).
// One workgroup (8 waves) per user row.
//   1. thread e < top looks at entry e: scored-candidate iff 0 <= id < n_items and niche_row[id] is a row of the niche image; the
//      candidates are compacted in entry order (ballot and prefix count).
//   2. a step = 64 compacted entries, one per lane, the same 64 for every wave: their niche-image rows are copied into LDS, row stride
//      ld | 1 floats (odd: lane c reads column j of its own row without a bank conflict).
//   3. per step the history is walked in blocks of 512 items, one per thread: hist_lo + index is checked against [0, n_items), then
//      pop_row against the popular image; the block's anchors (image row, global id) are compacted into LDS in history order, and their
//      image rows are staged in LDS 32 at a time (once for all steps when the whole history has no more than 32 anchors).  Groups of R
//      anchors are dealt round-robin to the waves (R = 1 while no more anchors than waves are staged, else 2); a group's rows are
//      wave-uniform broadcast reads, so a loop body is one ds_read_b32 per column plus one ds_read_b128 per anchor and four columns and,
//      per anchor, fma / rcp / fma on R independent accumulators.  (Scalar loads of the anchor rows, as k_pair_companions reads its
//      queries, left a user's few anchors waiting on L2 once per 64-byte line with nothing to hide it: DESIGN 5.20.)
//   4. a lane turns each logit s into q = llrint((double) s * 2^24) and adds it to its int64 sum, and keeps the largest (key, ~anchor id)
//      word (ltg_topk.h's words: score descending, then the lower id).  Integer adds and max commute: the result does not depend on
//      which wave, block or call holds an anchor.
//   5. the waves combine through LDS (integer add, max) and wave 0 writes the step's entries; entries that are no candidates are written
//      as sum 0 / no anchor by their own thread.  The anchors of this call's part of the history are counted once, before the steps.
// No workspace, no atomics at all, bit-identical from run to run.
#pragma once

constexpr int CR_NT = 512;          // 8 waves, two per SIMD
constexpr int CR_ET = 64;           // entries per step: one per lane
constexpr int CR_HB = 512;          // history items per block: one per thread
constexpr int CR_R = 2;             // anchors in flight per wave when a block holds more anchors than waves (else 1: an anchor per wave)
constexpr int CR_JU = 4;            // j per unrolled block (k_pair_companions' PC_JU)
constexpr int CR_NW = CR_NT / 64;
constexpr int CR_AB = 32;           // anchor rows staged in LDS at a time (four per wave): tile + rows <= 64 x 353 x 4 + 32 x 352 x 4 = 132 KiB

// history item b0 + tid of the row -> its row of the popular image and its global id, -1 / -1 when it is no anchor (past the history's end,
// outside the catalogue, not on the popular side)
__device__ __forceinline__ void cr_anchor_lookup(const int32_t* __restrict__ h_idx, int h0, int nh, int b0, int hist_lo, int n_items,
                                                 const int32_t* __restrict__ pop_row, int n_pop, int& arow, int& gid) {
    const int tid = threadIdx.x;
    arow = -1;
    gid = -1;
    if (b0 + tid < nh) {
        const int64_t x = (int64_t)hist_lo + (int64_t)h_idx[h0 + b0 + tid];
        if (x >= 0 && x < (int64_t)n_items) {
            const int r = pop_row[x];
            if (r >= 0 && r < n_pop) {
                arow = r;
                gid = (int)x;
            }
        }
    }
}

// the block's anchors (cr_anchor_lookup's, one per thread) compacted in history order into s_row / s_gid -> their number.  Every thread of
// the workgroup calls it; ends with a barrier.
__device__ __forceinline__ int cr_anchor_compact(int arow, int gid, int* s_row, int* s_gid, int* s_wcnt) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long m = __ballot(arow >= 0);
    if (lane == 0) s_wcnt[w] = __popcll(m);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int v = 0; v < CR_NW; ++v) {
        const int c = s_wcnt[v];
        off += v < w ? c : 0;
        total += c;
    }
    if (arow >= 0) {
        const int p = off + __popcll(m & ((1ull << lane) - 1ull));
        s_row[p] = arow;
        s_gid[p] = gid;
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ int cr_anchor_block(const int32_t* __restrict__ h_idx, int h0, int nh, int b0, int hist_lo, int n_items,
                                               const int32_t* __restrict__ pop_row, int n_pop, int* s_row, int* s_gid, int* s_wcnt) {
    int arow, gid;
    cr_anchor_lookup(h_idx, h0, nh, b0, hist_lo, n_items, pop_row, n_pop, arow, gid);
    return cr_anchor_compact(arow, gid, s_row, s_gid, s_wcnt);
}

// The staged anchors against the step's tile: arows [n][ld] fp32 in LDS (16-byte aligned rows), gids [n] their global ids.  Groups of R
// anchors are dealt round-robin to the waves (wave w: anchors R w .. R w + R - 1, then R (w + 8) ..).  A group's rows are wave-uniform:
// broadcast LDS reads, four columns per ds_read_b128, a block of CR_JU columns ahead of their use as in k_pair_companions.  sum / best: the
// lane's running fixed-point sum and best (key, ~anchor id) word.
template <int R>
__device__ __forceinline__ void cr_groups(int n, int w, int ld, int h3, const float* arows, const int* gids, const float* tl, const float* s_w4,
                                          const float& s_c0, long long& sum, uint64_t& best) {
    static_assert(CR_JU == 4, "a block of columns is one float4");
    const int nfull = h3 / CR_JU;
#pragma unroll 1
    for (int a0 = R * w; a0 < n; a0 += R * CR_NW) {
        const float* ea[R];      // anchors past the last mirror it (their result is dropped)
        int ag[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int a = min(a0 + r, n - 1);
            ea[r] = arows + a * ld;
            ag[r] = gids[a];
        }
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        float en[CR_JU];
        float4 qn[R], wn;
        if (nfull > 0) {
#pragma unroll
            for (int u = 0; u < CR_JU; ++u) en[u] = tl[u];
            wn = *reinterpret_cast<const float4*>(s_w4);
#pragma unroll
            for (int r = 0; r < R; ++r) qn[r] = *reinterpret_cast<const float4*>(ea[r]);
        }
#pragma unroll 1
        for (int b = 0; b < nfull; ++b) {
            const int j = b * CR_JU;
            float e[CR_JU], qv[R][CR_JU];
            const float wv[CR_JU] = {wn.x, wn.y, wn.z, wn.w};
#pragma unroll
            for (int u = 0; u < CR_JU; ++u) e[u] = en[u];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                qv[r][0] = qn[r].x;
                qv[r][1] = qn[r].y;
                qv[r][2] = qn[r].z;
                qv[r][3] = qn[r].w;
            }
            if (b + 1 < nfull) {
#pragma unroll
                for (int u = 0; u < CR_JU; ++u) en[u] = tl[j + CR_JU + u];
                wn = *reinterpret_cast<const float4*>(s_w4 + j + CR_JU);
#pragma unroll
                for (int r = 0; r < R; ++r) qn[r] = *reinterpret_cast<const float4*>(ea[r] + j + CR_JU);
            }
#pragma unroll
            for (int u = 0; u < CR_JU; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(wv[u], __builtin_amdgcn_rcpf(fmaf(qv[r][u], e[u], 1.f)), acc[r]);
        }
        for (int j = nfull * CR_JU; j < h3; ++j) {
            const float e = tl[j], wj = s_w4[j];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fmaf(wj, __builtin_amdgcn_rcpf(fmaf(ea[r][j], e, 1.f)), acc[r]);
        }
        // 4. the fixed-point sum and the best anchor
        const float c0 = s_c0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (a0 + r < n) {
                const float s = fmaf(-2.f, acc[r], c0);
                sum += __double2ll_rn((double)s * 16777216.0);
                const uint64_t word = tk_comp(tk_key(s), ag[r]);
                best = word > best ? word : best;
            }
        }
    }
}

// rows s_row[0 .. n) of the popular image -> arows [n][ld] in LDS: wave w carries rows w, w + 8, ..; every load is requested before the first
// LDS write.  No barrier inside.
__device__ __forceinline__ void cr_stage_anchors(const float* __restrict__ Ep, int ld, const int* s_row, int n, float* arows, int w, int lane) {
    float tv[CR_AB / CR_NW][PC_NJ];
#pragma unroll
    for (int i = 0; i < CR_AB / CR_NW; ++i) {
        const float* src = Ep + (size_t)s_row[min(w + CR_NW * i, n - 1)] * ld;
#pragma unroll
        for (int u = 0; u < PC_NJ; ++u)
            if (64 * u < ld) tv[i][u] = src[min(lane + 64 * u, ld - 1)];
    }
#pragma unroll
    for (int i = 0; i < CR_AB / CR_NW; ++i)
#pragma unroll
        for (int u = 0; u < PC_NJ; ++u)
            if (w + CR_NW * i < n && lane + 64 * u < ld) arows[(w + CR_NW * i) * ld + lane + 64 * u] = tv[i][u];
}

__global__ __launch_bounds__(CR_NT) void k_pair_critic(int h3, int ld, const float* __restrict__ Ep, int n_pop, const float* __restrict__ En,
                                                       int n_niche, const int32_t* __restrict__ pop_row, const int32_t* __restrict__ niche_row,
                                                       int n_items, const int32_t* __restrict__ h_ptr, const int32_t* __restrict__ h_idx,
                                                       int hist_lo, int k_in, const int32_t* __restrict__ id_in, int top,
                                                       const float* __restrict__ w4, const float* __restrict__ b4,
                                                       long long* __restrict__ sum_out, int32_t* __restrict__ cnt_out,
                                                       float* __restrict__ best_s, int32_t* __restrict__ best_i) {
    extern __shared__ __attribute__((aligned(16))) float cr_tile[];     // tile [CR_ET][ld | 1] fp32 | anchor rows [CR_AB][ld] fp32
    __shared__ long long s_sum[CR_NW][CR_ET];
    __shared__ uint64_t s_best[CR_NW][CR_ET];
    __shared__ int s_arow[CR_HB], s_agid[CR_HB];
    __shared__ int s_erow[LTG_CRITIC_MAX_TOP], s_epos[LTG_CRITIC_MAX_TOP];
    __shared__ int s_wcnt[CR_NW];
    __shared__ float s_c0;
    __shared__ __attribute__((aligned(16))) float s_w4[PC_MAX_H3];
    const int ldp = ld | 1;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row = blockIdx.x;

    // every load of the prologue is requested before the first barrier: w4, the row's entries, the first block of its history
    for (int j = tid; j < h3; j += CR_NT) s_w4[j] = w4[j];
    const float b4v = b4[0];
    const int h0 = h_ptr[row], nh = h_ptr[row + 1] - h0;
    int arow0, agid0;
    cr_anchor_lookup(h_idx, h0, nh, 0, hist_lo, n_items, pop_row, n_pop, arow0, agid0);

    // 1. the row's entries
    int erow = -1;
    if (tid < top) {
        const int g = id_in[row * k_in + tid];
        if (g >= 0 && g < n_items) {
            const int r = niche_row[g];
            if (r >= 0 && r < n_niche) erow = r;
        }
    }
    const unsigned long long em = __ballot(erow >= 0);
    if (lane == 0) s_wcnt[w] = __popcll(em);
    __syncthreads();
    int eoff = 0, n_ent = 0;
#pragma unroll
    for (int v = 0; v < CR_NW; ++v) {
        const int c = s_wcnt[v];
        eoff += v < w ? c : 0;
        n_ent += c;
    }
    if (erow >= 0) {
        const int p = eoff + __popcll(em & ((1ull << lane) - 1ull));
        s_erow[p] = erow;
        s_epos[p] = tid;
    }
    if (tid < top && erow < 0) {        // no candidate: nothing else writes this entry
        const size_t o = row * top + tid;
        sum_out[o] = 0ll;
        best_s[o] = -INFINITY;
        best_i[o] = -1;
    }
    if (tid == 0) {                     // c0 as k_pair_companions sums it: fp64, b4 then w4 ascending, rounded once (w4 is in LDS by now;
        double c = (double)b4v;         // eight reads in flight per eight dependent adds)
        int j = 0;
        for (; j + 8 <= h3; j += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = s_w4[j + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) c += (double)v[u];
        }
        for (; j < h3; ++j) c += (double)s_w4[j];
        s_c0 = (float)c;
    }
    __syncthreads();                    // (s_wcnt is free again)

    // the anchors of this call's part of the history
    int n_anchor = cr_anchor_compact(arow0, agid0, s_arow, s_agid, s_wcnt);
#pragma unroll 1
    for (int b0 = CR_HB; b0 < nh; b0 += CR_HB) n_anchor += cr_anchor_block(h_idx, h0, nh, b0, hist_lo, n_items, pop_row, n_pop, s_arow, s_agid, s_wcnt);
    if (tid == 0) cnt_out[row] = n_anchor;

    // a history of one block with no more than CR_AB anchors: their image rows are staged once and stay for every step
    float* arows = cr_tile + CR_ET * ldp;       // (64 ldp floats: a multiple of 256 bytes)
    const bool resident = nh <= CR_HB && n_anchor <= CR_AB;
    if (resident && n_anchor > 0 && n_ent > 0) cr_stage_anchors(Ep, ld, s_arow, n_anchor, arows, w, lane);      // (the step's first barrier covers it)
    const float* tl = cr_tile + lane * ldp;
#pragma unroll 1
    for (int base = 0; base < n_ent; base += CR_ET) {
        // 2. the step's niche-image rows: wave w carries rows w, w + 8, ... (rows past the last entry mirror it)
        {
            float tv[CR_ET / CR_NW][PC_NJ];     // every load is requested before the first LDS write
#pragma unroll
            for (int i = 0; i < CR_ET / CR_NW; ++i) {
                const float* src = En + (size_t)s_erow[min(base + w + CR_NW * i, n_ent - 1)] * ld;
#pragma unroll
                for (int u = 0; u < PC_NJ; ++u)
                    if (64 * u < ld) tv[i][u] = src[min(lane + 64 * u, ld - 1)];
            }
#pragma unroll
            for (int i = 0; i < CR_ET / CR_NW; ++i)
#pragma unroll
                for (int u = 0; u < PC_NJ; ++u)
                    if (lane + 64 * u < ld) cr_tile[(w + CR_NW * i) * ldp + lane + 64 * u] = tv[i][u];
        }
        long long sum = 0ll;
        uint64_t best = 0ull;
        __syncthreads();
        // 3. the history, a block at a time; a block's anchors, CR_AB rows of the popular image at a time, through LDS
#pragma unroll 1
        for (int b0 = 0; b0 < nh; b0 += CR_HB) {
            const int na = nh <= CR_HB ? n_anchor : cr_anchor_block(h_idx, h0, nh, b0, hist_lo, n_items, pop_row, n_pop, s_arow, s_agid, s_wcnt);
#pragma unroll 1
            for (int sub = 0; sub < na; sub += CR_AB) {
                const int n = min(CR_AB, na - sub);
                if (!resident) {
                    cr_stage_anchors(Ep, ld, s_arow + sub, n, arows, w, lane);
                    __syncthreads();
                }
                if (n <= CR_NW) cr_groups<1>(n, w, ld, h3, arows, s_agid + sub, tl, s_w4, s_c0, sum, best);       // an anchor per wave
                else cr_groups<CR_R>(n, w, ld, h3, arows, s_agid + sub, tl, s_w4, s_c0, sum, best);
                if (!resident) __syncthreads();     // every wave is done with the staged rows (and, after the last, with the block's anchors)
            }
        }
        // 5. the waves' parts of the step
        s_sum[w][lane] = sum;
        s_best[w][lane] = best;
        __syncthreads();
        if (w == 0 && base + lane < n_ent) {
            long long t = 0ll;
            uint64_t m = 0ull;
#pragma unroll
            for (int v = 0; v < CR_NW; ++v) {
                t += s_sum[v][lane];
                const uint64_t c = s_best[v][lane];
                m = c > m ? c : m;
            }
            const size_t o = row * top + s_epos[base + lane];
            const uint32_t key = (uint32_t)(m >> 32);
            sum_out[o] = t;
            best_i[o] = m != 0ull ? (int)~(uint32_t)m : -1;
            best_s[o] = m != 0ull ? __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key) : -INFINITY;
        }
        __syncthreads();                // the tile and the combine buffers are free for the next step
    }
}

// One thread per (row, entry); the row's scored entries are counted by its first wave's ballots (rows of up to 256 entries: one block a row).
__global__ __launch_bounds__(256) void k_critic_finish(int k_in, const int32_t* __restrict__ id_in, int top, const int32_t* __restrict__ niche_row,
                                                       int n_items, int n_niche, const long long* __restrict__ sum, const int32_t* __restrict__ cnt,
                                                       float* __restrict__ crit_out, int32_t* __restrict__ scored_out) {
    __shared__ int s_n[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t row = blockIdx.x;
    const int n_anchor = cnt[row];
    bool scored = false;
    if (tid < top && n_anchor > 0) {
        const int g = id_in[row * k_in + tid];
        if (g >= 0 && g < n_items) {
            const int r = niche_row[g];
            scored = r >= 0 && r < n_niche;
        }
    }
    if (tid < top) crit_out[row * top + tid] = scored ? (float)((double)sum[row * top + tid] / ((double)n_anchor * 16777216.0)) : 0.f;
    const unsigned long long m = __ballot(scored);
    if (lane == 0) s_n[w] = __popcll(m);
    __syncthreads();
    if (tid == 0) scored_out[row] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// One wave per row, four rows per workgroup.  Candidates are walked 64 at a time: an entry passes iff it is no padding and is unscored
// (flag < 0) or crit >= tau; its place in the list is the count of passing entries before it (ballot and prefix count).
__global__ __launch_bounds__(256) void k_topk_gate(int n_rows, int c_in, const float* __restrict__ cand_score, const int32_t* __restrict__ cand_id,
                                                   const float* __restrict__ crit, const int32_t* __restrict__ flag, float tau, int k,
                                                   float* __restrict__ score_out, int32_t* __restrict__ id_out, int32_t* __restrict__ stat_out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;          // (wave-uniform; no barrier below)
    const size_t in = (size_t)row * c_in, out = (size_t)row * k;
    int n_pass = 0, n_scored = 0, n_rej = 0;
    for (int b = 0; b < c_in; b += 64) {
        const int i = b + lane;
        int g = -1;
        float sc = -INFINITY;
        bool scored = false, pass = false;
        if (i < c_in) {
            g = cand_id[in + i];
            sc = cand_score[in + i];
            scored = g >= 0 && flag[in + i] >= 0;
            pass = g >= 0 && (!scored || crit[in + i] >= tau);
        }
        const unsigned long long pm = __ballot(pass), below = (1ull << lane) - 1ull;
        const int p = n_pass + __popcll(pm & below);
        if (pass && p < k) {
            score_out[out + p] = sc;
            id_out[out + p] = g;
        }
        n_scored += __popcll(__ballot(scored));
        n_rej += __popcll(__ballot(scored && !pass && p < k));
        n_pass += __popcll(pm);
    }
    const int len = min(n_pass, k);
    for (int p = len + lane; p < k; p += 64) {
        score_out[out + p] = -INFINITY;
        id_out[out + p] = -1;
    }
    if (lane == 0) {
        stat_out[(size_t)row * 3 + 0] = n_scored;
        stat_out[(size_t)row * 3 + 1] = n_rej;
        stat_out[(size_t)row * 3 + 2] = len;
    }
}
