// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_cap.h): share-targeted top-K lists
// (ltg_topk_share).  The promoted groups get `want` of all served slots, placed where they cost the least relevance.
//
// Per row two ltg_topk_groups lists, promoted and rest.  The plain list is the first kk entries of their merge: a promoted, b rest.  Step t
// of a row swaps the worst remaining rest entry for the best promoted item not yet in the list, at the cost  c_t = rest[b - t] - pro[a + t - 1]
// (one fp32 subtraction, -0.0 taken as +0.0).  Both lists descend, so the costs of a row never decrease: taking the globally cheapest steps
// is optimal, and a row's taken steps are a prefix.  A step is the word  (bits(c_t) << 32) | (row * k + t - 1);  costs are >= 0, so words
// order as (cost, row, t), they are distinct, and the words of a row strictly increase.
//
// k_share_zero:   state, the 8 x 256 global bins and the selection block <- 0: nothing relies on what the workspace held.
// k_share_steps:  one wave per row.  The lengths of the two lists (the first id < 0 ends one), a by a binary search along the merge path,
//   the row's words (all-ones where there is no step), a and kk per row, and the integer sums A, N, sum kk by one atomic per workgroup.
// k_share_hist / k_share_pick: a radix select of the take-th smallest word, most significant digit first, 8 bits a pass, a fixed 8 passes.
//   Every workgroup counts the words that agree with the digits chosen so far into a 256-bin LDS histogram and adds it to the pass's
//   global bins (integer sums: order-free); one workgroup then picks the digit and the rank left inside it.  take = min(max(0, want - A), N)
//   is derived on the device by every kernel that needs it; with take = 0 the passes do nothing.
// k_share_finish: one wave per row.  t_u = the row's words <= the threshold, then the first a + t_u promoted and the first b - t_u rest
//   entries merged: every entry finds its place by a binary search in the other list and is written with its original score.
// Ids never index anything; a word's low half is written, never read back as an index.
#pragma once

constexpr int SH_NT = 256;           // 4 waves
constexpr int SH_STATE = 8;          // == LTG_SHARE_STATE: {A, N, take, rows changed, bits of the threshold cost, sum kk, 0, 0}
constexpr int SH_PASSES = 8;
constexpr int SH_HIST_PER = 8;       // words per thread and trip of the histogram kernel's grid

struct sh_sel {                      // the selection as it stands: the digits chosen so far, and the rank left among the words that share them
    uint64_t prefix;
    int32_t rank;
    int32_t pad;
};

__device__ __forceinline__ uint64_t sh_word(const float* __restrict__ s, const int32_t* __restrict__ id, int i) { return tk_comp(tk_key(s[i]), id[i]); }

__device__ __forceinline__ int sh_take(const int32_t* __restrict__ state, int64_t want) {
    const int64_t miss = want - (int64_t)state[0];
    return (int)min(max(miss, (int64_t)0), (int64_t)state[1]);
}

// the non-padding entries of a list of m_in: the position of its first id < 0 (wave-uniform)
__device__ __forceinline__ int sh_len(const int32_t* __restrict__ id, int m_in, int lane) {
    for (int j0 = 0; j0 < m_in; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long neg = __ballot(j < m_in ? id[j] < 0 : true);
        if (neg != 0ull) return j0 + (int)__builtin_ctzll(neg);
    }
    return m_in;
}

// how many of the first n entries of a descending list come before the word w
__device__ __forceinline__ int sh_before(const float* __restrict__ s, const int32_t* __restrict__ id, int n, uint64_t w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sh_word(s, id, mid) > w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SH_NT) void k_share_zero(int32_t* __restrict__ state, int32_t* __restrict__ bins, sh_sel* __restrict__ sel) {
    const int tid = threadIdx.x;
    if (tid < SH_STATE) state[tid] = 0;
    for (int i = tid; i < SH_PASSES * 256; i += SH_NT) bins[i] = 0;
    if (tid == 0) {
        sel->prefix = 0ull;
        sel->rank = 0;
        sel->pad = 0;
    }
}

__global__ __launch_bounds__(SH_NT) void k_share_steps(int n_rows, int m_in, int k, const float* __restrict__ score_pro, const int32_t* __restrict__ id_pro,
                                                       const float* __restrict__ score_rest, const int32_t* __restrict__ id_rest,
                                                       uint64_t* __restrict__ words, int32_t* __restrict__ row_a, int32_t* __restrict__ row_kk,
                                                       int32_t* __restrict__ state) {
    __shared__ int s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, row = blockIdx.x * (SH_NT / 64) + (threadIdx.x >> 6);
    if (row < n_rows) {                              // (whole waves)
        const size_t base = (size_t)row * (size_t)m_in;
        const float *ps = score_pro + base, *rs = score_rest + base;
        const int32_t *pi = id_pro + base, *ri = id_rest + base;
        const int np = sh_len(pi, m_in, lane), nr = sh_len(ri, m_in, lane);
        const int kk = min(k, np + nr);
        // a = the largest x with pro[x - 1] before rest[kk - x]: that entry then has at most kk - 1 entries before it
        int lo = max(0, kk - nr), hi = min(kk, np);
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (sh_word(ps, pi, mid - 1) > sh_word(rs, ri, kk - mid)) lo = mid; else hi = mid - 1;
        }
        const int a = lo, b = kk - a, steps = min(b, np - a);
        const uint32_t w0 = (uint32_t)row * (uint32_t)k;                    // n_rows * k < 2^31
        uint64_t* wr = words + (size_t)row * (size_t)k;
        for (int t = lane; t < k; t += 64) {         // step t + 1
            uint64_t w = ~0ull;
            if (t < steps) {
                const float c = __fsub_rn(rs[b - 1 - t], ps[a + t]);
                const uint32_t bits = c == 0.f ? 0u : __float_as_uint(c);
                w = ((uint64_t)bits << 32) | (uint64_t)(w0 + (uint32_t)t);
            }
            wr[t] = w;
        }
        if (lane == 0) {
            row_a[row] = a;
            row_kk[row] = kk;
            atomicAdd(&s_sum[0], a);
            atomicAdd(&s_sum[1], steps);
            atomicAdd(&s_sum[2], kk);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&state[0], s_sum[0]);
        atomicAdd(&state[1], s_sum[1]);
        atomicAdd(&state[5], s_sum[2]);
    }
}

// pass p: bins[p][digit] += the words that agree with the digits of the passes before and carry `digit` at this one
__global__ __launch_bounds__(SH_NT) void k_share_hist(size_t n_words, int pass, int64_t want, const uint64_t* __restrict__ words,
                                                      const int32_t* __restrict__ state, const sh_sel* __restrict__ sel, int32_t* __restrict__ bins) {
    __shared__ int s_hist[256];
    if (sh_take(state, want) == 0) return;           // (uniform over the grid)
    const int tid = threadIdx.x, shift = 56 - 8 * pass;
    const uint64_t prefix = sel->prefix, mask = pass == 0 ? 0ull : ~0ull << (shift + 8);
    s_hist[tid] = 0;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * SH_NT;
    for (size_t i = (size_t)blockIdx.x * SH_NT + tid; i < n_words; i += stride) {
        const uint64_t w = words[i];
        if ((w & mask) == prefix) atomicAdd(&s_hist[(int)(w >> shift) & 255], 1);
    }
    __syncthreads();
    const int mine = s_hist[tid];
    if (mine != 0) atomicAdd(&bins[pass * 256 + tid], mine);
}

// one workgroup: the digit of pass p that holds the rank-th smallest word, and the rank left inside it.  The first pass starts from
// rank = take and records it; the last leaves the threshold word in sel->prefix and the bits of its cost in the state.
__global__ __launch_bounds__(256) void k_share_pick(int pass, int64_t want, int32_t* __restrict__ state, sh_sel* __restrict__ sel,
                                                    const int32_t* __restrict__ bins) {
    __shared__ int s_hist[256];
    const int tid = threadIdx.x, shift = 56 - 8 * pass;
    const int take = sh_take(state, want);
    if (take == 0) return;                           // (uniform; state[2] and state[4] stay 0)
    const int rank = pass == 0 ? take : sel->rank;
    const uint64_t prefix = sel->prefix;
    s_hist[tid] = bins[pass * 256 + tid];
    __syncthreads();
    int below = 0;
    for (int d = 0; d < tid; ++d) below += s_hist[d];
    const int mine = s_hist[tid];
    if (below < rank && rank <= below + mine) {      // exactly one thread: the counts of the bins below tid are a partition
        const uint64_t p = prefix | ((uint64_t)tid << shift);
        sel->prefix = p;
        sel->rank = rank - below;
        if (pass == 0) state[2] = take;
        if (pass == SH_PASSES - 1) state[4] = (int32_t)(uint32_t)(p >> 32);
    }
}

__global__ __launch_bounds__(SH_NT) void k_share_finish(int n_rows, int m_in, int k, int64_t want, const float* __restrict__ score_pro,
                                                        const int32_t* __restrict__ id_pro, const float* __restrict__ score_rest,
                                                        const int32_t* __restrict__ id_rest, const uint64_t* __restrict__ words,
                                                        const int32_t* __restrict__ row_a, const int32_t* __restrict__ row_kk,
                                                        const sh_sel* __restrict__ sel, float* __restrict__ score_out, int32_t* __restrict__ id_out,
                                                        int32_t* __restrict__ state) {
    __shared__ int s_changed;
    if (threadIdx.x == 0) s_changed = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, row = blockIdx.x * (SH_NT / 64) + (threadIdx.x >> 6);
    if (row < n_rows) {                              // (whole waves)
        const bool any = sh_take(state, want) > 0;
        const uint64_t thr = sel->prefix;
        const size_t base = (size_t)row * (size_t)m_in, obase = (size_t)row * (size_t)k;
        const float *ps = score_pro + base, *rs = score_rest + base;
        const int32_t *pi = id_pro + base, *ri = id_rest + base;
        int tu = 0;
        if (any) {
            const uint64_t* wr = words + obase;
            for (int t0 = 0; t0 < k; t0 += 64) {
                const int t = t0 + lane;
                const unsigned long long in = __ballot(t < k && wr[t] <= thr);
                tu += (int)__popcll(in);
                if (in != ~0ull) break;              // a row's words increase: past the first one above the threshold there is none at or under it
            }
        }
        const int kk = row_kk[row], a = row_a[row] + tu, b = kk - a;
        for (int e = lane; e < kk; e += 64) {        // entries 0 .. a - 1: promoted, a .. kk - 1: rest
            const bool pro = e < a;
            const int i = pro ? e : e - a;
            const float s = pro ? ps[i] : rs[i];
            const int id = pro ? pi[i] : ri[i];
            const uint64_t w = tk_comp(tk_key(s), id);
            const int pos = i + (pro ? sh_before(rs, ri, b, w) : sh_before(ps, pi, a, w));
            score_out[obase + pos] = s;
            id_out[obase + pos] = id;
        }
        for (int p = kk + lane; p < k; p += 64) {
            score_out[obase + p] = -INFINITY;
            id_out[obase + p] = -1;
        }
        if (lane == 0 && tu > 0) atomicAdd(&s_changed, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_changed != 0) atomicAdd(&state[3], s_changed);
}
