// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_topk.h): item audiences -- the k
// likeliest rows (users) of a chunk of the row-major logits for every query COLUMN (ltg_item_audience = k_item_audience + k_topk_merge
// over the row segments).
//
// Score of (row, column) = logit - lse[row] (one fp32 subtraction; lse == nullptr: the logit).  Row r is eligible for query column c iff c
// is not in r's fold-in list.  Order: score descending, equal scores lower row first, -0.0 == +0.0 (tk_key), padding id -1 / score -inf:
// ltg_topk's format with "id" = row_lo + row, so the lists go straight into ltg_topk_merge.
// Deterministic and exact: the only atomics are LDS integer counters; what they order is sorted by a total order afterwards, and the SET
// a column keeps does not depend on the order (the threshold below is a lower bound of the k-th best word, and words are distinct).
#pragma once

constexpr int AU_NT = 256;      // 4 waves
constexpr int AU_ROWS = 128;    // rows per workgroup step: a column gets at most this many new candidates between two looks at its count

// (key, row, was the score -0.0) as one 64-bit word: descending order of the word == score descending, then row ascending.  Rows are
// distinct within a column, so the flag in bit 0 never decides an order; it only restores the sign of a zero that tk_key dropped.
// 0 == no entry (every key of a non-NaN float is > 0).
__device__ __forceinline__ uint64_t au_comp(float score, int gid) {
    const uint32_t nz = __float_as_uint(score) == 0x80000000u ? 1u : 0u;
    return ((uint64_t)tk_key(score) << 32) | (uint64_t)(((0x7FFFFFFFu - (uint32_t)gid) << 1) | nz);
}
__device__ __forceinline__ int au_id(uint64_t c) { return (int)(0x7FFFFFFFu - ((uint32_t)c >> 1)); }
__device__ __forceinline__ float au_score(uint64_t c) {
    const uint32_t key = (uint32_t)(c >> 32);
    return ((uint32_t)c & 1u) ? -0.f : __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// entries past a column's count -> 0 (no entry), then a bitonic sort, descending, of every column's buffer [CAP] of buf [C][CAP] at once
// (CAP a power of two).  only_over >= 0: columns holding at most that many entries are left alone.  Ends with a barrier.
template <int C, int CAP>
__device__ __forceinline__ void au_pad_sort(uint64_t* buf, const int* cnt, int only_over) {
    for (int e = threadIdx.x; e < C * CAP; e += AU_NT)
        if ((e & (CAP - 1)) >= cnt[e / CAP]) buf[e] = 0ull;
    __syncthreads();
    for (int size = 2; size <= CAP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < C * CAP / 2; i += AU_NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                if (cnt[lo / CAP] <= only_over) continue;
                const bool desc = ((lo & (CAP - 1)) & size) == 0;
                const uint64_t a = buf[lo], b = buf[hi];
                if ((a < b) == desc) {
                    buf[lo] = b;
                    buf[hi] = a;
                }
            }
            __syncthreads();
        }
    }
}

// Workgroup (x, y) = query columns q_col[C x .. C x + C) against the rows [y seg_len, (y + 1) seg_len) of the chunk (seg_len % AU_ROWS == 0).
// Lanes are laid out with the columns fastest: thread t holds column t % C and, per step of AU_ROWS rows, the rows t / C + u (AU_NT / C),
// u = 0 .. U - 1 -- a wave's request for one row is C consecutive q_col entries, C x 4 contiguous bytes when those are consecutive columns,
// and the logits are read exactly once.  Every score becomes its word (au_comp) -- 0 if the row is past the segment's end or holds the
// column in its fold-in list -- and is compared with the column's threshold; a survivor is appended to the column's buffer [CAP] in LDS.
// thr = 0 until the column has been cut to k entries, then its k-th best word: always a true lower bound of the k-th best of everything
// the column has seen, and words are distinct, so `>` loses nothing.  A step appends at most AU_ROWS words per column; after every step
// (barrier), if any column holds more than CAP - AU_ROWS, the columns holding more than k are sorted and cut to their k best
// (k <= CAP - AU_ROWS).  Counts are sums, so this decision, the kept sets and every later threshold are independent of the order in which
// the waves appended.  At the end every column is sorted and written as a list: [segment][n_q][k].
// Fold-in marks: per step, thread r < AU_ROWS owns row r's word of s_mark (bit j = the row holds column j of the block).  The row's
// fold-in list is ascending, so the entries that can matter lie in [cmin, cmax] = the block's column range: a bisection for cmin, then a
// walk up to cmax.  A block of consecutive ascending columns (dense) turns an entry into its bit directly; any other block compares the
// entry with its C columns, which also gives duplicate query columns identical lists.  The logits are never modified.
template <int C, int CAP>
__global__ __launch_bounds__(AU_NT) void k_item_audience(int I, int n_rows, int row_lo, int n_q, int seg_len, int k, const float* __restrict__ logits,
                                                         const float* __restrict__ lse, const int32_t* __restrict__ tr_ptr,
                                                         const int32_t* __restrict__ tr_idx, const int32_t* __restrict__ q_col,
                                                         float* __restrict__ score_out, int32_t* __restrict__ id_out) {
    constexpr int RPP = AU_NT / C, U = AU_ROWS / RPP;      // rows per pass of the workgroup, passes per step
    static_assert(C <= 32 && AU_NT % C == 0 && AU_ROWS % RPP == 0 && CAP > AU_ROWS, "tile shape");
    extern __shared__ __attribute__((aligned(16))) uint64_t au_buf[];      // [C][CAP]
    __shared__ uint64_t s_thr[C];
    __shared__ int s_cnt[C];
    __shared__ int s_col[C];
    __shared__ uint32_t s_mark[AU_ROWS];
    __shared__ int s_range[3];                                             // cmin, cmax, dense
    uint64_t* buf = au_buf;
    const int tid = threadIdx.x, lane = tid & 63, j = tid % C, rr = tid / C;
    const int p0 = blockIdx.x * C, seg_lo = blockIdx.y * seg_len;      // (y < ceil(n_rows / seg_len): seg_lo < n_rows)
    const int seg_hi = (int)min((long long)n_rows, (long long)seg_lo + seg_len);
    if (tid < C) {                               // columns past n_q mirror the last query (their lists are not written)
        s_col[tid] = min(max(q_col[min(p0 + tid, n_q - 1)], 0), I - 1);    // (clamped: a bad column never becomes an address out of bounds)
        s_thr[tid] = 0ull;
        s_cnt[tid] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        int lo = s_col[0], hi = s_col[0], dense = 1;
        for (int t = 1; t < C; ++t) {
            lo = min(lo, s_col[t]);
            hi = max(hi, s_col[t]);
            dense &= s_col[t] == s_col[0] + t ? 1 : 0;
        }
        s_range[0] = lo;
        s_range[1] = hi;
        s_range[2] = dense;
    }
    __syncthreads();
    const int col = s_col[j], cmin = s_range[0], cmax = s_range[1];
    const bool dense = s_range[2] != 0;
    const float* lcol = logits + col;
#pragma unroll 1
    for (int r0 = seg_lo; r0 < seg_hi; r0 += AU_ROWS) {
        float x[U], l[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {            // U loads in flight per thread; rows past the end re-read the last row
            const int r = min(r0 + u * RPP + rr, n_rows - 1);
            x[u] = lcol[(size_t)r * (size_t)I];
            l[u] = lse ? lse[r] : 0.f;
        }
        if (tr_ptr && tid < AU_ROWS) {
            const int r = r0 + tid;
            uint32_t m = 0u;
            if (r < seg_hi) {
                const int b = tr_ptr[r + 1];
                int lo = tr_ptr[r], hi = b;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (tr_idx[mid] < cmin) lo = mid + 1; else hi = mid;
                }
                for (int e = lo; e < b; ++e) {
                    const int it = tr_idx[e];
                    if (it > cmax) break;
                    if (it < cmin) continue;     // (only a list that is not ascending gets here)
                    if (dense) {
                        m |= 1u << (it - cmin);
                    } else {
                        for (int t = 0; t < C; ++t) m |= s_col[t] == it ? 1u << t : 0u;
                    }
                }
            }
            s_mark[tid] = m;
        }
        __syncthreads();     // the marks are written; every wave has read the counts the last step left before they move again
        const uint64_t thr = s_thr[j];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rl = u * RPP + rr, r = r0 + rl;
            const bool ok = r < seg_hi && !(tr_ptr && ((s_mark[rl] >> j) & 1u));
            const float s = lse ? __fsub_rn(x[u], l[u]) : x[u];
            const uint64_t c = ok ? au_comp(s, row_lo + r) : 0ull;
            if (c > thr) buf[j * CAP + atomicAdd(&s_cnt[j], 1)] = c;
        }
        __syncthreads();
        if (__ballot(s_cnt[lane & (C - 1)] > CAP - AU_ROWS) != 0ull) {      // (the same counts in every wave: uniform over the workgroup)
            au_pad_sort<C, CAP>(buf, s_cnt, k);
            if (tid < C && s_cnt[tid] > k) {
                s_cnt[tid] = k;
                s_thr[tid] = buf[tid * CAP + k - 1];
            }
            __syncthreads();
        }
    }
    au_pad_sort<C, CAP>(buf, s_cnt, -1);
    const size_t seg = (size_t)blockIdx.y * (size_t)n_q;
    for (int e = tid; e < C * k; e += AU_NT) {
        const int t = e / k, i = e - t * k, p = p0 + t;
        if (p >= n_q) continue;
        const uint64_t c = buf[t * CAP + i];
        const size_t o = (seg + p) * (size_t)k + i;
        id_out[o] = c != 0ull ? au_id(c) : -1;
        score_out[o] = c != 0ull ? au_score(c) : -INFINITY;
    }
}
