// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_audience.h): exposure-capped top-K
// lists (ltg_cap_index, ltg_cap_rounds, ltg_cap_finish).  No item appears in more than cap[item] of the served lists, and the
// slots an over-full item gives up go to the best alternatives of the users it turned away: the user-optimal stable many-to-many matching
// of user-proposing deferred acceptance, computed as the least fixed point of per-item thresholds.
//
// A candidate entry (row u, position j) names item id = cand_id[u][j] and carries the word  w = au_comp(s, u),  s = cand_score - lse[u]
// (lse == nullptr: the logit): the audience order -- score descending, equal scores lower row first.  thr[id] (a word, 0 at the start)
// only rises.  Entry (u, j) is ADMISSIBLE iff id lies in the catalogue, cap[id] > 0 and w >= thr[id]; the ACTIVE entries of a row are its
// first k admissible ones -- a function of thr alone, so a round keeps no state but thr.  An item with more than cap active entries raises
// thr to its cap-th largest active word.  Words of one item are distinct (rows are), so exactly cap entries stay at or above it.
//
// k_cap_count / k_cap_scan / k_cap_scatter: the per-item index, a CSR over entry numbers u * c + j.  Global integer atomics give the counts
//   and the cursors; the order inside a segment depends on scheduling, and everything read from a segment is a sum or a selection by
//   value, so nothing computed depends on it.
// k_cap_propose: one wave per row, 64 entries per step, a ballot / popcount prefix up to the k-th admissible entry, one active byte per
//   entry (zero past the k-th, past the row's end and for ids outside the catalogue).
// k_cap_accept: one workgroup per item.  It leaves at once if the segment cannot exceed the cap; else a radix select (cp_select, shared
//   with ltg_floor.h) over the 64-bit words of the active entries of its segment, most significant digit first, 8 bits a pass: a 256-bin
//   LDS histogram by integer atomics (sums: order-free), the segment re-read per digit -- a head item's segment holds an entry of almost
//   every row and fits no LDS.  The first pass's total is the active count: at most cap, and the workgroup leaves.
// k_cap_finish / k_cap_stats: the lists from the active bytes, every entry with its original logit bit for bit, and the stats block.
// An id is used as an index only after it has been found inside [0, n_items); an entry number only comes out of the index.
#pragma once

constexpr int CP_NT = 256;           // 4 waves
constexpr int CP_STATE = 8;          // == LTG_CAP_STATE: {threshold raises, rounds run, entries passed over, short lists, last round that raised one}

// the id at position j of a row, -1 past its c entries: a wave walks a row 64 positions a step, and the first negative id ends the row
__device__ __forceinline__ int cp_load_id(const int32_t* __restrict__ cand_id, size_t base, int j, int c) { return j < c ? cand_id[base + j] : -1; }

__global__ __launch_bounds__(CP_NT) void k_cap_zero(int n_items, int32_t* __restrict__ cur, int32_t* __restrict__ state) {
    const int i = blockIdx.x * CP_NT + threadIdx.x;
    if (i < n_items) cur[i] = 0;
    if (i < CP_STATE) state[i] = 0;
}

// SCATTER false: cur[id] += 1 per indexed entry.  SCATTER true: seg[off[id] + cur[id]++] = the entry number.
template <bool SCATTER>
__global__ __launch_bounds__(CP_NT) void k_cap_count(int n_rows, int c, const int32_t* __restrict__ cand_id, int n_items, int32_t* __restrict__ cur,
                                                     const int32_t* __restrict__ off, int32_t* __restrict__ seg) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * (CP_NT / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                       // (whole waves)
    const size_t base = (size_t)row * (size_t)c;
    for (int j0 = 0; j0 < c; j0 += 64) {
        const int j = j0 + lane;
        const int id = cp_load_id(cand_id, base, j, c);
        const unsigned long long neg = __ballot(id < 0);
        const bool live = neg == 0ull || lane < (int)__builtin_ctzll(neg);     // before the first padding entry
        if (live && id < n_items) {
            const int p = atomicAdd(&cur[id], 1);
            if (SCATTER) seg[off[id] + p] = (int32_t)(base + j);
        }
        if (neg != 0ull) break;
    }
}

// off[i] = the exclusive prefix sum of cur[0 .. i), off[n_items] = the total; cur <- 0 (the scatter's cursors), thr <- 0.  One workgroup.
__global__ __launch_bounds__(1024) void k_cap_scan(int n_items, int32_t* __restrict__ cur, int32_t* __restrict__ off, uint64_t* __restrict__ thr) {
    __shared__ int s_w[16];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n_items; i0 += 1024) {
        const int i = i0 + tid;
        const int v = i < n_items ? cur[i] : 0;
        int x = v;                                   // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            x += lane >= o ? y : 0;
        }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        int before = s_carry;
        for (int t = 0; t < w; ++t) before += s_w[t];
        if (i < n_items) {
            off[i] = before + x - v;
            cur[i] = 0;
            thr[i] = 0ull;
        }
        __syncthreads();
        if (tid == 1023) s_carry = before + x;
        __syncthreads();
    }
    if (tid == 0) off[n_items] = s_carry;
}

__device__ __forceinline__ uint64_t cp_word(float score, const float* __restrict__ lse, int row) {
    return au_comp(lse ? __fsub_rn(score, lse[row]) : score, row);
}

__global__ __launch_bounds__(CP_NT) void k_cap_propose(int n_rows, int c, int k, const float* __restrict__ cand_score, const int32_t* __restrict__ cand_id,
                                                       const float* __restrict__ lse, const int32_t* __restrict__ cap, int n_items,
                                                       const uint64_t* __restrict__ thr, uint8_t* __restrict__ active, int32_t* __restrict__ state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] += 1;      // (rounds follow one another on the stream: one writer at a time)
    const int lane = threadIdx.x & 63, row = blockIdx.x * (CP_NT / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                       // (whole waves)
    const size_t base = (size_t)row * (size_t)c;
    int taken = 0;
    bool open = true;                                // wave-uniform: the row has not ended and still wants entries
    for (int j0 = 0; j0 < c; j0 += 64) {
        const int j = j0 + lane;
        bool act = false;
        if (open) {
            const int id = cp_load_id(cand_id, base, j, c);
            const unsigned long long neg = __ballot(id < 0);
            const bool live = neg == 0ull || lane < (int)__builtin_ctzll(neg);
            bool adm = false;
            if (live && id < n_items && cap[id] > 0) adm = cp_word(cand_score[base + j], lse, row) >= thr[id];
            const unsigned long long bal = __ballot(adm);
            act = adm && taken + (int)__popcll(bal & ((1ull << lane) - 1ull)) < k;
            taken += (int)__popcll(bal);
            open = neg == 0ull && taken < k;
        }
        if (j < c) active[base + j] = act ? 1 : 0;
    }
}

// The radix select of k_cap_accept and k_floor_select: the rank-th largest 64-bit word among the entries seg[e0 .. e1) that `word_of`
// counts, most significant digit first, 8 bits a pass, the segment re-read per digit.  word_of(entry number, w&) -> the entry counts, and
// then w is its word.  The first pass's total is the number of entries that count: with at most `rank` of them -> false, at once; else
// -> true with `out` = the selected word.  Both are uniform over the workgroup: all CP_NT threads call it, with s_hist[256] and s_sel[3]
// (the digit chosen, the rank left inside it, leave) in LDS.
template <typename F>
__device__ __forceinline__ bool cp_select(int e0, int e1, int rank, const int32_t* __restrict__ seg, int* s_hist, int* s_sel, uint64_t& out,
                                          F word_of) {
    const int tid = threadIdx.x;
    uint64_t prefix = 0ull, mask = 0ull;             // the rank-th largest of the counting words that agree with prefix under mask
#pragma unroll 1
    for (int shift = 56; shift >= 0; shift -= 8) {
        s_hist[tid] = 0;
        __syncthreads();
        for (int e = e0 + tid; e < e1; e += CP_NT) {
            uint64_t w;
            if (!word_of(seg[e], w)) continue;
            if ((w & mask) == prefix) atomicAdd(&s_hist[(int)(w >> shift) & 255], 1);
        }
        __syncthreads();
        int above = 0;
        for (int b = 255; b > tid; --b) above += s_hist[b];
        const int mine = s_hist[tid];
        if (shift == 56 && tid == 0) s_sel[2] = above + mine > rank ? 0 : 1;       // (rank is still the caller's: the count is at or under it)
        __syncthreads();
        if (shift == 56 && s_sel[2] != 0) return false;
        if (above < rank && rank <= above + mine) {  // exactly one thread: the counts of the bins above tid are a partition
            s_sel[0] = tid;
            s_sel[1] = rank - above;
        }
        __syncthreads();
        prefix |= (uint64_t)s_sel[0] << shift;
        mask |= 255ull << shift;
        rank = s_sel[1];
        __syncthreads();                             // (everyone has read the choice before the next pass clears the bins)
    }
    out = prefix;
    return true;
}

__global__ __launch_bounds__(CP_NT) void k_cap_accept(int c, const float* __restrict__ cand_score, const float* __restrict__ lse,
                                                      const int32_t* __restrict__ cap, const int32_t* __restrict__ off, const int32_t* __restrict__ seg,
                                                      const uint8_t* __restrict__ active, uint64_t* __restrict__ thr, int32_t* __restrict__ state) {
    __shared__ int s_hist[256];
    __shared__ int s_sel[3];
    const int tid = threadIdx.x, item = blockIdx.x;
    const int e0 = off[item], e1 = off[item + 1], capi = cap[item];
    if (capi < 1 || e1 - e0 <= capi) return;         // (uniform over the workgroup)
    uint64_t word;                                   // the capi-th largest active word; nothing to do with the active count at or under the cap
    if (!cp_select(e0, e1, capi, seg, s_hist, s_sel, word, [&](int ent, uint64_t& w) {
            if (!active[ent]) return false;
            w = cp_word(cand_score[ent], lse, ent / c);
            return true;
        }))
        return;
    if (tid == 0 && thr[item] != word) {
        thr[item] = word;
        atomicAdd(&state[0], 1);
        state[4] = state[1];                         // (every workgroup of a round writes the same number)
    }
}

// the lists: the active entries of a row in candidate order.  row_over[row] = the entries the row's walk passed over: catalogue entries
// before its k-th active one (all of them when the list is short) that are not active.
__global__ __launch_bounds__(CP_NT) void k_cap_finish(int n_rows, int c, int k, const float* __restrict__ cand_score, const int32_t* __restrict__ cand_id,
                                                      int n_items, const uint8_t* __restrict__ active, float* __restrict__ score_out,
                                                      int32_t* __restrict__ id_out, int32_t* __restrict__ row_over) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * (CP_NT / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                       // (whole waves)
    const size_t base = (size_t)row * (size_t)c, obase = (size_t)row * (size_t)k;
    int taken = 0, over = 0;
    for (int j0 = 0; j0 < c && taken < k; j0 += 64) {
        const int j = j0 + lane;
        const int id = cp_load_id(cand_id, base, j, c);
        const unsigned long long neg = __ballot(id < 0);
        const bool live = neg == 0ull || lane < (int)__builtin_ctzll(neg);
        const bool act = live && id < n_items && active[base + j] != 0;
        const unsigned long long bal = __ballot(act);
        const int pos = taken + (int)__popcll(bal & ((1ull << lane) - 1ull));
        if (act && pos < k) {
            score_out[obase + pos] = cand_score[base + j];
            id_out[obase + pos] = id;
        }
        const unsigned long long last = __ballot(act && pos == k - 1);            // the k-th active entry, if this step holds it
        const int stop = last != 0ull ? (int)__builtin_ctzll(last) : 64;
        over += (int)__popcll(__ballot(live && id < n_items && !act && lane < stop));
        taken += (int)__popcll(bal);
        if (neg != 0ull) break;
    }
    taken = min(taken, k);
    for (int p = taken + lane; p < k; p += 64) {
        score_out[obase + p] = -INFINITY;
        id_out[obase + p] = -1;
    }
    if (lane == 0) row_over[row] = over;
}

// state[2] = the sum of row_over, state[3] = the rows whose list is short.  One workgroup; integer sums.
__global__ __launch_bounds__(1024) void k_cap_stats(int n_rows, int k, const int32_t* __restrict__ id_out, const int32_t* __restrict__ row_over,
                                                    int32_t* __restrict__ state) {
    __shared__ int s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    int over = 0, shortl = 0;
    for (int r = threadIdx.x; r < n_rows; r += 1024) {
        over += row_over[r];
        shortl += id_out[(size_t)r * (size_t)k + (k - 1)] < 0 ? 1 : 0;
    }
    atomicAdd(&s_sum[0], over);
    atomicAdd(&s_sum[1], shortl);
    __syncthreads();
    if (threadIdx.x == 0) {
        state[2] = s_sum[0];
        state[3] = s_sum[1];
    }
}
