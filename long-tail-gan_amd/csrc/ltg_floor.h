// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_cap.h, whose index kernels and
// word it uses): exposure-floor top-K lists (ltg_floor_index, ltg_floor_rounds, ltg_floor_finish).  Every item with
// need[item] > 0 reaches need[item] of the served lists if that many users hold it among their candidates and can spare one of the last
// `reserve` slots of their list for it: the item-optimal stable matching of item-proposing deferred acceptance, computed as the greatest
// fixed point of per-user limits.
//
// A candidate entry (row u, position j) is a FLOOR entry iff j lies before the row's first padding id, its id lies in the catalogue and
// need[id] > 0; it carries the cap's word  w = au_comp(s, u),  s = cand_score - lse[u]  (lse == nullptr: the logit).  lim[u] (c - 1 at the
// start; read as k - 1 when reserve = 0) only falls.  A floor entry is ADMISSIBLE iff j <= lim[u]; the ACTIVE entries of an item are its
// need admissible entries with the largest words (all of them if it has no more) -- a function of lim alone, so a round keeps no state
// but lim.  A row with more than reserve active entries at positions >= k - reserve (its zone) lowers lim to the reserve-th of them.
//
// k_floor_lim: lim <- c - 1 (the index is ltg_cap.h's k_cap_zero / k_cap_count / k_cap_scan, sel in the place of thr).
// k_floor_select: one workgroup per item.  It leaves at once, sel = 0, if need < 1 or the segment is no longer than need; else the radix
//   select of ltg_cap.h (cp_select) of the need-th largest word among the ADMISSIBLE entries of its segment.  The first pass's total is
//   the admissible count: at most need, and sel = 0.
// k_floor_users: one wave per row, 64 positions a step up to lim[u]; an entry is active iff it is a floor entry and w >= sel[id]; a
//   ballot / popcount prefix over the zone finds the reserve-th active entry; with more than reserve of them the row stores its new limit.
// k_floor_finish: one wave per row.  The active flags of a row live in registers (one bit per 64-step and lane, c <= 1024).  With m zone
//   entries active, the entry with a of them behind it is served out of place iff j + a >= k, and then at position k - 1 - a: j + a only
//   falls along the zone's entries taken from the back, so those entries are the last t ones, t is the smallest value that leaves at most
//   t active entries at positions >= k - t, and the list is the first k - t live candidates followed by them.  Before convergence a row
//   counts only its first reserve zone entries, as the next round would.
// k_floor_stats: the state block and the held counts.  An id is used as an index only after it has been found inside [0, n_items); an
// entry number only comes out of the index; every position written lies in [0, k).
#pragma once

constexpr int FL_NT = 256;           // 4 waves
constexpr int FL_STATE = 8;          // == LTG_FLOOR_STATE
static_assert(FL_NT == CP_NT, "k_floor_select strides its segment as cp_select does");

__global__ __launch_bounds__(FL_NT) void k_floor_lim(int n_rows, int c, int32_t* __restrict__ lim) {
    const int r = blockIdx.x * FL_NT + threadIdx.x;
    if (r < n_rows) lim[r] = c - 1;
}

// the limit of a row as the rounds read it: never past the row, k - 1 without a reserve
__device__ __forceinline__ int fl_limit(const int32_t* __restrict__ lim, int row, int c, int k, int reserve) {
    return reserve > 0 ? min(lim[row], c - 1) : k - 1;
}

// bump != 0: the first launch of a round (rounds follow one another on the stream: one writer at a time).  held != nullptr: held <- 0.
__global__ __launch_bounds__(FL_NT) void k_floor_select(int c, int k, int reserve, const float* __restrict__ cand_score, const float* __restrict__ lse,
                                                        const int32_t* __restrict__ need, const int32_t* __restrict__ off,
                                                        const int32_t* __restrict__ seg, const int32_t* __restrict__ lim, uint64_t* __restrict__ sel,
                                                        int32_t* __restrict__ held, int32_t* __restrict__ state, int bump) {
    __shared__ int s_hist[256];
    __shared__ int s_sel[3];
    const int tid = threadIdx.x, item = blockIdx.x;
    if (bump && item == 0 && tid == 0) state[1] += 1;
    if (held && tid == 0) held[item] = 0;
    const int e0 = off[item], e1 = off[item + 1], needi = need[item];
    if (needi < 1 || e1 - e0 <= needi) {             // (uniform over the workgroup)
        if (tid == 0) sel[item] = 0ull;
        return;
    }
    uint64_t word;                                   // the needi-th largest admissible word
    if (!cp_select(e0, e1, needi, seg, s_hist, s_sel, word, [&](int ent, uint64_t& w) {
            const int u = ent / c;
            if (ent - u * c > fl_limit(lim, u, c, k, reserve)) return false;
            w = cp_word(cand_score[ent], lse, u);
            return true;
        }))
        word = 0ull;                                 // the admissible count is at or under need: every one is active
    if (tid == 0) sel[item] = word;
}

// is the entry at position j of the row (its id read, `live`: before the first padding id) active under sel?  Admissibility is the caller's.
__device__ __forceinline__ bool fl_active(bool live, int id, float score, const float* __restrict__ lse, int row, const int32_t* __restrict__ need,
                                          int n_items, const uint64_t* __restrict__ sel) {
    return live && id < n_items && need[id] > 0 && cp_word(score, lse, row) >= sel[id];
}

__global__ __launch_bounds__(FL_NT) void k_floor_users(int n_rows, int c, int k, int reserve, const float* __restrict__ cand_score,
                                                       const int32_t* __restrict__ cand_id, const float* __restrict__ lse,
                                                       const int32_t* __restrict__ need, int n_items, const uint64_t* __restrict__ sel,
                                                       int32_t* __restrict__ lim, int32_t* __restrict__ state) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * (FL_NT / 64) + (threadIdx.x >> 6);
    if (row >= n_rows || reserve < 1) return;        // (whole waves; without a reserve nothing past k - 1 is admissible)
    const size_t base = (size_t)row * (size_t)c;
    const int L = fl_limit(lim, row, c, k, reserve), z0 = k - reserve;
    int taken = 0, rth = -1;                         // the active entries of the zone so far, the position of the reserve-th
    for (int j0 = 0; j0 <= L; j0 += 64) {
        const int j = j0 + lane;
        const int id = cp_load_id(cand_id, base, j, c);
        const unsigned long long neg = __ballot(id < 0);
        const bool live = neg == 0ull || lane < (int)__builtin_ctzll(neg);
        bool act = false;
        if (j >= z0 && j <= L && live) act = fl_active(live, id, cand_score[base + j], lse, row, need, n_items, sel);
        const unsigned long long bal = __ballot(act);
        const unsigned long long hit = __ballot(act && taken + (int)__popcll(bal & ((1ull << lane) - 1ull)) == reserve - 1);
        if (hit != 0ull) rth = j0 + (int)__builtin_ctzll(hit);       // the reserve-th active entry lies in this step
        if (taken + (int)__popcll(bal) > reserve) {  // ... and another one behind it, in this step or a later one
            if (lane == 0) {
                lim[row] = rth;
                atomicAdd(&state[0], 1);
                state[4] = state[1];                 // (every wave of a round writes the same number)
            }
            break;
        }
        taken += (int)__popcll(bal);
        if (neg != 0ull) break;
    }
}

__global__ __launch_bounds__(FL_NT) void k_floor_finish(int n_rows, int c, int k, int reserve, const float* __restrict__ cand_score,
                                                        const int32_t* __restrict__ cand_id, const float* __restrict__ lse,
                                                        const int32_t* __restrict__ need, int n_items, const uint64_t* __restrict__ sel,
                                                        const int32_t* __restrict__ lim, float* __restrict__ score_out, int32_t* __restrict__ id_out,
                                                        uint8_t* __restrict__ active_out, int32_t* __restrict__ held, int32_t* __restrict__ row_t) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * (FL_NT / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                       // (whole waves)
    const size_t base = (size_t)row * (size_t)c, obase = (size_t)row * (size_t)k;
    const int L = fl_limit(lim, row, c, k, reserve), z0 = k - reserve;
    const unsigned long long below = (1ull << lane) - 1ull;
    // pass 1: the active flags (bit s of `mine`: position 64 s + lane), the zone's count m, the row's length, the held counts
    uint32_t mine = 0u;
    int m = 0, len = c;
    bool open = true;                                // wave-uniform: the row has not ended
    const int upper = max(L + 1, k);                 // nothing past the limit is active, and the list reads the first k positions
    for (int j0 = 0; j0 < c && (active_out != nullptr || (open && j0 < upper)); j0 += 64) {
        const int j = j0 + lane;
        bool act = false;
        if (open) {
            const int id = cp_load_id(cand_id, base, j, c);
            const unsigned long long neg = __ballot(id < 0);
            const bool live = neg == 0ull || lane < (int)__builtin_ctzll(neg);
            if (j <= L && live) act = fl_active(live, id, cand_score[base + j], lse, row, need, n_items, sel);
            const unsigned long long zbal = __ballot(act && j >= z0);
            if (act && j >= z0 && m + (int)__popcll(zbal & below) >= reserve) act = false;      // (only before convergence)
            m = min(m + (int)__popcll(zbal), reserve);
            if (act) {
                mine |= 1u << (j0 >> 6);
                atomicAdd(&held[id], 1);
            }
            if (neg != 0ull) {
                len = j0 + (int)__builtin_ctzll(neg);
                open = false;
            }
        }
        if (active_out && j < c) active_out[base + j] = act ? 1 : 0;
    }
    // pass 2: the zone's entries that are served out of place, each at k - 1 - (the active entries behind it)
    int t = 0, seen = 0;
    for (int j0 = 0; j0 <= L && m > 0; j0 += 64) {
        const int j = j0 + lane;
        const bool za = ((mine >> (j0 >> 6)) & 1u) != 0u && j >= z0;
        const unsigned long long bal = __ballot(za);
        const int behind = m - (seen + (int)__popcll(bal & below) + 1);
        const bool tail = za && j + behind >= k;
        if (tail) {
            const int p = k - 1 - behind;            // in [k - m, k): m <= reserve <= k
            score_out[obase + p] = cand_score[base + j];
            id_out[obase + p] = cand_id[base + j];
        }
        t += (int)__popcll(__ballot(tail));
        seen += (int)__popcll(bal);
    }
    // pass 3: the first k - t live candidates, and the padding of a row that ends before them
    for (int p = lane; p < k - t; p += 64) {
        const bool have = p < len;
        score_out[obase + p] = have ? cand_score[base + p] : -INFINITY;
        id_out[obase + p] = have ? cand_id[base + p] : -1;
    }
    if (lane == 0) row_t[row] = t;
}

// state[2] = the floor items that hold fewer entries than their floor, [3] = the rows with t > 0, [5] = the sum of t, [6] = the floor
// items, [7] = 0; held_out <- held.  One workgroup; integer sums.
__global__ __launch_bounds__(1024) void k_floor_stats(int n_rows, int n_items, const int32_t* __restrict__ need, const int32_t* __restrict__ held,
                                                      const int32_t* __restrict__ row_t, int32_t* __restrict__ held_out, int32_t* __restrict__ state) {
    __shared__ int s_sum[4];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
    __syncthreads();
    int slots = 0, rows = 0, items = 0, shortf = 0;
    for (int r = threadIdx.x; r < n_rows; r += 1024) {
        const int t = row_t[r];
        slots += t;
        rows += t > 0 ? 1 : 0;
    }
    for (int i = threadIdx.x; i < n_items; i += 1024) {
        const int h = held[i], nd = need[i];
        items += nd > 0 ? 1 : 0;
        shortf += nd > 0 && h < nd ? 1 : 0;
        if (held_out) held_out[i] = h;
    }
    atomicAdd(&s_sum[0], shortf);
    atomicAdd(&s_sum[1], rows);
    atomicAdd(&s_sum[2], slots);
    atomicAdd(&s_sum[3], items);
    __syncthreads();
    if (threadIdx.x == 0) {
        state[2] = s_sum[0];
        state[3] = s_sum[1];
        state[5] = s_sum[2];
        state[6] = s_sum[3];
        state[7] = 0;
    }
}
