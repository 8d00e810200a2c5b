// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_topk.h): the long-tail report
// (ltg_topk_metrics).  Per user: NDCG@k_ndcg / Recall@k_r1 / Recall@k_r2 of each item group and of all items, read off the user's top-K
// list instead of another scan of the logits, plus the exposure counts item_hits[i] = users whose first k_exp list entries hold item i.
//
// The list is what ltg_topk / ltg_topk_merge wrote (GLOBAL ids in rank order, distinct, padding -1 at the end), so the position of a
// held-out item in it is the rank k_rank_metrics counts, and an item absent from it has rank >= k_in >= every cutoff.  The report
// therefore inherits ltg_topk's limits: n_items per slab <= 360 448, k <= 1 024.
//
// Equality with k_rank_metrics: for rows whose logits are finite and whose fold-in and held-out sets are disjoint, slot n_groups ("all")
// equals ltg_rank_metrics bit for bit and slot g equals ltg_rank_metrics on the held-out CSR filtered to group g: every slot adds its DCG
// terms in double precision in the order of the held-out row (ascending item id), the order rank_finish_row adds them in, and IDCG and the
// divisions are rank_write_row's.  Outside those conditions the two may differ: a held-out item that is also a fold-in item never appears
// in the list (k_rank_metrics ranks it with score -inf), and -inf logits inside the first K are eligible here as in ltg_topk.
//
// Deterministic: item_hits through integer atomicAdd (order-free), no floating-point atomics; the LDS counters of a slot belong to one
// thread.  An id outside [0, n_items_global) is never used as an index (list: not counted; held-out: no group, still in "all").
#pragma once

constexpr int LT_CH = 256;       // held-out entries per pass (Askubuntu's longest held-out row: 384)
constexpr int LT_MAXG = 8;       // item groups; slot n_groups is "all"
constexpr int LT_NOGROUP = 255;

// One workgroup (NT threads, 4 waves) per user.  LDS: the list (k_in ids, <= 4 KB) | the k_ndcg DCG terms (<= 8 KB) | per pass: id, rank,
// label of LT_CH held-out entries.
//   1. stage the list; the first k_exp entries add 1 to item_hits
//   2. per pass of LT_CH held-out entries: stage their ids and labels, wave w looks entries w, w + 4, ... up (64 lanes stride over the
//      list, first match by ballot: at most ceil(k_in / 64) LDS reads per lane and entry; no global load inside that loop), then thread
//      s < n_groups + 1 folds slot s over the pass IN ENTRY ORDER
//   3. thread s writes slot s with rank_write_row's arithmetic (IDCG summed from the same terms in the same order)
__global__ __launch_bounds__(NT) void k_topk_metrics(int k_in, const int32_t* __restrict__ id_in, const int32_t* __restrict__ te_ptr,
                                                     const int32_t* __restrict__ te_idx, const uint8_t* __restrict__ item_group,
                                                     int n_items_global, int n_groups, int k_ndcg, int k_r1, int k_r2, int k_exp,
                                                     float* __restrict__ out, int32_t* __restrict__ item_hits) {
    __shared__ int s_list[1024];
    __shared__ int s_held[LT_CH];
    __shared__ int s_rank[LT_CH];
    __shared__ int s_lab[LT_CH];
    __shared__ double s_term[1024];                      // 1 / log2(r + 2), r < k_ndcg
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int32_t* list = id_in + (size_t)b * k_in;
    for (int j = tid; j < k_in; j += NT) {
        const int id = list[j];
        s_list[j] = id;
        if (item_hits && j < k_exp && id >= 0 && id < n_items_global) atomicAdd(&item_hits[id], 1);
    }
    const int t0 = te_ptr[b], nte = te_ptr[b + 1] - t0;
    // the DCG / IDCG terms, the expression rank_finish_row and rank_write_row add, once per rank and in parallel instead of once per
    // hit and per IDCG step on the slot's one thread (a double-precision log2 and a division each)
    if (nte > 0)
        for (int r = tid; r < k_ndcg; r += NT) s_term[r] = 1.0 / log2((double)r + 2.0);
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};                     // this thread's slot (tid <= n_groups)
    int cnt = 0;                                         // held-out items of the slot
    for (int p0 = 0; p0 < nte; p0 += LT_CH) {
        const int np = min(LT_CH, nte - p0);
        for (int t = tid; t < np; t += NT) {             // the pass's held-out ids and their labels: one coalesced load, one gather
            const int h = te_idx[t0 + p0 + t];
            s_held[t] = h;
            s_lab[t] = h >= 0 && h < n_items_global ? (int)item_group[h] : LT_NOGROUP;
        }
        __syncthreads();
        for (int t = w; t < np; t += NT / 64) {          // (wave-uniform trip count: the ballot below needs every lane)
            const int h = s_held[t];
            int r = INT_MAX;
            for (int j0 = 0; j0 < k_in; j0 += 64) {
                const int j = j0 + lane;
                const unsigned long long m = __ballot(j < k_in && s_list[j] == h);
                if (m != 0ull) {
                    r = j0 + __builtin_ctzll(m);
                    break;
                }
            }
            if (lane == 0) s_rank[t] = h >= 0 ? r : INT_MAX;   // (a negative held-out id must not match the padding)
        }
        __syncthreads();
        if (tid <= n_groups) {
            for (int t = 0; t < np; ++t) {
                if (tid != n_groups && s_lab[t] != tid) continue;
                ++cnt;
                const int r = s_rank[t];
                if (r < k_ndcg) acc[0] += s_term[r];
                if (r < k_r1) acc[1] += 1.0;
                if (r < k_r2) acc[2] += 1.0;
            }
        }
        __syncthreads();
    }
    if (tid <= n_groups) {
        double idcg = 0.0;                               // rank_write_row's sum, in its order
        for (int r = 0; r < min(cnt, k_ndcg); ++r) idcg += s_term[r];
        rank_write_row_idcg(out + ((size_t)b * (n_groups + 1) + tid) * 4, acc, idcg, cnt, k_r1, k_r2);
    }
}
