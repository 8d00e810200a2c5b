// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_sampler.h): exact masked top-K
// per row of the logits (ltg_topk; restricted to admitted item groups: ltg_topk_groups), the merge of per-slab top-K lists (ltg_topk_merge)
// and the composition of a list with a minimum of slots per group from such lists (ltg_topk_quota).
//
// Order: score descending, equal scores lower GLOBAL id first -- the rule k_rank_metrics ranks by, so Recall@k computed from the ids
// equals ltg_rank_metrics'.  -0.0 == +0.0 (the key canonicalises -0.0).  Fold-in items never appear; every other item is eligible,
// -inf included.  A row with fewer than k eligible items is padded with id -1 / score -inf.  NaN logits are outside the contract.
// Deterministic: the only atomics are LDS integer counters whose results are sorted by a total order afterwards.
#pragma once

constexpr int TK_NT = 1024;   // 16 waves: one per-thread maximum per thread is what the first threshold is chosen from (k <= 1024)

// order-preserving 32-bit key of a float: larger key == larger float; -0.0 -> +0.0; 0 is below every non-NaN key (-inf -> 0x007FFFFF)
__device__ __forceinline__ uint32_t tk_key(float x) {
    uint32_t u = __float_as_uint(x);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// (key, global id) as one 64-bit word: descending order of the word == score descending, then id ascending.  0 == no entry.
__device__ __forceinline__ uint64_t tk_comp(uint32_t key, int gid) { return ((uint64_t)key << 32) | (uint64_t)(~(uint32_t)gid); }

// bitonic sort, descending, of n words in LDS (n a power of two).  Ends with a barrier.
__device__ __forceinline__ void tk_sort_desc(uint64_t* buf, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (n >> 1); i += TK_NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
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

// the 4 items 4j .. 4j+3 of a row: values and fold-in flags (bit t of the nibble).  VEC: 16-byte load (I % 4 == 0, aligned rows)
template <bool VEC>
__device__ __forceinline__ void tk_load4(const float* row, int I, const unsigned* bits, int j, float (&v)[4], unsigned& fold) {
    const int i0 = 4 * j;
    if (VEC) {
        const ltg_f32x4 x = reinterpret_cast<const ltg_f32x4*>(row)[j];
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = i0 + t < I ? row[i0 + t] : 0.f;
    }
    fold = (bits[j >> 3] >> ((j & 7) * 4)) & 15u;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (i0 + t >= I) fold |= 1u << t;       // past the end: treated like a fold-in item
}

// One workgroup per row.  LDS: bitset of the items that are not eligible (ceil(I/32) words) | buf (cap 64-bit words).
// GRP (ltg_topk_groups): an item whose label's bit is not in group_mask is not eligible either.  labels = the slab's part of the uint8 array
// (label of column i at labels[i]); bit min(label, 8) of group_mask admits it.  Every row's workgroup reads the labels itself (I bytes,
// from the L2 after the first rows): no workspace, no second launch, and the passes below do not know about groups (n_elig falls out
// of the popcount).  Without GRP the two arguments are not read.
//   pass 1  per-thread maximum key of the eligible items; T0 = the k-th largest of the TK_NT maxima (bitonic sort of TK_NT words):
//           at least k eligible items have key >= T0, so the k-th largest key of the row is >= T0
//   pass 2  every eligible item with key >= T0 into buf (LDS counter); if they fit (<= cap): sort them, write the first k
//   else    (many equal keys or a flat row, large k) exact radix select of the k-th key Tk over 4 digits of 8 bits (one row pass each),
//           then one pass that keeps every key > Tk (< k of them) and the first (k - #above) items with key == Tk in id order (a block
//           scan per tile), sort, write.
template <bool VEC, bool GRP>
__global__ __launch_bounds__(TK_NT) void k_topk(int I, int item_lo, const float* __restrict__ logits, const int32_t* __restrict__ tr_ptr,
                                                 const int32_t* __restrict__ tr_idx, int k, int cap, float* __restrict__ score_out,
                                                 int32_t* __restrict__ id_out, const uint8_t* __restrict__ labels, uint32_t group_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];
    __shared__ int s_hist[256];
    __shared__ int s_wsum[TK_NT / 64];
    __shared__ int s_cnt, s_kk;
    __shared__ uint32_t s_prefix;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nw = (I + 31) >> 5;
    unsigned* s_bits = s_dyn;
    uint64_t* buf = reinterpret_cast<uint64_t*>(s_dyn + ((nw + 1) & ~1));
    for (int i = tid; i < nw; i += TK_NT) s_bits[i] = 0u;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if (tr_ptr) {
        for (int e = tr_ptr[b] + tid; e < tr_ptr[b + 1]; e += TK_NT) {
            const int it = tr_idx[e];
            if (it >= 0 && it < I) atomicOr(&s_bits[it >> 5], 1u << (it & 31));
        }
    }
    __syncthreads();
    if (GRP) {
        if ((reinterpret_cast<uintptr_t>(labels) & 15) == 0) {      // (item_lo = 0, or a slab cut at a multiple of 16)
            const int n_full = I >> 5;                   // bitset words whose 32 labels all exist: two 16-byte loads per thread and word
            for (int i = tid; i < n_full; i += TK_NT) {
                const uint4 a = reinterpret_cast<const uint4*>(labels)[2 * i], c = reinterpret_cast<const uint4*>(labels)[2 * i + 1];
                const unsigned wd[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
                unsigned out = 0u;
#pragma unroll
                for (int t = 0; t < 32; ++t) out |= (((group_mask >> min((wd[t >> 2] >> ((t & 3) * 8)) & 255u, 8u)) & 1u) ^ 1u) << t;
                s_bits[i] |= out;
            }
            if (tid < (I & 31) && !((group_mask >> min((unsigned)labels[32 * n_full + tid], 8u)) & 1u)) atomicOr(&s_bits[n_full], 1u << tid);
        } else {                                         // any alignment: one byte per lane, a wave's ballot is the word pair 2q, 2q + 1
            const int n64 = (I + 63) >> 6;
            for (int q0 = w; q0 < n64; q0 += 4 * (TK_NT / 64)) {   // four byte loads in flight per lane
                unsigned lab[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int it = (q0 + u * (TK_NT / 64)) * 64 + lane;
                    lab[u] = it < I ? labels[it] : 0xFFFFFFFFu;    // past the end: no bit here (tk_load4 treats those columns)
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + u * (TK_NT / 64);
                    const unsigned long long out = __ballot(lab[u] != 0xFFFFFFFFu && !((group_mask >> min(lab[u], 8u)) & 1u));
                    if (lane == 0 && q < n64) {                    // (the pair belongs to this wave alone: plain read-modify-write)
                        s_bits[2 * q] |= (unsigned)out;
                        if (2 * q + 1 < nw) s_bits[2 * q + 1] |= (unsigned)(out >> 32);
                    }
                }
            }
        }
        __syncthreads();
    }
    int nf = 0;                                          // items of the row that are not eligible (fold-in duplicates counted once)
    for (int i = tid; i < nw; i += TK_NT) nf += __popc(s_bits[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o);
    if (lane == 0) s_wsum[w] = nf;
    __syncthreads();
    int n_fold = 0;
#pragma unroll
    for (int q = 0; q < TK_NT / 64; ++q) n_fold += s_wsum[q];
    __syncthreads();
    const float* row = logits + (size_t)b * I;
    const int n4 = (I + 3) >> 2;
    const int n_elig = I - n_fold;
    float* so = score_out + (size_t)b * k;
    int32_t* io = id_out + (size_t)b * k;

    // ---- pass 1: per-thread maximum, four 16-byte loads in flight per thread
    uint32_t mx = 0u;
    for (int j0 = 0; j0 < n4; j0 += 4 * TK_NT) {
        float v[4][4];
        unsigned f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * TK_NT + tid;
            f[u] = 15u;
            if (j < n4) tk_load4<VEC>(row, I, s_bits, j, v[u], f[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (!((f[u] >> t) & 1u)) mx = max(mx, tk_key(v[u][t]));
    }
    buf[tid] = (uint64_t)mx << 32;
    __syncthreads();
    tk_sort_desc(buf, TK_NT);
    const uint32_t t0 = (uint32_t)(buf[k - 1] >> 32);      // 0 when fewer than k threads saw an eligible item: every eligible item qualifies
    __syncthreads();

    // ---- pass 2: candidates key >= T0 (one LDS atomic per wave per 4-item step that has any)
    for (int j0 = 0; j0 < n4; j0 += TK_NT) {            // (uniform trip count: the wave scan below needs every lane)
        const int j = j0 + tid;
        float v[4];
        unsigned f = 15u;
        if (j < n4) tk_load4<VEC>(row, I, s_bits, j, v, f);
        uint64_t c[4];
        int nc = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t key = ((f >> t) & 1u) ? 0u : tk_key(v[t]);
            c[t] = key >= t0 && key != 0u ? tk_comp(key, item_lo + 4 * j + t) : 0ull;
            nc += c[t] != 0ull ? 1 : 0;
        }
        if (__ballot(nc > 0) == 0ull) continue;          // (the common case: nothing of this wave's 256 items qualifies)
        int incl = nc;                                   // wave inclusive scan of the per-lane counts
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const int tot = __shfl(incl, 63);
        int base = 0;
        if (tot > 0) {
            if (lane == 63) base = atomicAdd(&s_cnt, tot);
            base = __shfl(base, 63);
            int p = base + incl - nc;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (c[t] != 0ull) {
                    if (p < cap) buf[p] = c[t];
                    ++p;
                }
        }
    }
    __syncthreads();
    const int n_cand = s_cnt;
    int n_sorted;
    if (n_cand <= cap) {
        n_sorted = n_cand;
    } else {
        // ---- exact radix select of the k-th largest key Tk among the eligible items (all of them have key >= T0)
        uint32_t prefix = 0u;
        int kk = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            const uint32_t hmask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < 256; i += TK_NT) s_hist[i] = 0;
            __syncthreads();
            for (int j = tid; j < n4; j += TK_NT) {
                float v[4];
                unsigned f;
                tk_load4<VEC>(row, I, s_bits, j, v, f);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t key = tk_key(v[t]);
                    if (!((f >> t) & 1u) && key >= t0 && (key & hmask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
                }
            }
            __syncthreads();
            if (w == 0) {                                // lane l holds digits 255-4l .. 252-4l (descending)
                int h[4], s = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) { h[t] = s_hist[255 - 4 * lane - t]; s += h[t]; }
                int incl = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(incl, o);
                    if (lane >= o) incl += y;
                }
                const int excl = incl - s;               // items in higher digits than this lane's
                const unsigned long long hit = __ballot(excl < kk && incl >= kk);
                const int src = __builtin_ctzll(hit);
                if (lane == src) {
                    int above = excl, d = 255 - 4 * lane;
                    for (int t = 0; t < 4; ++t, --d) {
                        if (above + h[t] >= kk) break;
                        above += h[t];
                    }
                    s_prefix = prefix | ((uint32_t)d << shift);
                    s_kk = kk - above;                // items still to take inside the chosen digit
                }
            }
            __syncthreads();
            prefix = s_prefix;
            kk = s_kk;
            __syncthreads();
        }
        // ---- keys > Tk (fewer than k) by LDS counter; keys == Tk: the first kk in id order (block scan per tile)
        const uint32_t tk = prefix;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        const int eq0 = k - kk;                          // slots [0, k-kk) for the keys above, [k-kk, k) for the equal ones
        int run = 0;
        for (int j0 = 0; j0 < n4; j0 += TK_NT) {
            const int j = j0 + tid;
            float v[4];
            unsigned f = 15u;
            if (j < n4) tk_load4<VEC>(row, I, s_bits, j, v, f);
            int ne = 0;
            uint32_t key[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                key[t] = ((f >> t) & 1u) ? 0u : tk_key(v[t]);
                if (key[t] > tk) {
                    const int p = atomicAdd(&s_cnt, 1);
                    if (p < cap) buf[p] = tk_comp(key[t], item_lo + 4 * j + t);
                }
                ne += key[t] == tk ? 1 : 0;
            }
            int incl = ne;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (lane == 63) s_wsum[w] = incl;
            __syncthreads();
            int before = run, total = run;
#pragma unroll
            for (int q = 0; q < TK_NT / 64; ++q) {
                before += q < w ? s_wsum[q] : 0;
                total += s_wsum[q];
            }
            int p = before + incl - ne;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (key[t] == tk) {
                    if (p < kk) buf[eq0 + p] = tk_comp(tk, item_lo + 4 * j + t);
                    ++p;
                }
            run = total;
            __syncthreads();
        }
        n_sorted = k;
    }
    int n_pow = 2;
    while (n_pow < n_sorted) n_pow <<= 1;
    for (int i = n_sorted + tid; i < n_pow; i += TK_NT) buf[i] = 0ull;
    __syncthreads();
    tk_sort_desc(buf, n_pow);
    const int n_out = min(k, n_elig);
    for (int i = tid; i < k; i += TK_NT) {
        if (i < n_out && buf[i] != 0ull) {
            const int gid = (int)~(uint32_t)buf[i];
            io[i] = gid;
            so[i] = row[gid - item_lo];
        } else {
            io[i] = -1;
            so[i] = -INFINITY;
        }
    }
}

// Merge of n_parts lists per row, each sorted as k_topk writes it (padding id -1 at the end) over DISJOINT item sets: the rank of an
// entry in the union = its position in its own list + the entries of every other list that precede it (binary search).  No LDS.
__device__ __forceinline__ uint64_t tk_comp_at(const float* s, const int32_t* id, int i) {
    const int g = id[i];
    return g < 0 ? 0ull : tk_comp(tk_key(s[i]), g);
}
// #{i < n : entry i > c} of a list sorted as k_topk writes it (descending words, padding == 0 at the end)
__device__ __forceinline__ int tk_count_above(const float* s, const int32_t* id, int n, uint64_t c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tk_comp_at(s, id, mid) > c) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(NT) void k_topk_merge(int n_parts, int n_rows, int k_in, const float* __restrict__ score_in,
                                                   const int32_t* __restrict__ id_in, int k, float* __restrict__ score_out,
                                                   int32_t* __restrict__ id_out) {
    __shared__ int s_valid;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t part = (size_t)n_rows * k_in;
    const int n = n_parts * k_in;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    int nv = 0;
    for (int e = tid; e < n; e += NT) nv += id_in[(size_t)(e / k_in) * part + (size_t)b * k_in + (e % k_in)] >= 0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o);
    if ((tid & 63) == 0) atomicAdd(&s_valid, nv);
    __syncthreads();
    const int n_valid = s_valid;
    float* so = score_out + (size_t)b * k;
    int32_t* io = id_out + (size_t)b * k;
    for (int i = n_valid + tid; i < k; i += NT) {
        io[i] = -1;
        so[i] = -INFINITY;
    }
    for (int e = tid; e < n; e += NT) {
        const int p = e / k_in, j = e % k_in;
        const float* sp = score_in + p * part + (size_t)b * k_in;
        const int32_t* ip = id_in + p * part + (size_t)b * k_in;
        const uint64_t c = tk_comp_at(sp, ip, j);
        if (c == 0ull || j >= k) continue;
        int rank = j;
        for (int q = 0; q < n_parts && rank < k; ++q) {
            if (q == p) continue;
            const float* sq = score_in + q * part + (size_t)b * k_in;
            const int32_t* iq = id_in + q * part + (size_t)b * k_in;
            int lo = 0, hi = k_in;                       // #{i : comp(q, i) > c}: the list is descending
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tk_comp_at(sq, iq, mid) > c) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            io[rank] = ip[j];
            so[rank] = sp[j];
        }
    }
}

// Minimum slots per group, composed from lists (ltg_topk_quota).  Per row: all = the plain list [k_in]; grp = n_lists reserved
// lists [m_in], pairwise disjoint, all sorted and padded as k_topk writes them; u_j = the entries of list j among its first quota[j] that
// are not padding.  U = those entries; S = U + the first (k - |U|) entries of `all` that are not in U.  No sort: the rank of an entry in S is
// its position in its own sequence plus the entries of every other sequence that precede it, each a binary search -- a plain entry's
// searches of the reserved lists also say whether it is a member of U (the entry found equals it).  The kept non-members are a prefix of the
// non-members of `all`, so "kept non-members before c" = min(non-members among the first lo entries of `all`, k - |U|) with the exclusive
// scan s_nm of the non-member flags.  One thread per plain entry (k_in <= TK_NT; the block is k_in rounded up to whole waves).  Scores and
// ids are copied, ids never index anything.
struct tk_quota { int32_t q[8]; };
__global__ __launch_bounds__(TK_NT) void k_topk_quota(int n_rows, int k_in, const float* __restrict__ score_all, const int32_t* __restrict__ id_all,
                                                       int n_lists, int m_in, const float* __restrict__ score_grp,
                                                       const int32_t* __restrict__ id_grp, tk_quota quota, int k, float* __restrict__ score_out,
                                                       int32_t* __restrict__ id_out) {
    __shared__ int s_nm[TK_NT + 1];
    __shared__ int s_wsum[TK_NT / 64];
    __shared__ int s_u[8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nt = blockDim.x;                           // k_in rounded up to whole waves (the host's choice): a thread per plain entry
    const float* sa = score_all + (size_t)b * k_in;
    const int32_t* ia = id_all + (size_t)b * k_in;
    const size_t part = (size_t)n_rows * m_in, row = (size_t)b * m_in;
    if (tid < n_lists) {                                 // padding is at the end of a list: u_j by bisection
        int q = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) q = j == tid ? quota.q[j] : q;
        const int32_t* ig = id_grp + tid * part + row;
        int lo = 0, hi = q;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ig[mid] >= 0) lo = mid + 1; else hi = mid;
        }
        s_u[tid] = lo;
    }
    __syncthreads();
    int n_u = 0;
    for (int j = 0; j < n_lists; ++j) n_u += s_u[j];
    const int n_free = k - n_u;
    // ---- the plain entry of this thread: entries of U before it, and is it one of them
    const uint64_t c = tid < k_in ? tk_comp_at(sa, ia, tid) : 0ull;
    int ahead = 0;
    bool member = false;
    if (c != 0ull) {
        for (int j = 0; j < n_lists; ++j) {
            const float* sg = score_grp + j * part + row;
            const int32_t* ig = id_grp + j * part + row;
            const int uj = s_u[j], lo = tk_count_above(sg, ig, uj, c);
            ahead += lo;
            member = member || (lo < uj && tk_comp_at(sg, ig, lo) == c);
        }
    }
    const int flag = c != 0ull && !member ? 1 : 0;
    int incl = flag;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    int p = incl - flag, n_nm = 0;
    for (int q = 0; q < (nt >> 6); ++q) {
        p += q < w ? s_wsum[q] : 0;
        n_nm += s_wsum[q];
    }
    s_nm[tid] = p;
    if (tid == 0) s_nm[nt] = n_nm;
    __syncthreads();
    float* so = score_out + (size_t)b * k;
    int32_t* io = id_out + (size_t)b * k;
    if (flag && p < n_free && p + ahead < k) {
        io[p + ahead] = ia[tid];
        so[p + ahead] = sa[tid];
    }
    // ---- the entries of U: entry tid of every list (u_j <= quota[j] <= k <= k_in <= the block)
    for (int j = 0; j < n_lists; ++j) {
        const int t = tid;
        if (t >= s_u[j]) continue;
        const float* sg = score_grp + j * part + row;
        const int32_t* ig = id_grp + j * part + row;
        const uint64_t cu = tk_comp_at(sg, ig, t);
        int rank = t + min(s_nm[tk_count_above(sa, ia, k_in, cu)], n_free);
        for (int q = 0; q < n_lists; ++q)
            if (q != j) rank += tk_count_above(score_grp + q * part + row, id_grp + q * part + row, s_u[q], cu);
        if (rank < k) {
            io[rank] = ig[t];
            so[rank] = sg[t];
        }
    }
    for (int i = n_u + min(n_free, n_nm) + tid; i < k; i += nt) {
        io[i] = -1;
        so[i] = -INFINITY;
    }
}
