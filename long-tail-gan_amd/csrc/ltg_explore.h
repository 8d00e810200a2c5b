// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_topk.h): exploration lists --
// top-K sampled without replacement under the Plackett-Luce policy at temperature T, with the conditional log-probability of every
// pick (ltg_topk_sample, ltg_topk_sample_mass, ltg_topk_sample_finish).
//
// The draw is Gumbel-top-k: key = s * inv_temp + g, one fp32 multiply and one fp32 add that are never contracted, g = -logf(-logf(u)),
// u = ltg_rng_uniform(seed, LTG_STREAM_SERVE_GUMBEL, draw, global row * n_items_global + global id).  The key is a pure function of
// (seed, draw, global row, global id): no chunk, slab or rank enters it, so per-slab lists merge (ltg_topk_merge) into the list of the
// whole row bit for bit.  u == 0 gives key -inf: eligible, last.  The noise is recomputed in every pass and never stored.
// Order, ties, padding and the -0.0 == +0.0 rule are ltg_topk's applied to the keys (the tk_* words of ltg_topk.h).
#pragma once

// the product and the sum each rounded to fp32 on their own: the translation unit is built with contraction on, and __fmul_rn / __fadd_rn are
// plain operators there (ltg_calibrate.h), so the pragma is what keeps s * inv_temp + g from becoming one fused multiply-add
__device__ __forceinline__ float ex_key(float s, float inv_temp, float g) {
#pragma clang fp contract(off)
    const float p = s * inv_temp;
    return p + g;
}
// x = (s - M) * inv_temp: a difference, then a product (nothing here can fuse; the pragma states it)
__device__ __forceinline__ float ex_x(float s, float M, float inv_temp) {
#pragma clang fp contract(off)
    const float d = s - M;
    return d * inv_temp;
}
__device__ __forceinline__ float ex_gumbel(uint64_t seed, uint64_t draw, uint64_t idx) {
    return -logf(-logf(ltg_rng_uniform(seed, LTG_STREAM_SERVE_GUMBEL, draw, idx)));
}
// where a row's noise comes from: the injected values of the row (aligned with the slab's columns), else the counter at idx0 + column
struct ex_noise {
    const float* g;
    uint64_t seed, draw, idx0;
    __device__ __forceinline__ float at(int col) const { return g ? g[col] : ex_gumbel(seed, draw, idx0 + (uint64_t)col); }
};

// the keys (tk_key words; 0 = not eligible) of the 4 items 4j .. 4j+3 of a row
template <bool VEC>
__device__ __forceinline__ void ex_keys4(const float* row, int I, const unsigned* bits, int j, float inv_temp, const ex_noise& nz, uint32_t (&key)[4]) {
    float v[4];
    unsigned f;
    tk_load4<VEC>(row, I, bits, j, v, f);
#pragma unroll
    for (int t = 0; t < 4; ++t) key[t] = ((f >> t) & 1u) ? 0u : tk_key(ex_key(v[t], inv_temp, nz.at(4 * j + t)));
}

// the bitset of a row's items that are not eligible: fold-in items of tr, and the ids of list[0 .. n_list) that lie inside the slab
// (GLOBAL ids; ids outside the slab and padding index nothing).  Ends with a barrier.
__device__ __forceinline__ void ex_mark(unsigned* s_bits, int I, int item_lo, int b, const int32_t* tr_ptr, const int32_t* tr_idx,
                                        const int32_t* list, int n_list) {
    const int tid = threadIdx.x, nw = (I + 31) >> 5;
    for (int i = tid; i < nw; i += TK_NT) s_bits[i] = 0u;
    __syncthreads();
    if (tr_ptr) {
        for (int e = tr_ptr[b] + tid; e < tr_ptr[b + 1]; e += TK_NT) {
            const int it = tr_idx[e];
            if (it >= 0 && it < I) atomicOr(&s_bits[it >> 5], 1u << (it & 31));
        }
    }
    for (int e = tid; e < n_list; e += TK_NT) {
        const int g = list[e];
        if (g >= item_lo && g - item_lo < I) atomicOr(&s_bits[(g - item_lo) >> 5], 1u << ((g - item_lo) & 31));
    }
    __syncthreads();
}

// One workgroup per row; k_topk's passes over the keys instead of the logits.  LDS: bitset of the items that are not eligible | buf.
//   pass 1  per-thread maximum key; T0 = the k-th largest of the TK_NT maxima
//   pass 2  every eligible item with key >= T0 into buf; if they fit: sort, write the first k
//   else    exact radix select of the k-th key over 4 digits of 8 bits, then the keys above it and the first equal ones in id order
template <bool VEC>
__global__ __launch_bounds__(TK_NT) void k_topk_sample(int I, int item_lo, uint64_t I_glob, const float* __restrict__ logits,
                                                        const int32_t* __restrict__ tr_ptr, const int32_t* __restrict__ tr_idx, int k, int cap,
                                                        float inv_temp, uint64_t seed, uint64_t draw, int row_lo,
                                                        const int32_t* __restrict__ excl_id, int f_in, const float* __restrict__ g_noise,
                                                        float* __restrict__ key_out, int32_t* __restrict__ id_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];
    __shared__ int s_hist[256];
    __shared__ int s_wsum[TK_NT / 64];
    __shared__ int s_cnt, s_kk;
    __shared__ uint32_t s_prefix;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nw = (I + 31) >> 5;
    unsigned* s_bits = s_dyn;
    uint64_t* buf = reinterpret_cast<uint64_t*>(s_dyn + ((nw + 1) & ~1));
    if (tid == 0) s_cnt = 0;
    ex_mark(s_bits, I, item_lo, b, tr_ptr, tr_idx, f_in > 0 ? excl_id + (size_t)b * f_in : nullptr, f_in);
    int nf = 0;
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
    const ex_noise nz = {g_noise ? g_noise + (size_t)b * I : nullptr, seed, draw, ((uint64_t)row_lo + (uint64_t)b) * I_glob + (uint64_t)item_lo};
    const int n4 = (I + 3) >> 2;
    const int n_elig = I - n_fold;
    float* ko = key_out + (size_t)b * k;
    int32_t* io = id_out + (size_t)b * k;

    // ---- pass 1: per-thread maximum key
    uint32_t mx = 0u;
    for (int j = tid; j < n4; j += TK_NT) {
        uint32_t key[4];
        ex_keys4<VEC>(row, I, s_bits, j, inv_temp, nz, key);
        mx = max(max(mx, key[0]), max(key[1], max(key[2], key[3])));
    }
    buf[tid] = (uint64_t)mx << 32;
    __syncthreads();
    tk_sort_desc(buf, TK_NT);
    const uint32_t t0 = (uint32_t)(buf[k - 1] >> 32);      // 0 when fewer than k threads saw an eligible item: every eligible item qualifies
    __syncthreads();

    // ---- pass 2: candidates key >= T0
    for (int j0 = 0; j0 < n4; j0 += TK_NT) {            // (uniform trip count: the wave scan below needs every lane)
        const int j = j0 + tid;
        uint32_t key[4] = {0u, 0u, 0u, 0u};
        if (j < n4) ex_keys4<VEC>(row, I, s_bits, j, inv_temp, nz, key);
        int nc = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            key[t] = key[t] >= t0 ? key[t] : 0u;
            nc += key[t] != 0u ? 1 : 0;
        }
        if (__ballot(nc > 0) == 0ull) continue;
        int incl = nc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const int tot = __shfl(incl, 63);
        int base = 0;
        if (lane == 63) base = atomicAdd(&s_cnt, tot);
        base = __shfl(base, 63);
        int p = base + incl - nc;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (key[t] != 0u) {
                if (p < cap) buf[p] = tk_comp(key[t], item_lo + 4 * j + t);
                ++p;
            }
    }
    __syncthreads();
    const int n_cand = s_cnt;
    int n_sorted;
    if (n_cand <= cap) {
        n_sorted = n_cand;
    } else {
        // ---- exact radix select of the k-th largest key Tk among the eligible items (all of the k largest have key >= T0)
        uint32_t prefix = 0u;
        int kk = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            const uint32_t hmask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < 256; i += TK_NT) s_hist[i] = 0;
            __syncthreads();
            for (int j = tid; j < n4; j += TK_NT) {
                uint32_t key[4];
                ex_keys4<VEC>(row, I, s_bits, j, inv_temp, nz, key);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (key[t] != 0u && key[t] >= t0 && (key[t] & hmask) == prefix) atomicAdd(&s_hist[(key[t] >> shift) & 255u], 1);
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
            uint32_t key[4] = {0u, 0u, 0u, 0u};
            if (j < n4) ex_keys4<VEC>(row, I, s_bits, j, inv_temp, nz, key);
            int ne = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
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
            ko[i] = ex_key(row[gid - item_lo], inv_temp, nz.at(gid - item_lo));    // (the same arithmetic as in the passes: the same bits)
        } else {
            io[i] = -1;
            ko[i] = -INFINITY;
        }
    }
}

// The mass of a row over this slab, given the FINAL picks id_in [k] (GLOBAL ids): the raw logit of every pick the slab owns, M = the
// largest eligible logit (picks included), rest = the sum over the eligible items that were NOT picked of exp((s - M) * inv_temp).  Every
// term is positive; -inf logits add nothing.  One workgroup per row; thread t adds the items 4 (t + TK_NT i) .. + 3 for i = 0, 1, .. in
// that order, then a fixed tree (xor butterfly inside the wave, then over the TK_NT / 64 wave sums): bit-identical from run to run.
template <bool VEC>
__global__ __launch_bounds__(TK_NT) void k_topk_sample_mass(int I, int item_lo, const float* __restrict__ logits, const int32_t* __restrict__ tr_ptr,
                                                             const int32_t* __restrict__ tr_idx, int k, float inv_temp,
                                                             const int32_t* __restrict__ excl_id, int f_in, const int32_t* __restrict__ id_in,
                                                             float* __restrict__ score_out, float* __restrict__ max_out, float* __restrict__ rest_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_bits[];
    __shared__ float s_red[TK_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* row = logits + (size_t)b * I;
    const int32_t* picks = id_in + (size_t)b * k;
    ex_mark(s_bits, I, item_lo, b, tr_ptr, tr_idx, f_in > 0 ? excl_id + (size_t)b * f_in : nullptr, f_in);
    // ---- the picks: their logits; the eligible ones enter the maximum here, and all of them leave the sum below
    float mx = -INFINITY;
    for (int j = tid; j < k; j += TK_NT) {
        const int g = picks[j];
        float s = -INFINITY;
        if (g >= item_lo && g - item_lo < I) {
            const int c = g - item_lo;
            s = row[c];
            if (!((s_bits[c >> 5] >> (c & 31)) & 1u)) mx = fmaxf(mx, s);
        }
        score_out[(size_t)b * k + j] = s;
    }
    __syncthreads();                                     // (every thread has read the bits of its picks)
    for (int j = tid; j < k; j += TK_NT) {
        const int g = picks[j];
        if (g >= item_lo && g - item_lo < I) atomicOr(&s_bits[(g - item_lo) >> 5], 1u << ((g - item_lo) & 31));
    }
    __syncthreads();
    const int n4 = (I + 3) >> 2;
    for (int j = tid; j < n4; j += TK_NT) {
        float v[4];
        unsigned f;
        tk_load4<VEC>(row, I, s_bits, j, v, f);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (!((f >> t) & 1u)) mx = fmaxf(mx, v[t]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) s_red[w] = mx;
    __syncthreads();
    float M = s_red[0];
#pragma unroll
    for (int q = 1; q < TK_NT / 64; ++q) M = fmaxf(M, s_red[q]);
    __syncthreads();
    float acc = 0.f;
    for (int j = tid; j < n4; j += TK_NT) {
        float v[4];
        unsigned f;
        tk_load4<VEC>(row, I, s_bits, j, v, f);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (!((f >> t) & 1u) && v[t] != -INFINITY) acc += expf(ex_x(v[t], M, inv_temp));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) s_red[w] = acc;
    __syncthreads();
    if (w == 0) {
        float a = lane < TK_NT / 64 ? s_red[lane] : 0.f;
#pragma unroll
        for (int o = TK_NT / 128; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) {
            max_out[b] = M;
            rest_out[b] = a;
        }
    }
}

// logp of every pick, one wave per row: x_j = (s_j - M) * inv_temp, logp_j = x_j - log(rest + sum_{m >= j} exp(x_m)).  Lane l owns the
// entries l c .. l c + c - 1 (c = ceil(k / 64)); the lanes' totals are suffix-scanned by shuffles, then every lane walks its entries from
// the last to the first.  Only positive terms are ever added.  A score of -inf (padding) gets 0.0 and adds nothing.
__global__ __launch_bounds__(NT) void k_topk_sample_finish(int n_rows, int k, const float* __restrict__ score, const float* __restrict__ Mv,
                                                            const float* __restrict__ restv, float inv_temp, float* __restrict__ logp_out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;                             // (whole waves: no barrier below)
    const float* s = score + (size_t)r * k;
    float* lp = logp_out + (size_t)r * k;
    const float M = Mv[r];
    const int c = (k + 63) >> 6, j0 = min(k, lane * c), j1 = min(k, j0 + c);
    float tot = 0.f;
    for (int j = j1 - 1; j >= j0; --j)
        if (s[j] != -INFINITY) tot += expf(ex_x(s[j], M, inv_temp));
    float incl = tot;                                    // the entries of this lane and of every later one
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_down(incl, o);
        if (lane + o < 64) incl += y;
    }
    const float later = __shfl_down(incl, 1);
    float run = restv[r] + (lane < 63 ? later : 0.f);
    for (int j = j1 - 1; j >= j0; --j) {
        if (s[j] == -INFINITY) {
            lp[j] = 0.f;
            continue;
        }
        const float x = ex_x(s[j], M, inv_temp);
        run += expf(x);
        lp[j] = x - logf(run);
    }
}
