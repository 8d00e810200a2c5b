// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_explore.h): replay of an exploration
// log under other policies -- the mass of a FOREIGN list under up to 8 target temperatures in one read of the logits (ltg_list_mass), and
// the prefix importance weights with their per-group sums (ltg_replay_rows).
//
// A logged list is not the target's own sample: an entry may be a fold-in item of the row or an item of the target's head, and then it has
// no support under the target.  k_list_mass therefore reads the eligibility of every logged entry BEFORE it takes the supported ones out of
// the sum, and says which is which (state 1 / 2); an unsupported entry adds no mass anywhere.  The arithmetic of a term is
// k_topk_sample_mass's: expf(ex_x(s, M, inv_temp)) added in fp32, thread t walking the items 4 (t + TK_NT i) .. + 3 in that order, then the
// same fixed tree.  Max and sum are two passes over the row (the second one is served by the cache the first one filled), as there.
#pragma once

constexpr int RP_MAXP = 8;        // target temperatures per call
constexpr int RP_MAXG = 8;        // item groups, ltg_topk_metrics' range (LT_MAXG of ltg_longtail.h, included later); slot n_groups is "all"
struct rp_temps {
    float v[RP_MAXP];
};

// One workgroup per row.  LDS: bitset of the items that are not eligible under the target (fold-in items, the target's head), to which the
// supported logged entries are added once their state is written.  NP = n_pol rounded up to 1, 4 or 8: the sums live in registers.
template <bool VEC, int NP>
__global__ __launch_bounds__(TK_NT) void k_list_mass(int I, int item_lo, const float* __restrict__ logits, const int32_t* __restrict__ tr_ptr,
                                                      const int32_t* __restrict__ tr_idx, int n_rows, int k, const int32_t* __restrict__ id_in,
                                                      int f_in, const int32_t* __restrict__ excl_id, int n_pol, rp_temps it,
                                                      float* __restrict__ score_out, int32_t* __restrict__ state_out, float* __restrict__ max_out,
                                                      float* __restrict__ rest_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_bits[];
    __shared__ float s_red[NP][TK_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* row = logits + (size_t)b * I;
    const int32_t* list = id_in + (size_t)b * k;
    ex_mark(s_bits, I, item_lo, b, tr_ptr, tr_idx, f_in > 0 ? excl_id + (size_t)b * f_in : nullptr, f_in);
    // ---- the logged entries: state and raw logit; the supported ones enter the maximum here and leave the sum below
    float mx = -INFINITY;
    for (int j = tid; j < k; j += TK_NT) {
        const int g = list[j];
        float s = -INFINITY;
        int st = 0;
        if (j >= f_in && g >= item_lo && g - item_lo < I) {
            const int c = g - item_lo;
            if ((s_bits[c >> 5] >> (c & 31)) & 1u) {
                st = 2;
            } else {
                st = 1;
                s = row[c];
                mx = fmaxf(mx, s);
            }
        }
        score_out[(size_t)b * k + j] = s;
        state_out[(size_t)b * k + j] = st;
    }
    __syncthreads();                                     // (every thread has read the bits of its entries)
    for (int j = tid; j < k; j += TK_NT) {               // (an entry of state 2 has its bit already; ids of a row are distinct)
        const int g = list[j];
        if (j >= f_in && g >= item_lo && g - item_lo < I) atomicOr(&s_bits[(g - item_lo) >> 5], 1u << ((g - item_lo) & 31));
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
    if (lane == 0) s_red[0][w] = mx;
    __syncthreads();
    float M = s_red[0][0];
#pragma unroll
    for (int q = 1; q < TK_NT / 64; ++q) M = fmaxf(M, s_red[0][q]);
    __syncthreads();
    float acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.f;
    for (int j = tid; j < n4; j += TK_NT) {
        float v[4];
        unsigned f;
        tk_load4<VEC>(row, I, s_bits, j, v, f);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (!((f >> t) & 1u) && v[t] != -INFINITY) {
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    if (p < n_pol) acc[p] += expf(ex_x(v[t], M, it.v[p]));
            }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        float a = acc[p];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) s_red[p][w] = a;
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float a = lane < TK_NT / 64 ? s_red[p][lane] : 0.f;
#pragma unroll
            for (int o = TK_NT / 128; o > 0; o >>= 1) a += __shfl_xor(a, o);
            if (lane == 0 && p < n_pol) rest_out[(size_t)p * n_rows + b] = a;
        }
        if (lane == 0) max_out[b] = M;
    }
}

// is logged slot j of a row supported under the target?  -1 = padding, 0 = no, 1 = yes
__device__ __forceinline__ int rp_support(int j, int f_in, int gid, const int32_t* head, const int32_t* state) {
    if (gid < 0) return -1;
    return j < f_in ? (head[j] == gid ? 1 : 0) : (state[j] == 1 ? 1 : 0);
}

// Prefix importance weights of a logged row under every target policy, one wave per row, all in fp64.  Lane l owns the slots l c .. l c + c - 1
// (c = ceil(k / 64)).  Per policy: the lanes' sums of exp(x) are suffix-scanned by shuffles and every lane walks its slots from the last to
// the first (logp1, positive terms only); the d = logp1 - logp0 of its slots wait in LDS, the lanes' sums of d are prefix-scanned and every
// lane walks its slots from the first to the last (c_j, w_j, A, B); A and B go through an xor butterfly.  logp1_out: 0.0 for padding and a
// matching head entry, -inf for a slot without support.  A row without a real slot has W = exp(min(0, log clip)), the empty product.
// No workspace, no atomics: the same bits on every run.
__global__ __launch_bounds__(NT) void k_replay_rows(int n_rows, int k, int n_pol, rp_temps it, int f_in, const int32_t* __restrict__ head_id,
                                                     const int32_t* __restrict__ id_in, const float* __restrict__ logp0,
                                                     const float* __restrict__ reward, const float* __restrict__ score,
                                                     const int32_t* __restrict__ state, const float* __restrict__ Mv,
                                                     const float* __restrict__ restv, const uint8_t* __restrict__ item_group, int n_groups,
                                                     int n_items_global, double log_clip, double* __restrict__ row_out, double* __restrict__ w_out,
                                                     int32_t* __restrict__ first_bad_out, float* __restrict__ logp1_out) {
    __shared__ double s_d[NT / 64][1024];                // d_j of the wave's row under the policy at hand
    const int lane = threadIdx.x & 63, r = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;                             // (whole waves: no barrier below)
    const int32_t* ids = id_in + (size_t)r * k;
    const int32_t* st = state + (size_t)r * k;
    const int32_t* head = f_in > 0 ? head_id + (size_t)r * f_in : nullptr;
    const float* sc = score + (size_t)r * k;
    const float* lp0 = logp0 + (size_t)r * k;
    const float* y = reward + (size_t)r * k;
    const double M = (double)Mv[r];
    const int c = (k + 63) >> 6, j0 = min(k, lane * c), j1 = min(k, j0 + c);
    // ---- what no policy changes: the first unsupported slot and the last real one
    int bad = k, last = -1;
    for (int j = j0; j < j1; ++j) {
        const int s = rp_support(j, f_in, ids[j], head, st);
        if (s == 0) bad = min(bad, j);
        if (s >= 0) last = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad = min(bad, __shfl_xor(bad, o));
        last = max(last, __shfl_xor(last, o));
    }
    for (int p = 0; p < n_pol; ++p) {
        const double itp = (double)it.v[p];
        // ---- logp1: suffix sums of exp(x) over the supported sampled slots
        double tot = 0.0;
        for (int j = j1 - 1; j >= j0; --j)
            if (j >= f_in && rp_support(j, f_in, ids[j], head, st) == 1) tot += exp(((double)sc[j] - M) * itp);
        double incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double v = __shfl_down(incl, o);
            if (lane + o < 64) incl += v;
        }
        const double later = __shfl_down(incl, 1);
        double run = (double)restv[(size_t)p * n_rows + r] + (lane < 63 ? later : 0.0);
        double dsum = 0.0;                               // this lane's sum of d over its supported slots
        for (int j = j1 - 1; j >= j0; --j) {
            const int s = rp_support(j, f_in, ids[j], head, st);
            double l1 = s == 0 ? -INFINITY : 0.0;        // (padding and a matching head entry: 0; no support: log 0)
            if (s == 1 && j >= f_in) {
                const double x = ((double)sc[j] - M) * itp;
                run += exp(x);
                l1 = x - log(run);
            }
            const double dj = s == 1 ? l1 - (double)lp0[j] : 0.0;
            s_d[threadIdx.x >> 6][j] = dj;               // (read back below by this lane alone)
            dsum += dj;
            if (logp1_out) logp1_out[((size_t)p * n_rows + r) * k + j] = (float)l1;
        }
        // ---- c_j: prefix sums of d
        double pre = dsum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double v = __shfl_up(pre, o);
            if (lane >= o) pre += v;
        }
        double cj = pre - dsum;                          // the slots of the earlier lanes
        double A[RP_MAXG + 1], B[RP_MAXG + 1];
#pragma unroll
        for (int g = 0; g <= RP_MAXG; ++g) A[g] = B[g] = 0.0;
        double w_last = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int gid = ids[j];
            if (gid < 0) continue;
            cj += s_d[threadIdx.x >> 6][j];
            double wj = 0.0;
            if (j < bad) wj = exp(fmin(cj, log_clip));
            if (j == last) w_last = wj;
            const double wy = wj * (double)y[j];
            const int lab = gid < n_items_global ? (int)item_group[gid] : 255;
#pragma unroll
            for (int g = 0; g < RP_MAXG; ++g)
                if (g == lab && g < n_groups) {
                    A[g] += wy;
                    B[g] += wj;
                }
            A[RP_MAXG] += wy;
            B[RP_MAXG] += wj;
        }
#pragma unroll
        for (int g = 0; g <= RP_MAXG; ++g) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                A[g] += __shfl_xor(A[g], o);
                B[g] += __shfl_xor(B[g], o);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w_last += __shfl_xor(w_last, o);       // (one lane holds it, the others 0.0)
        if (lane == 0) {
            double* out = row_out + ((size_t)r * n_pol + p) * (size_t)(n_groups + 1) * 2;
#pragma unroll
            for (int g = 0; g < RP_MAXG; ++g)
                if (g < n_groups) {
                    out[2 * g] = A[g];
                    out[2 * g + 1] = B[g];
                }
            out[2 * n_groups] = A[RP_MAXG];
            out[2 * n_groups + 1] = B[RP_MAXG];
            w_out[(size_t)r * n_pol + p] = bad < k ? 0.0 : (last < 0 ? exp(fmin(0.0, log_clip)) : w_last);
            first_bad_out[(size_t)r * n_pol + p] = bad;
        }
    }
}
