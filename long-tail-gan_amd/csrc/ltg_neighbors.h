// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_topk.h): item-to-item neighbours.
//   k_item_pack       an item table (W_p1t or W_q0, fp32 [I][H]) -> the bf16 operand image [I][608] of the W_p1t shadow; cosine: unit rows
//   k_item_neighbors  the top-k of (query image) x (table image)^T per query row and item SEGMENT, fused: the scores never leave the chip
// (ltg_item_neighbors = k_item_neighbors + k_topk_merge over the segments)
//
// Order and padding are ltg_topk's (64-bit (key, ~id) words of ltg_topk.h), so the lists go straight into ltg_topk_merge.
// Score of a pair = the accumulator of ONE chain of 19 v_mfma_f32_16x16x32_bf16 over the K steps in ascending order, whatever tile, wave,
// workgroup, segment or slab holds the item: an item-sharded run reproduces the unsharded scores bit for bit.
// Deterministic: the only atomics are LDS integer counters; what they order is sorted by a total order afterwards, and the SET a row keeps
// does not depend on the order (see the threshold below).
#pragma once

constexpr int NB_NT = 256;      // 4 waves
constexpr int NB_STEP = 128;    // items per workgroup step: one 32-item tile (two 16-item sub-tiles) per wave
constexpr int NB_ENT = 8192;    // candidate words per workgroup = query rows x capacity per row (64 KiB)

// one wave per item row: fp64 squared norm (cosine), one fp32 product per element, bf16 RNE, 16-byte stores; K padding written as zeros
template <bool COS>
__global__ __launch_bounds__(NT) void k_item_pack(int I, int H, const float* __restrict__ W, unsigned short* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6); i < I; i += gridDim.x * (NT / 64)) {
        const float* row = W + (size_t)i * H;
        float x[2][8];
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = 8 * (lane + 64 * u) + j;     // (chunk lane + 64 u of the row's 76: columns >= H, and chunks >= 76, are zero)
                x[u][j] = kk < H ? row[kk] : 0.f;
                s += (double)x[u][j] * (double)x[u][j];
            }
        float inv = 1.f;
        if (COS) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            inv = s > 0.0 ? (float)(1.0 / sqrt(s)) : 0.f;    // a zero row stays zero: its scores are 0, never NaN
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = lane + 64 * u;
            if (c < ST_C16) {
                ltg_u32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = COS ? x[u][2 * j] * inv : x[u][2 * j], b = COS ? x[u][2 * j + 1] * inv : x[u][2 * j + 1];
                    v[j] = (unsigned)ltg_f2bf(a) | ((unsigned)ltg_f2bf(b) << 16);
                }
                reinterpret_cast<ltg_u32x4*>(out + (size_t)i * ST_KP)[c] = v;
            }
        }
    }
}

// bitonic sort, descending, of every row [CAP] of buf [NB_ENT / CAP][CAP] at once (CAP a power of two).  only_over >= 0: rows holding at most
// that many entries are left alone.  Ends with a barrier.  NTH = the threads of the workgroup (ltg_companions.h sorts with 512).
template <int CAP, int NTH = NB_NT>
__device__ __forceinline__ void nb_sort_rows(uint64_t* buf, const int* cnt, int only_over) {
    for (int size = 2; size <= CAP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < NB_ENT / 2; i += NTH) {
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
// entries past a row's count -> 0 (no entry), then the sort
template <int CAP, int NTH = NB_NT>
__device__ __forceinline__ void nb_pad_sort(uint64_t* buf, const int* cnt, int only_over) {
    for (int e = threadIdx.x; e < NB_ENT; e += NTH)
        if ((e & (CAP - 1)) >= cnt[e / CAP]) buf[e] = 0ull;
    __syncthreads();
    nb_sort_rows<CAP, NTH>(buf, cnt, only_over);
}

// Workgroup (x, y) = query block x (16 NTB rows) against item segment y ([y seg_len, (y + 1) seg_len) of the slab, seg_len % 128 == 0).
// The product has k_dec1_fwd_stream2's shape: the query rows are resident in LDS in B-fragment order ([K step][row tile][lane] x 16 B, a
// straight copy of the image), items are the M dimension, every wave streams its own 32-item tile per step global -> VGPR in A-fragment
// order through a ring of 19 load units (unit u and u + 19 share registers; a step's last tile re-requests itself), indices are clamped
// instead of branched on, so every vmcnt in the K loop is an exact count.
// Epilogue instead of a store: a lane holds 2 x 4 consecutive items of row 16 nt + lr.  Each is turned into its (key, ~global id) word --
// 0 if not eligible (past the segment's end, the query itself, label not admitted) -- and compared with the row's threshold; a survivor is
// appended to the row's buffer [CAP] in LDS.  thr = 0 until the row has been compacted with k entries, then its k-th best word: always a
// true lower bound of the k-th best of everything the row has seen, and words are distinct, so `>` loses nothing.  A step appends at most
// 128 words per row; after every step (barrier), if any row holds more than CAP - 128, the rows holding more than k are sorted and cut to
// their k best (CAP >= k + 128).  Counts are sums, so this decision, the kept sets and every later threshold are independent of the order
// in which the waves appended.  At the end every row is sorted and written as a list: [segment][n_q][k].
template <int NTB, bool GRP>
__global__ __launch_bounds__(NB_NT) void k_item_neighbors(int I, int item_lo, int n_q, int seg_len, int k, const unsigned short* __restrict__ Tb,
                                                          const unsigned short* __restrict__ Qb, const int32_t* __restrict__ q_gid,
                                                          const uint8_t* __restrict__ labels, uint32_t group_mask, float* __restrict__ score_out,
                                                          int32_t* __restrict__ id_out) {
    constexpr int ROWS = 16 * NTB, CAP = NB_ENT / ROWS, NE = ST_KS * NTB * 64;
    static_assert(CAP >= LTG_NBR_MAX_K / (NTB == 1 ? 1 : 2) + NB_STEP, "a compacted row must have room for one more step");
    extern __shared__ __attribute__((aligned(16))) ltg_u32x4 nb_lds[];   // query fragments [NE] x 16 B | buf [ROWS][CAP] x 8 B
    __shared__ uint64_t s_thr[ROWS];
    __shared__ int s_cnt[ROWS];
    ltg_u32x4* Hs = nb_lds;
    uint64_t* buf = reinterpret_cast<uint64_t*>(nb_lds + NE);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int q0 = blockIdx.x * ROWS, seg_lo = blockIdx.y * seg_len, seg_hi = min(I, seg_lo + seg_len);
    const int nsteps = (seg_hi - seg_lo + NB_STEP - 1) / NB_STEP;
    const ltg_gchar* Tg = ltg_uniform_ptr(Tb);    // (32-bit byte offsets: the host refuses slabs of 2^32 bytes or more)
    auto rowoff = [&](int b, int ss) -> unsigned {
        const int it = min(b + 16 * ss + lr, I - 1);
        return (unsigned)it * (unsigned)(ST_KP * 2) + 16u * (unsigned)lq;
    };
    ltg_u32x4 Wr[ST2_RING];
    typedef const ltg_u32x4 __attribute__((address_space(1))) * nb_gp;
#define NB_LOAD(u, OFF0, OFF1) Wr[(u) % ST2_RING] = *(nb_gp)(Tg + (((u) & 1) ? (OFF1) : (OFF0)) + 64u * (unsigned)((u) >> 1));
    int base = seg_lo + 32 * w;
    unsigned c0 = rowoff(base, 0), c1 = rowoff(base, 1);
#pragma unroll
    for (int u = 0; u < ST2_RING; ++u) { NB_LOAD(u, c0, c1) }
    for (int e = tid; e < NE; e += NB_NT) {      // rows >= n_q mirror row n_q - 1 (their lists are not written)
        const int ln = e & 63, fr = e >> 6, nt = fr % NTB, ks = fr / NTB;
        const int row = min(q0 + 16 * nt + (ln & 15), n_q - 1);
        Hs[e] = reinterpret_cast<const ltg_u32x4*>(Qb + (size_t)row * ST_KP)[4 * ks + (ln >> 4)];
    }
    if (tid < ROWS) {
        s_thr[tid] = 0ull;
        s_cnt[tid] = 0;
    }
    int qg[NTB];
#pragma unroll
    for (int nt = 0; nt < NTB; ++nt) qg[nt] = q_gid[min(q0 + 16 * nt + lr, n_q - 1)];
    __syncthreads();
    const ltg_u32x4* Hl = Hs + lane;
#pragma unroll 1
    for (int s = 0; s < nsteps; ++s, base += NB_STEP) {
        const int nb = s + 1 < nsteps ? base + NB_STEP : base;
        const unsigned n0 = rowoff(nb, 0), n1 = rowoff(nb, 1);
        // the labels of the lane's 2 x 4 items, requested in front of the K loop (older than every refill: the wait for them drains nothing)
        unsigned lab[2][4];
        if (GRP) {
#pragma unroll
            for (int ss = 0; ss < 2; ++ss)
#pragma unroll
                for (int j = 0; j < 4; ++j) lab[ss][j] = labels[min(base + 16 * ss + 4 * lq + j, I - 1)];
        }
        ltg_f32x4 acc[2][NTB];
#pragma unroll
        for (int nt = 0; nt < NTB; ++nt) {
            acc[0][nt] = ltg_f32x4{0.f, 0.f, 0.f, 0.f};
            acc[1][nt] = ltg_f32x4{0.f, 0.f, 0.f, 0.f};
        }
        ltg_u32x4 bnx[NTB];      // the query fragments of the NEXT K step are read under this step's MFMAs (one wave per SIMD: nobody else hides them)
#pragma unroll
        for (int nt = 0; nt < NTB; ++nt) bnx[nt] = Hl[nt * 64];
#pragma unroll
        for (int ks = 0; ks < ST_KS; ++ks) {
            ltg_u32x4 bfr[NTB];
#pragma unroll
            for (int nt = 0; nt < NTB; ++nt) bfr[nt] = bnx[nt];
            if (ks + 1 < ST_KS) {
#pragma unroll
                for (int nt = 0; nt < NTB; ++nt) bnx[nt] = Hl[((ks + 1) * NTB + nt) * 64];
            }
            const ltg_bf16x8 a0 = __builtin_bit_cast(ltg_bf16x8, Wr[(2 * ks) % ST2_RING]);
            const ltg_bf16x8 a1 = __builtin_bit_cast(ltg_bf16x8, Wr[(2 * ks + 1) % ST2_RING]);
#pragma unroll
            for (int nt = 0; nt < NTB; ++nt) {
                const ltg_bf16x8 b = __builtin_bit_cast(ltg_bf16x8, bfr[nt]);
                acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[0][nt], 0, 0, 0);
                acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[1][nt], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (2 * ks + ST2_RING < ST2_UNITS) { NB_LOAD(2 * ks + ST2_RING, c0, c1) } else { NB_LOAD(2 * ks + ST2_RING - ST2_UNITS, n0, n1) }
            if (2 * ks + 1 + ST2_RING < ST2_UNITS) { NB_LOAD(2 * ks + 1 + ST2_RING, c0, c1) } else { NB_LOAD(2 * ks + 1 + ST2_RING - ST2_UNITS, n0, n1) }
            __builtin_amdgcn_sched_barrier(0);
        }
        // eligibility of the lane's items as a mask on the id word: an item that is not eligible compares as "no entry"
        int gid[2][4];
        bool ok[2][4];
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int it = base + 16 * ss + 4 * lq + j;
                gid[ss][j] = item_lo + it;
                ok[ss][j] = it < seg_hi;
                if (GRP) ok[ss][j] = ok[ss][j] && ((group_mask >> min(lab[ss][j], 8u)) & 1u);
            }
        __syncthreads();     // every wave has read the counts the last step left (below) before they move again
#pragma unroll
        for (int nt = 0; nt < NTB; ++nt) {
            const int r = 16 * nt + lr;
            const uint64_t thr = s_thr[r];
#pragma unroll
            for (int ss = 0; ss < 2; ++ss)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t c = ok[ss][j] && gid[ss][j] != qg[nt] ? tk_comp(tk_key(acc[ss][nt][j]), gid[ss][j]) : 0ull;
                    if (c > thr) buf[r * CAP + atomicAdd(&s_cnt[r], 1)] = c;
                }
        }
        __syncthreads();
        if (__ballot(s_cnt[lane & (ROWS - 1)] > CAP - NB_STEP) != 0ull) {      // (the same counts in every wave: uniform over the workgroup)
            nb_pad_sort<CAP>(buf, s_cnt, k);
            if (tid < ROWS && s_cnt[tid] > k) {
                s_cnt[tid] = k;
                s_thr[tid] = buf[tid * CAP + k - 1];
            }
            __syncthreads();
        }
        c0 = n0;
        c1 = n1;
    }
#undef NB_LOAD
    nb_pad_sort<CAP>(buf, s_cnt, -1);
    const size_t seg = (size_t)blockIdx.y * n_q;
    for (int e = tid; e < ROWS * k; e += NB_NT) {
        const int r = e / k, i = e - r * k, row = q0 + r;
        if (row >= n_q) continue;
        const uint64_t c = buf[r * CAP + i];
        const uint32_t key = (uint32_t)(c >> 32);
        const size_t o = (seg + row) * k + i;
        id_out[o] = c != 0ull ? (int)~(uint32_t)c : -1;
        score_out[o] = c != 0ull ? __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key) : -INFINITY;
    }
}
