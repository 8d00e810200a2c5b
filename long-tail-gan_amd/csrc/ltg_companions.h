// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_neighbors.h): niche companions --
// the discriminator's top-k partners of an item.
//   k_pair_pack        ids -> the side image [n][ld] fp32: E = expf(2 x) of the pre-activation x that one side contributes to the fc layer
//   k_pair_companions  the top-k of score(q, c) per query row and candidate SEGMENT, fused: the scores never leave the chip
//   k_pair_fill        all-padding lists (no candidates)
// (ltg_pair_companions = k_pair_companions + k_topk_merge over the segments.)
//
// s(a, b) = b4 + sum_j w4[j] tanh(U[a][j] + V[b][j]) does not separate into a product of item vectors, but exp does:
// tanh(u + v) = 1 - 2 / (1 + exp(2u) exp(2v)), so with Eu = exp(2u), Ev = exp(2v) stored per item the pair loop holds no exponential:
//   s = c0 - 2 sum_j w4[j] rcp(1 + Eq[j] Ec[j]),   c0 = b4 + sum_j w4[j]
// -- per element one v_fma_f32, one v_rcp_f32 (1 ulp, quarter rate: what bounds the kernel) and one v_fma_f32.
// Order: ONE chain acc <- fma(w4[j], rcp(fma(Eq[j], Ec[j], 1)), acc) from acc = 0 over j = 0 .. h3 - 1 ascending, then fma(-2, acc, c0); c0 is
// summed in fp64 (b4, then w4[0 .. h3 - 1] ascending) and rounded once.  Nothing of that depends on the tile, wave, workgroup, segment or
// call that holds the pair (and the product Eq Ec commutes), so candidates or queries split across calls reproduce the same bits.
// x is clamped to [-40, 40] by the pack: E lies in [e^-80, e^80], finite and normal, so Eq Ec is 0 .. +inf but never inf x 0; rcp(1) = 1 and
// rcp(inf) = 0 are the two saturated ends.  The loop ends at h3: the padding columns [h3, ld) of an image are never read.
// Order and padding of the lists are ltg_topk's (64-bit (key, ~id) words of ltg_topk.h), so per-part lists go straight into ltg_topk_merge.
// Deterministic: no atomics at all -- a query row's buffer belongs to one wave, which appends by ballot and prefix count.
#pragma once

constexpr int PC_NT = 512;       // 8 waves, two per SIMD (one workgroup per CU: the LDS holds the candidate tile and the row buffers)
constexpr int PC_CT = 64;        // candidates per step: one per lane, the same 64 for every wave
constexpr int PC_ENT = 8192;     // candidate words per workgroup = query rows x capacity per row (64 KiB)
constexpr int PC_JU = 4;         // j per unrolled block: a block's Eq / w4 arrive as scalar loads one block ahead (8: the SGPRs spill)
constexpr int PC_MAX_H3 = 352;   // the tile [64][ld | 1] fp32 and the row buffers share the CU's 160 KiB
constexpr int PC_NJ = (PC_MAX_H3 + 63) / 64;   // dwords per lane of one image row
constexpr int PK_IDS = 8;       // ids per workgroup of the pack: every weight read serves eight rows
constexpr int PK_MAX_H = 2048;   // h0 + max(h1, h2): the pack keeps eight embedding rows and eight branch activations in LDS (64 KiB)

// Workgroup b = ids [8 b, 8 b + 8).  wb [h0][hb], bb [hb]: the side's branch layer; w3s [hb][h3]: the side's rows of w3; b3 [h3] on the niche
// side, NULL on the popular side.  Every output element is one fmaf chain in ascending index order from 0, the bias added last: an id's row
// is the same bits wherever it sits in `ids` and whatever n is.  Padding columns are written as E(0) = 1.
__global__ __launch_bounds__(NT) void k_pair_pack(int n, int h0, int hb, int h3, int ld, const float* __restrict__ emb, const float* __restrict__ wb,
                                                  const float* __restrict__ bb, const float* __restrict__ w3s, const float* __restrict__ b3,
                                                  const int32_t* __restrict__ ids, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float pk_lds[];      // e [PK_IDS][h0] | t [PK_IDS][hb]
    float* e = pk_lds;
    float* t = pk_lds + PK_IDS * h0;
    const int tid = threadIdx.x;
    const size_t i0 = (size_t)blockIdx.x * PK_IDS;
    for (int u = 0; u < PK_IDS; ++u) {      // (rows past n mirror row n - 1; they are not written)
        const size_t id = (size_t)ids[i0 + u < (size_t)n ? i0 + u : (size_t)n - 1];
        for (int r = tid; r < h0; r += NT) e[u * h0 + r] = emb[id * h0 + r];
    }
    __syncthreads();
    for (int i = tid; i < hb; i += NT) {
        float acc[PK_IDS];
#pragma unroll
        for (int u = 0; u < PK_IDS; ++u) acc[u] = 0.f;
        for (int r = 0; r < h0; ++r) {
            const float w = wb[(size_t)r * hb + i];
#pragma unroll
            for (int u = 0; u < PK_IDS; ++u) acc[u] = fmaf(e[u * h0 + r], w, acc[u]);
        }
        const float b = bb[i];
#pragma unroll
        for (int u = 0; u < PK_IDS; ++u) t[u * hb + i] = tanhf(acc[u] + b);
    }
    __syncthreads();
    for (int j = tid; j < ld; j += NT) {
        float E[PK_IDS];
        if (j < h3) {
            float acc[PK_IDS];
#pragma unroll
            for (int u = 0; u < PK_IDS; ++u) acc[u] = 0.f;
            for (int i = 0; i < hb; ++i) {
                const float w = w3s[(size_t)i * h3 + j];
#pragma unroll
                for (int u = 0; u < PK_IDS; ++u) acc[u] = fmaf(t[u * hb + i], w, acc[u]);
            }
            const float b = b3 ? b3[j] : 0.f;
#pragma unroll
            for (int u = 0; u < PK_IDS; ++u) {
                const float x = fminf(fmaxf(b3 ? acc[u] + b : acc[u], -40.f), 40.f);
                E[u] = expf(2.f * x);       // libm's expf (1 ulp), not __expf
            }
        } else {
#pragma unroll
            for (int u = 0; u < PK_IDS; ++u) E[u] = 1.f;
        }
#pragma unroll
        for (int u = 0; u < PK_IDS; ++u)
            if (i0 + u < (size_t)n) out[(i0 + u) * ld + j] = E[u];
    }
}

__global__ __launch_bounds__(NT) void k_pair_fill(size_t n, float* __restrict__ score_out, int32_t* __restrict__ id_out) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        score_out[i] = -INFINITY;
        id_out[i] = -1;
    }
}

// Workgroup (x, y) = query block x (8 R rows) against candidate segment y ([y seg_len, (y + 1) seg_len) of the candidates, seg_len % 64 == 0).
// A step = 64 candidates.  Their image rows are copied into LDS, row stride ld | 1 floats (odd: lane c reads column j of its own row without
// a bank conflict, and the copy writes along a row).  Lane c of EVERY wave owns candidate c of the step; wave w owns the query rows R w ..
// R w + R - 1 of the block: its Eq[row][j] are wave-uniform and arrive as scalar loads, w4[j] as a broadcast LDS read, a block of PC_JU
// columns ahead of their use, so a loop body is one ds_read_b32 per column and, per row, fma / rcp / fma on R independent accumulators
// (two waves per SIMD: 2 R reciprocals in flight).
// Epilogue instead of a store: a lane turns its R scores into (key, ~global id) words -- 0 if not eligible (past the segment's end, the
// query itself) -- and compares with the row's threshold; the wave appends the survivors to the row's buffer [CAP] by ballot and prefix
// count (the row is this wave's alone: no atomics, and the order of the buffer is fixed too).  thr = 0 until the row has been compacted
// with k entries, then its k-th best word: always a true lower bound of the k-th best of everything the row has seen, and words are
// distinct, so `>` loses nothing.  A step appends at most 64 words per row; after every step (barrier), if any row holds more than
// CAP - 64, the rows holding more than k are sorted and cut to their k best (CAP >= k + 64).  At the end every row is sorted and written
// as a list: [segment][n_q][k].
template <int R>
__global__ __launch_bounds__(PC_NT) void k_pair_companions(int n_q, int n_c, int seg_len, int k, int h3, int ld, const float* __restrict__ Eq,
                                                           const int32_t* __restrict__ q_gid, const float* __restrict__ Ec,
                                                           const int32_t* __restrict__ c_gid, const float* __restrict__ w4,
                                                           const float* __restrict__ b4, float* __restrict__ score_out,
                                                           int32_t* __restrict__ id_out) {
    constexpr int ROWS = (PC_NT / 64) * R, CAP = PC_ENT / ROWS;
    static_assert(PC_ENT == NB_ENT, "the row buffers are sorted by ltg_neighbors.h's nb_pad_sort");
    static_assert(CAP >= LTG_PAIR_MAX_K / (R == 2 ? 1 : 2) + PC_CT, "a compacted row must have room for one more step");
    extern __shared__ __attribute__((aligned(16))) uint64_t pc_lds[];   // buf [ROWS][CAP] x 8 B | tile [PC_CT][ld | 1] fp32
    __shared__ uint64_t s_thr[ROWS];
    __shared__ int s_cnt[ROWS];
    __shared__ float s_c0;
    __shared__ float s_w4[PC_MAX_H3];
    uint64_t* buf = pc_lds;
    float* tile = reinterpret_cast<float*>(pc_lds + PC_ENT);
    const int ldp = ld | 1;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q0 = blockIdx.x * ROWS, seg_lo = blockIdx.y * seg_len, seg_hi = min(n_c, seg_lo + seg_len);
    if (tid < ROWS) {
        s_thr[tid] = 0ull;
        s_cnt[tid] = 0;
    }
    if (tid == 0) {
        double c = (double)b4[0];
        for (int j = 0; j < h3; ++j) c += (double)w4[j];
        s_c0 = (float)c;
    }
    for (int j = tid; j < h3; j += PC_NT) s_w4[j] = w4[j];
    const float* eq[R];     // rows >= n_q mirror row n_q - 1 (their lists are not written)
    int qg[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = min(q0 + R * w + r, n_q - 1);
        eq[r] = Eq + (size_t)row * ld;
        qg[r] = q_gid[row];
    }
    // A step's tile travels global -> registers -> LDS: wave w carries rows w, w + 8, ..., a lane one dword per 64 columns (rows past the end
    // mirror the last row, columns past ld the last column: every load is in bounds, the writes are masked).  The NEXT step's rows are
    // requested before this step is computed, so their latency hides under the reciprocals.
    float tv[PC_CT / (PC_NT / 64)][PC_NJ];
    auto fetch = [&](int base) {
#pragma unroll
        for (int i = 0; i < PC_CT / (PC_NT / 64); ++i) {
            const float* src = Ec + (size_t)min(base + w + (PC_NT / 64) * i, n_c - 1) * ld;
#pragma unroll
            for (int u = 0; u < PC_NJ; ++u)
                if (64 * u < ld) tv[i][u] = src[min(lane + 64 * u, ld - 1)];
        }
    };
    fetch(seg_lo);
    const float* tl = tile + lane * ldp;
    const int nfull = h3 / PC_JU;
    __syncthreads();
#pragma unroll 1
    for (int base = seg_lo; base < seg_hi; base += PC_CT) {
#pragma unroll
        for (int i = 0; i < PC_CT / (PC_NT / 64); ++i)
#pragma unroll
            for (int u = 0; u < PC_NJ; ++u)
                if (lane + 64 * u < ld) tile[(w + (PC_NT / 64) * i) * ldp + lane + 64 * u] = tv[i][u];
        const int ci = base + lane;
        const int gid = c_gid[min(ci, n_c - 1)];
        __syncthreads();
        if (base + PC_CT < seg_hi) fetch(base + PC_CT);
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        // block b + 1's operands -- the lane's tile columns and w4 (LDS; w4 a broadcast read), the wave's Eq (scalar loads) -- are requested
        // before block b is computed: both kinds count in lgkmcnt and scalar loads return out of order, so a request placed beside its use
        // would wait for all of them
        float en[PC_JU], qn[R][PC_JU], wn[PC_JU];
        if (nfull > 0) {
#pragma unroll
            for (int u = 0; u < PC_JU; ++u) {
                en[u] = tl[u];
                wn[u] = s_w4[u];
#pragma unroll
                for (int r = 0; r < R; ++r) qn[r][u] = eq[r][u];
            }
        }
#pragma unroll 1
        for (int b = 0; b < nfull; ++b) {
            const int j = b * PC_JU;
            float e[PC_JU], qv[R][PC_JU], wv[PC_JU];
#pragma unroll
            for (int u = 0; u < PC_JU; ++u) {
                e[u] = en[u];
                wv[u] = wn[u];
#pragma unroll
                for (int r = 0; r < R; ++r) qv[r][u] = qn[r][u];
            }
            if (b + 1 < nfull) {
#pragma unroll
                for (int u = 0; u < PC_JU; ++u) {
                    en[u] = tl[j + PC_JU + u];
                    wn[u] = s_w4[j + PC_JU + u];
#pragma unroll
                    for (int r = 0; r < R; ++r) qn[r][u] = eq[r][j + PC_JU + u];
                }
            }
#pragma unroll
            for (int u = 0; u < PC_JU; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(wv[u], __builtin_amdgcn_rcpf(fmaf(qv[r][u], e[u], 1.f)), acc[r]);
        }
        for (int j = nfull * PC_JU; j < h3; ++j) {
            const float e = tl[j], wj = s_w4[j];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fmaf(wj, __builtin_amdgcn_rcpf(fmaf(eq[r][j], e, 1.f)), acc[r]);
        }
        const float c0 = s_c0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int rr = R * w + r;
            const float s = fmaf(-2.f, acc[r], c0);
            const uint64_t word = ci < seg_hi && gid != qg[r] ? tk_comp(tk_key(s), gid) : 0ull;
            const bool pass = word > s_thr[rr];
            const unsigned long long m = __ballot(pass);
            if (m != 0ull) {
                const int cnt = s_cnt[rr];
                if (pass) buf[rr * CAP + cnt + __popcll(m & ((1ull << lane) - 1ull))] = word;
                if (lane == 0) s_cnt[rr] = cnt + __popcll(m);
            }
        }
        __syncthreads();     // every wave is done with the tile; the counts are final for this step
        if (__ballot(s_cnt[lane & (ROWS - 1)] > CAP - PC_CT) != 0ull) {      // (the same counts in every wave: uniform over the workgroup)
            nb_pad_sort<CAP, PC_NT>(buf, s_cnt, k);
            if (tid < ROWS && s_cnt[tid] > k) {
                s_cnt[tid] = k;
                s_thr[tid] = buf[tid * CAP + k - 1];
            }
            __syncthreads();
        }
    }
    nb_pad_sort<CAP, PC_NT>(buf, s_cnt, -1);
    const size_t seg = (size_t)blockIdx.y * n_q;
    for (int e = tid; e < ROWS * k; e += PC_NT) {
        const int r = e / k, i = e - r * k, row = q0 + r;
        if (row >= n_q) continue;
        const uint64_t c = buf[r * CAP + i];
        const uint32_t key = (uint32_t)(c >> 32);
        const size_t o = (seg + row) * k + i;
        id_out[o] = c != 0ull ? (int)~(uint32_t)c : -1;
        score_out[o] = c != 0ull ? __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key) : -INFINITY;
    }
}
