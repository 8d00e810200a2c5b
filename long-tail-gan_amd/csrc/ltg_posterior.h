// Part of csrc/ltg_kernels.hip (one translation unit, one anonymous namespace; included there after ltg_explore.h): posterior-aware scores.
//   k_post_h2       S samples of z per user row -> tanh(dec-0) -> the bf16 operand image [n * S][ld], reparameterisation through pack
//   k_post_scores   (image) x (W_p1t)^T on v_mfma_f32_16x16x32_bf16, reduced over the S sample rows in the accumulator registers:
//                   mean + beta * std per (user, item); the [n * S][I] logits never leave the chip
//   k_post_entries  the same mean and std for the k list entries of every row, one wave per entry
//   The operands of the big product are bf16 WHATEVER cfg->precision is: the image is bf16 by construction, W_p1t is the bf16
// shadow or the fp32 rows rounded on the fly (the same values).
// Score of (sample row, item) = the accumulator of ONE chain of ld / 32 MFMAs over the K steps in ascending order, plus the bias; the S
// values of a (user, item) are then added in a fixed balanced tree over the sample index.  Neither depends on the tile, the wave, the
// workgroup, the segment or the slab that holds the item: an item-sharded run reproduces the unsharded scores bit for bit.  No atomics.
#pragma once

constexpr int PO_NT = 256;                  // 4 waves
constexpr int PO_RT = 4;                    // 16-row tiles of the image per workgroup: 64 sample rows, resident in LDS
constexpr int PO_ROWS = 16 * PO_RT;
constexpr int PO_IT = 4;                    // 16-item tiles per wave and step
constexpr int PO_STEP = 4 * 16 * PO_IT;     // items per workgroup step
constexpr int PO_PF = 3;                    // K steps the B fragments are requested ahead

// One workgroup per user row: the S samples of z in LDS, then every thread owns columns of dec-0 for all S samples (W_p0 is read once per
// row, coalesced; the sum over Z is one fmaf chain in ascending order, so a row's image does not depend on the call that holds it).
template <int S>
__global__ __launch_bounds__(PO_NT) void k_post_h2(int Z, int H, int ld, const float* __restrict__ mulv, const float* __restrict__ eps,
                                                   uint64_t seed, uint64_t draw, int row_lo, const float* __restrict__ Wp0,
                                                   const float* __restrict__ bp0, unsigned short* __restrict__ image,
                                                   float* __restrict__ z_out) {
    extern __shared__ __attribute__((aligned(16))) float po_z[];   // [S][Z]
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* mv = mulv + (size_t)r * 2 * Z;
    for (int e = tid; e < S * Z; e += PO_NT) {
        const int s = e / Z, j = e - s * Z;
        const float mu = mv[j], sd = expf(0.5f * mv[Z + j]);
        const float en = eps ? eps[((size_t)r * S + s) * Z + j]
                             : ltg_rng_normal(seed, LTG_STREAM_POSTERIOR_EPS, draw, ((uint64_t)(row_lo + r) * S + s) * (uint64_t)Z + j);
        const float z = mu + sd * en;
        po_z[e] = z;
        if (z_out) z_out[((size_t)r * S + s) * Z + j] = z;
    }
    __syncthreads();
    for (int c = tid; c < ld; c += PO_NT) {
        float acc[S];
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] = 0.f;
        if (c < H) {
            for (int j = 0; j < Z; ++j) {
                const float w = Wp0[(size_t)j * H + c];
#pragma unroll
                for (int s = 0; s < S; ++s) acc[s] = fmaf(po_z[s * Z + j], w, acc[s]);
            }
        }
        const float b = c < H ? bp0[c] : 0.f;
#pragma unroll
        for (int s = 0; s < S; ++s)
            image[((size_t)r * S + s) * ld + c] = c < H ? ltg_f2bf(tanhf(acc[s] + b)) : (unsigned short)0;   // K padding written as zeros
    }
}

// the sum of a lane's value over the lanes that hold the other sample rows of the same (user, item): lane ^ 16 from S = 8, lane ^ 32 from
// S = 16.  a + b is commutative, so every lane of a group ends with the same bits.
template <int S>
__device__ __forceinline__ float po_lanes(float x) {
    if (S >= 8) x += __shfl_xor(x, 16);
    if (S >= 16) x += __shfl_xor(x, 32);
    return x;
}
__device__ __forceinline__ float po_sum4(const ltg_f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ float po_sq4(const ltg_f32x4 v, float m) {
    const float a = v[0] - m, b = v[1] - m, c = v[2] - m, d = v[3] - m;
    return (a * a + b * b) + (c * c + d * d);
}

// Workgroup (x, y) = sample rows [64 x, 64 x + 64) against item segment y ([y seg_len, (y + 1) seg_len) of the slab, seg_len % 256 == 0).
// The 64 image rows are resident in LDS in A-fragment order ([K step][row tile][lane] x 16 B: a wave's read is 1 KiB contiguous, no bank
// conflict); sample rows are the MFMA's M dimension, items its N dimension.  Per step every wave owns 4 x 16 items: it loads their B
// fragments global -> VGPR (16 B per lane, PO_PF K steps ahead of the MFMAs that use them) and runs 16 MFMAs per K step against 4 LDS
// reads.  Indices are clamped instead of branched on; rows >= M and items >= I are computed and not written.
// C/D map: col = lane & 15 (item), row = 4 (lane >> 4) + reg (sample row).  S divides 64 and blocks start at multiples of 64, so the S
// rows of a user lie in one block: in the 4 registers of a lane (S = 4), plus lane ^ 16 (8), plus lane ^ 32 (16), plus the next row tile (32).
// Two passes over the live values: mean = sum / S, var = sum (l - mean)^2 / S.
template <int S, bool SHADOW>
__global__ __launch_bounds__(PO_NT) void k_post_scores(int M, int I, int H, int ld, int seg_len, const unsigned short* __restrict__ img,
                                                       const unsigned short* __restrict__ Wb, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float beta, float* __restrict__ score,
                                                       float* __restrict__ spread) {
    extern __shared__ __attribute__((aligned(16))) ltg_u32x4 po_lds[];   // [ks_n][PO_RT][64] x 16 B
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int ks_n = ld / 32;
    const int m0 = blockIdx.x * PO_ROWS, seg_lo = blockIdx.y * seg_len, seg_hi = min(I, seg_lo + seg_len);
    for (int e = tid; e < ks_n * PO_RT * 64; e += PO_NT) {      // rows >= M mirror row M - 1 (their scores are not written)
        const int ln = e & 63, fr = e >> 6, rt = fr % PO_RT, ks = fr / PO_RT;
        const int row = min(m0 + 16 * rt + (ln & 15), M - 1);
        po_lds[e] = reinterpret_cast<const ltg_u32x4*>(img + (size_t)row * ld)[4 * ks + (ln >> 4)];
    }
    __syncthreads();                                             // (the only barrier: waves leave the loop below at different steps)
    const ltg_u32x4* Hl = po_lds + lane;
    const float inv_s = 1.f / (float)S;
    const int base0 = seg_lo + 64 * w;
    const int total = base0 < seg_hi ? (seg_hi - base0 + PO_STEP - 1) / PO_STEP * ks_n : 0;      // (item step, K step) pairs of this wave
    // the B fragments of pair L + PO_PF are requested while pair L multiplies: a ring of PO_PF register stages that runs on across the
    // item steps, so a step's first K steps are on their way while the step before it finishes (past the last pair it re-reads clamped rows)
    int pk = 0, pbase = base0;
    auto fetch = [&](ltg_u32x4(&dst)[PO_IT]) {
        const int k0 = 32 * pk + 8 * lq;
#pragma unroll
        for (int t = 0; t < PO_IT; ++t) {
            const int item = min(pbase + 16 * t + lr, I - 1);
            if (SHADOW) {
                dst[t] = *reinterpret_cast<const ltg_u32x4*>(Wb + (size_t)item * ST_KP + k0);
            } else {    // fp32 rows, rounded as the shadow rounds them (H % 4 == 0: a group of four is whole or absent)
                const float* p = W + (size_t)item * H;
                const float4 x = ltg_ld4(p, k0, H, true), y = ltg_ld4(p, k0 + 4, H, true);
                dst[t][0] = (unsigned)ltg_f2bf(x.x) | ((unsigned)ltg_f2bf(x.y) << 16);
                dst[t][1] = (unsigned)ltg_f2bf(x.z) | ((unsigned)ltg_f2bf(x.w) << 16);
                dst[t][2] = (unsigned)ltg_f2bf(y.x) | ((unsigned)ltg_f2bf(y.y) << 16);
                dst[t][3] = (unsigned)ltg_f2bf(y.z) | ((unsigned)ltg_f2bf(y.w) << 16);
            }
        }
        if (++pk == ks_n) {
            pk = 0;
            pbase += PO_STEP;
        }
    };
    ltg_u32x4 bq[PO_PF][PO_IT];
#pragma unroll
    for (int p = 0; p < PO_PF; ++p) fetch(bq[p]);
    ltg_f32x4 acc[PO_IT][PO_RT];
#pragma unroll
    for (int t = 0; t < PO_IT; ++t)
#pragma unroll
        for (int rt = 0; rt < PO_RT; ++rt) acc[t][rt] = ltg_f32x4{0.f, 0.f, 0.f, 0.f};
    int ks = 0, base = base0;
#pragma unroll 1
    for (int L0 = 0; L0 < total; L0 += PO_PF) {
#pragma unroll
        for (int p = 0; p < PO_PF; ++p) {
            if (L0 + p >= total) break;                          // (uniform over the wave)
            ltg_u32x4 bfr[PO_IT], afr[PO_RT];
#pragma unroll
            for (int t = 0; t < PO_IT; ++t) bfr[t] = bq[p][t];
            fetch(bq[p]);
#pragma unroll
            for (int rt = 0; rt < PO_RT; ++rt) afr[rt] = Hl[(ks * PO_RT + rt) * 64];
#pragma unroll
            for (int t = 0; t < PO_IT; ++t)
#pragma unroll
                for (int rt = 0; rt < PO_RT; ++rt)
                    acc[t][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ltg_bf16x8, afr[rt]),
                                                                         __builtin_bit_cast(ltg_bf16x8, bfr[t]), acc[t][rt], 0, 0, 0);
            if (++ks < ks_n) continue;
            // the item step is complete: reduce over the samples and store
#pragma unroll
            for (int t = 0; t < PO_IT; ++t) {
                const int it = base + 16 * t + lr;
                const bool ok = it < seg_hi;
                const float bv = bias[min(it, I - 1)];
                ltg_f32x4 l[PO_RT];
#pragma unroll
                for (int rt = 0; rt < PO_RT; ++rt) l[rt] = acc[t][rt] + bv;
                if (S == 1) {
#pragma unroll
                    for (int rt = 0; rt < PO_RT; ++rt)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int row = m0 + 16 * rt + 4 * lq + j;
                            if (ok && row < M) {
                                score[(size_t)row * I + it] = l[rt][j];
                                if (spread) spread[(size_t)row * I + it] = 0.f;
                            }
                        }
                } else if (S <= 16) {
#pragma unroll
                    for (int rt = 0; rt < PO_RT; ++rt) {
                        const float mean = po_lanes<S>(po_sum4(l[rt])) * inv_s;
                        const float sd = sqrtf(po_lanes<S>(po_sq4(l[rt], mean)) * inv_s);
                        const int row0 = m0 + 16 * rt + (S == 4 ? 4 * lq : S == 8 ? 8 * (lq >> 1) : 0);
                        const bool writer = S == 4 || (S == 8 ? (lq & 1) == 0 : lq == 0);
                        if (ok && writer && row0 < M) {
                            const size_t o = (size_t)(row0 / S) * I + it;
                            score[o] = fmaf(beta, sd, mean);
                            if (spread) spread[o] = sd;
                        }
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < PO_RT / 2; ++q) {
                        const float mean = (po_lanes<16>(po_sum4(l[2 * q])) + po_lanes<16>(po_sum4(l[2 * q + 1]))) * inv_s;
                        const float sd = sqrtf((po_lanes<16>(po_sq4(l[2 * q], mean)) + po_lanes<16>(po_sq4(l[2 * q + 1], mean))) * inv_s);
                        const int row0 = m0 + 32 * q;
                        if (ok && lq == 0 && row0 < M) {
                            const size_t o = (size_t)(row0 / S) * I + it;
                            score[o] = fmaf(beta, sd, mean);
                            if (spread) spread[o] = sd;
                        }
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < PO_IT; ++t)
#pragma unroll
                for (int rt = 0; rt < PO_RT; ++rt) acc[t][rt] = ltg_f32x4{0.f, 0.f, 0.f, 0.f};
            ks = 0;
            base += PO_STEP;
        }
    }
}

// One wave per (row, entry): the entry's W_p1t row in registers (bf16 values, 8 K per lane and half), then one dot product per sample
// against the image row, summed over the lanes by a fixed butterfly; sample s stays in lane s, and mean / std are taken over lanes 0 .. 31
// (lanes >= S hold 0).  Ids outside the slab and padding give 0.0 in both outputs: item shards add up under a sum all-reduce.
template <bool SHADOW>
__global__ __launch_bounds__(PO_NT) void k_post_entries(int n_ent, int k, int S, int I, int H, int ld, int item_lo,
                                                        const unsigned short* __restrict__ img, const unsigned short* __restrict__ Wb,
                                                        const float* __restrict__ W, const float* __restrict__ bias,
                                                        const int32_t* __restrict__ id_in, float* __restrict__ mean_out,
                                                        float* __restrict__ std_out) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * (PO_NT / 64) + (threadIdx.x >> 6);
    if (e >= n_ent) return;
    const int r = e / k, id = id_in[e], col = id - item_lo;
    if (id < 0 || col < 0 || col >= I) {
        if (lane == 0) {
            mean_out[e] = 0.f;
            std_out[e] = 0.f;
        }
        return;
    }
    float wv[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 8 * (lane + 64 * u) + j;
            float x = 0.f;
            if (kk < H) x = SHADOW ? __uint_as_float((unsigned)Wb[(size_t)col * ST_KP + kk] << 16) : __uint_as_float((unsigned)ltg_f2bf(W[(size_t)col * H + kk]) << 16);
            wv[u][j] = x;
        }
    const float bv = bias[col];
    float mine = 0.f;
    for (int s = 0; s < S; ++s) {
        const unsigned short* row = img + ((size_t)r * S + s) * ld;
        float p = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = 8 * (lane + 64 * u) + j;
                if (kk < H) p = fmaf(__uint_as_float((unsigned)row[kk] << 16), wv[u][j], p);
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
        if (lane == s) mine = p + bv;
    }
    float sum = mine;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)S;
    const float d = lane < S ? mine - mean : 0.f;
    float q = d * d;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (lane == 0) {
        mean_out[e] = mean;
        std_out[e] = sqrtf(q / (float)S);
    }
}
