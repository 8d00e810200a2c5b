// HIP kernels + C ABI (include/ltg.h) of the MI355X-native Long-Tail-GAN training path.
// gfx950 only.  Reference citations are relative to /root/reference/.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <stdint.h>

#include "../../include/ltg.h"
#include "ltg_gemm.h"
#include "ltg_rng.h"

namespace {

constexpr int NT = 256;

struct AdamC {
    float lr_t, b1, b2, eps;
};

// tf.train.AdamOptimizer update (train.py:160-164, Q5): m,v updated for EVERY element (dense).
// One element, with the rounding PINNED (explicit fma; `b1 m + (1-b1) g` may otherwise contract either way, kernel by
// kernel): every kernel that applies Adam -- dense sweeps, tile epilogues, the lazy clock of W_q0 -- yields the same bits
// for the same (p, m, v, g).
// p - lr_t m / (sqrt(v) + eps).  Default: the hardware's square root and reciprocal (v_sqrt_f32, v_rcp_f32: 1 ulp each, the
// quotient within ~2.5 ulp of the correctly rounded one -- 3e-7 of a step that is itself ~lr of the weight) instead of the IEEE
// sequences (~25 VALU instructions per element: what bounds the lazy clock's catch-up kernels and a fifth of the streaming weight
// update's issue slots).  The product with the reciprocal and the subtraction are ONE explicit fma: left to the compiler,
// `p - lm * r` contracts in one kernel and not in another.  -DLTG_ADAM_IEEE builds the correctly rounded form (A/B:
// scripts/build_variant.sh).  Every Adam update of the library goes through this one function, so dense sweep == lazy clock
// bit for bit either way.
__device__ __forceinline__ float adam_move(const float p, const float lm, const float v, const float eps) {
#ifdef LTG_ADAM_IEEE
    return p - lm / (sqrtf(v) + eps);
#else
    return __builtin_fmaf(-lm, __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) + eps), p);
#endif
}
__device__ __forceinline__ void adam1(float& p, float& m, float& v, const float g, const float lr_t, const AdamC& c) {
    m = __builtin_fmaf(c.b1, m, (1.f - c.b1) * g);
    v = __builtin_fmaf(c.b2, v, ((1.f - c.b2) * g) * g);
    p = adam_move(p, lr_t * m, v, c.eps);
}
__device__ __forceinline__ void adam_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                            size_t i, float g, const AdamC c) {
    float pn = p[i], mn = m[i], vn = v[i];
    adam1(pn, mn, vn, g, c.lr_t, c);
    m[i] = mn;
    v[i] = vn;
    p[i] = pn;
}

__device__ __forceinline__ float block_sum(float x, float* red /*[NT/64]*/) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ float block_max(float x, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) s = fmaxf(s, red[i]);
    return s;
}

// ---- device-side hand-over between the two streams of the one-call step (include/ltg.h: ltg_pipe.sync).  A cross-stream event costs
// ~12 us per direction on this pool (scripts/micro/sync_cost.hip: hipEventRecord + hipStreamWaitEvent between two 10-us kernels) and
// ~6 us of bubble on the recording stream; a word in device memory costs the consumer one poll.  A gate is a 32-bit sequence number:
// the producer stores the call's ordinal, the consumer waits until the word has reached it (wrap-safe compare).  Every wait is bounded
// (30 s, counted in ltg_pipe.sync[2]): a call that failed half-way leaves a waiter behind, not a hung GPU.
// The two streams must be CONCURRENT: HIP maps streams onto a few hardware queues, and a waiter in front of its producer in one queue
// waits for ever -- ltg_g_pipe_probe tests a pair of streams for that.
struct LtgGate {
    unsigned* word;   // NULL: no gate
    unsigned seq;
    unsigned* expired;   // counts the waits that gave up (ltg_pipe.sync[2]: the host checks it when it joins the pipe)
    int limit;           // milliseconds before a wait gives up (0: 30 s)
};
#define LTG_NO_GATE LtgGate{nullptr, 0u, nullptr, 0}
// acquire = false: the consumer only needs to run AFTER the producer (a write-after-read hazard), it reads nothing the producer wrote --
// no cache invalidation (dec-0: 14.7 -> ~8 us; whoever reads the producer's data later does so behind a kernel boundary)
__device__ __forceinline__ bool ltg_poisoned_word(const unsigned* p) {
    return p && __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}
__device__ __forceinline__ void ltg_gate_wait(LtgGate g, bool acquire = true) {   // first statement of a consumer kernel; every thread calls
    if (!g.word) return;
    if (threadIdx.x == 0) {
        bool open = false;
        const unsigned long long ticks = (unsigned long long)(g.limit > 0 ? g.limit : 30000) * 100000ull;   // wall_clock64: 100 MHz
        const unsigned long long t0 = wall_clock64();
        bool dead = false;     // the pipe is poisoned already: nothing behind this wait will touch the model, so nothing is waited for
        while (!open) {
            open = (int)(__hip_atomic_load(g.word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - g.seq) >= 0;
            dead = ltg_poisoned_word(g.expired);
            if (open || dead || wall_clock64() - t0 > ticks) break;
            __builtin_amdgcn_s_sleep(8);
        }
        if (!open && !dead && g.expired) atomicAdd(g.expired, 1u);
    }
    __syncthreads();
    if (acquire) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
// The same wait as the LAST thing ONE thread of a kernel does: the kernel behind it on the stream starts in stream order, i.e. after this
// one has ended, so that kernel is gated whatever its size while a single wave of the whole device spins (no workgroup of a large
// launch ever occupies a CU polling for a producer that still needs one: forward progress by construction).  A wait that gives up
// POISONS the pipe (word 2 != 0): the kernels behind it skip their work (ltg_poisoned) and the host raises when it next looks.
__device__ __forceinline__ void ltg_gate_wait_tail(LtgGate g) {
    if (!g.word) return;
    const unsigned long long ticks = (unsigned long long)(g.limit > 0 ? g.limit : 30000) * 100000ull;   // wall_clock64: 100 MHz
    const unsigned long long t0 = wall_clock64();
    bool open = false, dead = false;
    while (!open) {
        open = (int)(__hip_atomic_load(g.word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - g.seq) >= 0;
        dead = ltg_poisoned_word(g.expired);     // (poisoned already: the kernels behind this wait return at once -- nothing to wait for)
        if (open || dead || wall_clock64() - t0 > ticks) break;
        __builtin_amdgcn_s_sleep(8);
    }
    if (!open && !dead && g.expired) atomicAdd(g.expired, 1u);
}
// word 2 of ltg_pipe.sync: a device-side wait of this pipe has given up -- nothing that follows may touch the model
// (round 5: a PLAIN load -- the scalar unit's, see ltg_poison_word below for why that is enough -- instead of an agent-scope atomic one: the
// guard is the first statement of its kernels, and as a vector load it was a ~1-us round trip in front of every other request)
// (round 6: the pointer is NOT __restrict__ -- waiters on other streams atomicAdd this word while the kernel runs, so a noalias promise would be
// false.  The guarantee is stated as what it is: a kernel sees every expiry that happened before it STARTED (its dispatch acquires); an expiry
// DURING the kernel is seen from the next kernel boundary on.  That is all the design needs: the wait that gates a kernel sits in front of it
// on its own stream.)
__device__ __forceinline__ bool ltg_poisoned(const unsigned* p) { return p && *p != 0u; }
// The word itself, for kernels that REQUEST it first and look at it in front of their first store (round 5): `if (ltg_poisoned(p)) return;`
// as a kernel's first statement is a vector-memory round trip of its own in front of every other request.  A PLAIN load of a uniform address
// before the kernel's first store: the compiler issues it on the SCALAR unit (s_load_dword, beside the kernel-argument loads), so nothing in
// the vector-memory queue waits for it.  Plain is enough here: every poisoner is a wait that sits IN FRONT of the reading kernel on its own
// stream (a kernel's end releases, a kernel's start acquires); a wait on another stream that gives up while this kernel runs is seen by the
// next kernel, as with the atomic load.
__device__ __forceinline__ unsigned ltg_poison_word(const unsigned* p) { return p ? *p : 0u; }
__device__ __forceinline__ bool ltg_word_set(unsigned w) { return w != 0u; }
// by ONE thread.  Every producer in this library is a WHOLE KERNEL that ended in front of the kernel that stores the word (the store
// is the first thing a kernel does when it starts, or a one-wave kernel of its own behind the producer), and the end of a kernel is
// already the device-wide release of what it wrote; the agent-scope release below is belt and braces -- measured in round 4 against a
// build without it: bit-identical over 3 400 soak steps and no timing difference (profiles/r4_ab_gate_fence.txt), so it stays.
__device__ __forceinline__ void ltg_gate_set(LtgGate g) {
    if (!g.word) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_store(g.word, g.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one wave in front of the side stream's work: returns when the gate opens (the kernels behind it start in stream order)
// (set_first: a gate this kernel opens when it starts -- whatever preceded it on its stream is complete)
__global__ __launch_bounds__(64) void k_gate_wait(LtgGate g, LtgGate set_first = LTG_NO_GATE) {
    if (threadIdx.x == 0) ltg_gate_set(set_first);
    ltg_gate_wait(g);
}
// one wave behind the side stream's work: opens the gate
__global__ __launch_bounds__(64) void k_gate_set(LtgGate g, LtgGate g2 = LTG_NO_GATE) {
    if (threadIdx.x == 0) {
        ltg_gate_set(g);
        ltg_gate_set(g2);
    }
}


#include "ltg_gen_fwd.h"
#include "ltg_stream.h"
#include "ltg_disc.h"
#include "ltg_gstep.h"
#include "ltg_clock.h"
#include "ltg_sampler.h"
#include "ltg_topk.h"
#include "ltg_explore.h"
#include "ltg_posterior.h"
#include "ltg_replay.h"
#include "ltg_audience.h"
#include "ltg_cap.h"
#include "ltg_floor.h"
#include "ltg_share.h"
#include "ltg_longtail.h"
#include "ltg_neighbors.h"
#include "ltg_companions.h"
#include "ltg_diversify.h"
#include "ltg_explain.h"
#include "ltg_calibrate.h"
#include "ltg_critic.h"

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// a hand-over word of ltg_pipe.sync / ltg_d_opts.sync (include/ltg.h: enum ltg_word) as the gate a kernel stores `seq` to ...
inline LtgGate gate_store(uint32_t* sync, int word, unsigned seq) { return LtgGate{sync + word, seq, nullptr, 0}; }
// ... or polls for `seq` in (a poll that gives up counts in the poison word)
inline LtgGate gate_poll(uint32_t* sync, int word, unsigned seq) { return LtgGate{sync + word, seq, sync + LTG_WORD_POISON, 0}; }

// Which of the round-2 latency-path kernels (ltg_fast.h) apply.  Tuning-knob bit 18 of ltg_config.tuning switches all of
// them off (the round-1 kernels compute the same function; kept for A/B measurements and as the path of unusual sizes).
inline bool fast_on(const ltg_config* c) { return (c->tuning & (1 << 18)) == 0; }
// the wide discriminator (BASELINE config 5's shape): its GEMMs are throughput-bound, the generic kernels' large tiles serve it
inline bool d_wide(const ltg_config* c) { return c->d_h0 >= 512 && c->d_h1 + c->d_h2 >= 512 && c->d_h3 >= 128; }

constexpr int DH2_NH = 2;   // column halves of the streaming dh2 product (k_dh2_stream<.., NH>)
// The item dimension of the dh2 product cut into partial [B][H] slabs (summed by k_da2): items per slab and their number.  The route of
// a step (g_route) and the workspace (carve) both take it from here.
struct Dh2Split {
    int chunk, nsplit;
};
inline Dh2Split dh2_split(int I, bool stream) {
    int c;
    if (stream) {
        // items per workgroup of k_dh2_stream = one partial [B][H] slab each: up to 256 workgroups, but at least 4 tiles per
        // workgroup -- at 20 000 items 157 slabs instead of 209 (each slab is 240 KB written and read once more by k_da2)
        c = (I + 255) / 256;
        c = (c + ST_BN - 1) / ST_BN * ST_BN;
        c = DH2_NH * (c < 4 * ST_BN ? 4 * ST_BN : c);
    } else {
        // split the item dimension so that ~128 workgroups x (H/64) share the reduction
        c = (I + 63) / 64;
        c = (c + 31) / 32 * 32;
        if (c < 256) c = 256;
    }
    return Dh2Split{c, (I + c - 1) / c};
}

// rows of the sparse W_q0 gradient = distinct items of a batch <= min(n_items, nnz of the batch).  The workspace is sized
// without knowing nnz, so the table bound is used: one heavy user in a short batch can never overflow it.
inline size_t gq0_rows(const ltg_config* cfg, int /*max_rows*/) { return (size_t)cfg->n_items; }

constexpr int RD_MAXI = 4096;   // "small item slab": a row of logits fits the registers of one workgroup (ltg_fast.h)
struct Workspace {
    // generator backward
    float *rowpart, *segpart, *nb, *Pb, *scal, *dlog, *part, *dh2, *da2, *dmlv, *da1, *gq0;
    int32_t* slotmap;   // [I] item -> gradient row of the current batch (only used when the caller passes no slot[] cache)
    // discriminator
    float *A1, *A3, *y, *ds, *lrow, *dpre1, *dpre3, *slab;
    // fast path: per-column-tile partial dot products of the output unit, w4 * dA3/dpre, per-row loss terms of the G step
    float *spart, *G3, *rowout, *xd;
    uint8_t* A1_8;      // the branch layers' output in e4m3 (fp8 operand storage of the wide discriminator)
    // operand-format storage of the fp8 backward (ltg_fp8bwd.h): transposed / row-major e4m3 copies, pair rows padded to np8
    uint8_t *A1T_8, *dpre3_8, *dpre3T_8, *dpre1T_8, *ET_8;
    unsigned short* dA1T_16;
    int np8;
    float* wsp;         // the discriminator's weights split into bf16 terms in MFMA fragment order (ltg_tower.h), rebuilt by every forward-only tower
    size_t bytes;
};
// stride of one discriminator gradient slab: the P gradients + one slot for the chunk's loss sum, padded to whole float4
inline int d_slab_stride(int P) { return (P + 1 + 3) & ~3; }

// geometry of the one-kernel forward-only tower (ltg_tower.h)
constexpr int FT_BM = 64, FT_NT = 512;
constexpr int FT_KP1_MAX = 4;       // h0 <= 128: the gathered embedding rows of a wave stay in registers, split
inline int ft_lda(int h12) { return ((h12 + 31) & ~31) + 4; }      // floats; = 4 mod 32: the 16 rows of a ds_read_b128 fragment read hit every bank once
inline size_t ft_lds_bytes(int h12) { return ((size_t)FT_BM * ft_lda(h12) + 4 * FT_BM) * sizeof(float); }
// fragment triples (3 KiB each) of the three split matrices
inline size_t ft_wsp_triples(int h0, int h1, int h2, int h3) {
    const size_t kp1 = (h0 + 31) / 32, kp3 = (h1 + h2 + 31) / 32;
    return (size_t)((h1 + 15) / 16) * kp1 + (size_t)((h2 + 15) / 16) * kp1 + (size_t)((h3 + 15) / 16) * kp3;
}
inline size_t ft_wsp_bytes(int h0, int h1, int h2, int h3) { return ft_wsp_triples(h0, h1, h2, h3) * 3 * 1024; }
// sizes the one-kernel forward-only tower (ltg_tower.h) serves: the latency path's fp32 discriminator with h0 <= 128 (a wave's gathered rows stay in
// registers), h3 <= 320 (five 16-column tiles per wave column) and A1 [64][h1 + h2] within the LDS.  The choice depends on the layer sizes and
// d_arith only, so the tower inside a step and the batched tower run the same kernel and produce the same bits.
inline bool ft_wsp_capable(const ltg_config* c) {
    return fast_on(c) && c->d_precision == LTG_PREC_FP32 && !d_wide(c) && c->d_h0 >= 4 &&
           c->d_h0 <= 32 * FT_KP1_MAX && (c->d_h0 % 4) == 0 && c->d_h1 >= 1 && c->d_h2 >= 1 && c->d_h3 >= 1 && c->d_h3 <= 320 &&
           ft_lds_bytes(c->d_h1 + c->d_h2) <= (size_t)160 * 1024;
}
Workspace carve(const ltg_config* cfg, int max_rows, int max_pairs, char* base) {
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t nfloat) {
        float* p = reinterpret_cast<float*>(base + off);
        off += align_up(nfloat * sizeof(float));
        return p;
    };
    const size_t R = (size_t)max_rows, I = (size_t)cfg->n_items, H = (size_t)cfg->h_enc, Z = (size_t)cfg->z_dim;
    const size_t P = (size_t)max_pairs, h12 = (size_t)cfg->d_h1 + cfg->d_h2, h3 = (size_t)cfg->d_h3;
    // (sized without a generator state: whichever form of the dh2 product the step's route takes)
    const size_t nsplit = (size_t)std::max(dh2_split(cfg->n_items, false).nsplit, dh2_split(cfg->n_items, true).nsplit);
    w.rowpart = take(R * RP);
    w.segpart = take(segpart_floats(I, R));
    w.nb = take(R);
    w.Pb = take(R);
    w.scal = take(16);
    w.dlog = take(R * I);
    w.part = take(nsplit * R * H);
    w.dh2 = take(R * H);
    w.da2 = take(R * H);
    w.dmlv = take(R * 2 * Z);
    w.da1 = take(R * H);
    w.gq0 = take((size_t)(gq0_rows(cfg, max_rows) + ENC0_BIAS_PARTS) * H);   // sparse gradient rows of W_q0 (+ partial bias rows)
    w.slotmap = reinterpret_cast<int32_t*>(take(I));
    w.A1 = take(P * h12);
    w.A3 = take(P * h3);
    w.y = take(P);
    w.ds = take(P);
    w.lrow = take(P);
    w.dpre1 = take(P * h12);
    w.dpre3 = take(P * h3);
    {
        const DLayout L = d_layout(cfg->d_h0, cfg->d_h1, cfg->d_h2, cfg->d_h3);
        const size_t ks = (P + D_KCHUNK - 1) / D_KCHUNK;
        w.slab = take(ks * (size_t)d_slab_stride(L.off[8]));
    }
    w.spart = take((((h3 + 31) / 32) + 1) * P);   // per-tile partial dot products of the output unit: 32-column tiles, or 2 strips per 64-column tile
    w.G3 = take(P * h3);
    w.rowout = take(R * 4);
    w.xd = take(I <= (size_t)RD_MAXI ? R * I : 1);   // dense operand rows of enc-0 (small item slabs)
    w.A1_8 = reinterpret_cast<uint8_t*>(take((P * h12 + 3) / 4));
    {
        const bool f8 = cfg->d_precision == LTG_PREC_FP8;      // (only that mode carries these buffers)
        const size_t np = ((P + 127) / 128 * 128), h0 = (size_t)cfg->d_h0;
        auto take8 = [&](size_t nbytes) { return reinterpret_cast<uint8_t*>(take(f8 ? (nbytes + 3) / 4 : 1)); };
        w.np8 = (int)np;
        w.A1T_8 = take8((h12 + 1) * np);
        w.dA1T_16 = reinterpret_cast<unsigned short*>(take8(2 * h12 * np));   // dA1 / dpre1 of the branch layers, bf16, transposed (ltg_fp8bwd.h)
        w.dpre3_8 = take8(P * h3);
        w.dpre3T_8 = take8(h3 * np);
        w.dpre1T_8 = take8(h12 * np);
        w.ET_8 = take8(2 * (h0 + 1) * np);
    }
    w.wsp = take(ft_wsp_capable(cfg) ? ft_wsp_bytes(cfg->d_h0, cfg->d_h1, cfg->d_h2, cfg->d_h3) / sizeof(float) : 1);
    w.bytes = off;
    return w;
}

inline AdamC make_adam(const ltg_config* cfg, int t) {
    AdamC a;
    const double b1 = cfg->beta1, b2 = cfg->beta2;
    a.lr_t = (float)((double)cfg->lr * sqrt(1.0 - pow(b2, (double)t)) / (1.0 - pow(b1, (double)t)));
    a.b1 = cfg->beta1;
    a.b2 = cfg->beta2;
    a.eps = cfg->adam_eps;
    return a;
}

struct Probe {
    const ltg_probe* p;
    hipStream_t st;
    inline void before(int id) const {
        if (p && p->kernel_id == id && p->ev_start) (void)hipEventRecord((hipEvent_t)p->ev_start, st);
    }
    inline void after(int id) const {
        if (p && p->kernel_id == id && p->ev_stop) (void)hipEventRecord((hipEvent_t)p->ev_stop, st);
    }
};
#define LTG_PROBED(pr, id, stmt) \
    do {                         \
        (pr).before(id);         \
        stmt;                    \
        (pr).after(id);          \
    } while (0)

inline int check_launch() { return hipGetLastError() == hipSuccess ? LTG_OK : LTG_ELAUNCH; }
// hipGetLastError is sticky across unrelated runtime calls of the host program: clear it on entry
inline void clear_errors() { (void)hipGetLastError(); }

inline dim3 grid2(int N, int M, int bn = 64, int bm = 64, int z = 1) { return dim3((N + bn - 1) / bn, (M + bm - 1) / bm, z); }
// workgroups of NT threads for n elements, at most `cap` of them (grid-stride kernels)
inline dim3 grid1(int n, int cap) { return dim3((n + NT - 1) / NT < cap ? (n + NT - 1) / NT : cap); }

}  // namespace
namespace {
#include "ltg_fast.h"
#include "ltg_fp8bwd.h"
#include "ltg_tower.h"
#include "ltg_oneshot.h"
}
namespace {

#define LTG_D_SPL_LAUNCH(SPLV, KERNEL, ...)                                       \
    do {                                                                          \
        if ((SPLV) == 6) hipLaunchKernelGGL((KERNEL<6>), __VA_ARGS__);            \
        else if ((SPLV) == 4) hipLaunchKernelGGL((KERNEL<4>), __VA_ARGS__);       \
        else hipLaunchKernelGGL((KERNEL<0>), __VA_ARGS__);                        \
    } while (0)

// ltg_config.tuning: the selection bits include/ltg.h lists; a configuration with any other bit is refused
constexpr int32_t TUNING_BITS = (1 << 14) | (1 << 17) | (1 << 18) | (1 << 19) | (1 << 20) | (1 << 21) | (1 << 22) | (1 << 26);
bool cfg_ok(const ltg_config* c) {
    return c && c->n_items > 0 && c->h_enc > 0 && c->h_enc <= 768 && (c->h_enc % 4) == 0 && c->z_dim > 0 &&
           c->d_h0 >= 1 && c->d_h1 >= 1 && c->d_h2 >= 1 && c->d_h3 >= 1 &&      // (a layer of width 0 has no tile to launch: refused, not computed)
           (c->precision == LTG_PREC_BF16 || c->precision == LTG_PREC_FP32) && c->d_precision >= 0 && c->d_precision <= LTG_PREC_FP8 &&
           c->d_arith >= 0 && (c->d_arith & 3) <= LTG_DARITH_BF16X4 && (c->d_arith & ~0xF3) == 0 && (c->tuning & ~TUNING_BITS) == 0;
}

inline int Ig_of(const ltg_config* cfg) { return cfg->n_items_global > 0 ? cfg->n_items_global : cfg->n_items; }

// lazy Adam clock of W_q0 (ltg_gen_state.q0_last): usable when the caller supplies clock, history ring and a period
inline bool q0_lazy(const ltg_config* cfg, const ltg_gen_state* gen) {
    return gen->q0_last && gen->q0_lr_hist && gen->q0_period >= 1 && gen->q0_period <= LTG_Q0_HIST / 2 && gen->q0_ord >= 0 && (cfg->h_enc % 4) == 0 &&
           cfg->n_items >= 8192;   // smaller slabs update W_q0 as a dense product: nothing to defer
}

// ---- the generator's route: which kernel every stage of a step over `rows` batch rows runs.  A pure function of its arguments, computed
// once per call; the stages switch on the fields and test nothing themselves.  (ltg_g_route hands it out: include/ltg.h has the fields.)
// staged: the step cut at its exchange points (ltg_g_fwd_* / ltg_g_bwd_*), which has no small-slab form.
ltg_g_route_info g_route(const ltg_config* c, const ltg_gen_state* gen, int rows, bool staged = false) {
    ltg_g_route_info r = {};
    const int I = c->n_items, H = c->h_enc;
    const bool fast = fast_on(c), bf = c->precision == LTG_PREC_BF16, big = I >= 8192;
    const bool vz = (c->z_dim % 4) == 0;   // 16-B loaders of the middle layers (H % 4 == 0 always)
    const bool unsharded = c->item_lo == 0 && (c->n_items_global == 0 || c->n_items_global == I);
    r.enc0 = fast ? LTG_ENC0_FAST : LTG_ENC0_GENERIC;
    // small item slab: a row's softmax statistics, loss terms and dlogits need no other row -> one launch per stage
    r.small = !staged && fast && unsharded && I <= RD_MAXI && (I % 4) == 0 && vz && rows <= 256;
    r.mid = (fast && vz && rows <= 256) ? LTG_MID_FAST : LTG_MID_DENSE;
    r.mid_vec = vz;
    // the streaming decoder kernels: bf16, large item slab, a training batch (<= 128 rows), H <= 608, 16-B aligned rows
    const bool stream = gen->wp1t_bf16 && bf && big && (I % 8) == 0 && rows <= 128 && H <= ST_KP && (H % 4) == 0;
    // k_dec1_bwd_adam_stream walks the 4 H/4 float4 a wave owns per tile as exactly ten 64-lane accesses
    const bool dw_stream = stream && (H % 4) == 0 && H > 576 && H <= 640;
    if (fast && I <= RD_MAXI && rows <= 256) r.dec = LTG_DEC_SMALL;
    else if (stream) {
        // the second form for the HBM-bound slabs (see k_dec1_fwd_stream2); tuning-knob bit 26: the first form at every size, bit 17: the second
        // form from 8 192 items (A/B measurements)
        const int st2_min = (c->tuning & (1 << 17)) ? 8192 : ST2_MIN_ITEMS;
        // (the second form addresses the logits AND the shadow rows with 32-bit byte offsets from a uniform base: R * I * 4 and I * ST_KP * 2 must both
        // stay below 2^32 -- 3 532 110 items of one slab for the shadow; beyond either limit the first form, which has none)
        const bool form2 = (c->tuning & (1 << 26)) == 0 && I >= st2_min && (size_t)rows * (size_t)I < ((size_t)1 << 30) &&
                           (size_t)I * (size_t)(ST_KP * 2) < ((size_t)1 << 32);
        r.dec = form2 ? LTG_DEC_STREAM2 : LTG_DEC_STREAM1;
    } else {
        r.dec = LTG_DEC_TILE;
        r.dec_tile = big ? 128 : 32;
    }
    // (tuning-knob bit 21: statistics from a second pass over the logits)
    r.seg_pass = I > 2 * RS_SEG;
    r.stats = (stream && (c->tuning & (1 << 21)) == 0) ? LTG_STATS_EPILOGUE : (r.seg_pass ? LTG_STATS_SEGMENT : LTG_STATS_ROW);
    r.loss = r.small ? LTG_LOSS_ROW : (fast ? LTG_LOSS_COMBINE : LTG_LOSS_GENERIC);
    // dlog as bf16: when BOTH its consumers are the streaming kernels (k_dh2_stream, k_dec1_bwd_adam_stream + ragged tail); tuning-knob bit 22: fp32
    r.dlog_bf16 = fast && dw_stream && (c->tuning & (1 << 22)) == 0;
    if (r.small) r.dh2 = LTG_DH2_SMALL;
    else {
        r.dh2 = stream ? LTG_DH2_STREAM : LTG_DH2_PARTIAL;
        if (!stream) r.dh2_tile = big ? 128 : ((bf && (I % 4) == 0) ? -32 : 32);
        const Dh2Split s = dh2_split(I, stream);
        r.dh2_chunk = s.chunk;
        r.dh2_nsplit = s.nsplit;
    }
    if (r.small) r.dw = LTG_DW_TAIL_JOB;
    else if (dw_stream) {
        r.dw = LTG_DW_STREAM;
        r.dw_ragged = (I % 32) != 0;   // ragged tail: the generic tile kernel on the last I % 32 item rows
    } else {
        r.dw = LTG_DW_TILE;
        r.dw_tile = big ? 64 : ((bf && (I % 4) == 0) ? -32 : 32);
    }
    r.q0 = r.small ? LTG_Q0_DENSE : (q0_lazy(c, gen) ? LTG_Q0_LAZY : LTG_Q0_SWEEP);
    // HBM-bound sweep: its own launch at full occupancy (measured 490 vs 525 us at 200 000 items when it rode in the 118-register job
    // kernel); the generic chain's sweep always is one
    r.q0_own_launch = r.q0 == LTG_Q0_LAZY || (r.q0 == LTG_Q0_SWEEP && (big || r.mid == LTG_MID_DENSE));
    r.grad_rows = (c->tuning & (1 << 14)) == 0;   // tuning-knob bit 14: the column-blocked shape of the sparse gradient
    r.sharded_ok = r.mid == LTG_MID_FAST && r.dlog_bf16 && r.q0 == LTG_Q0_LAZY;
    return r;
}

// the item rows this batch reads, up to the caller's clock (no-ops for rows that are current)
void q0_touch(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_g_route_info& r, const ltg_batch* bt, hipStream_t st, const unsigned* poison = nullptr,
              int32_t* mark = nullptr, unsigned seq = 0u) {
    if (r.q0 != LTG_Q0_LAZY || bt->n_rows <= 0) return;
    const AdamC ad = make_adam(cfg, 1);   // b1, b2, eps; the learning rates come from the history ring
    if (bt->uptr && bt->csr_pos) {
        if (bt->n_unique > 0)
            hipLaunchKernelGGL(k_q0_touch_unique, dim3(bt->n_unique), dim3(Q0_NT), 0, st, cfg->h_enc, bt->n_unique, bt->uptr, bt->csr_pos, bt->indices, bt->uitem,
                               gen->q0_ord, *gen, ad, poison, mark, seq);
    } else {
        hipLaunchKernelGGL(k_q0_touch_rows, dim3(bt->n_rows), dim3(Q0_NT), 0, st, cfg->h_enc, bt->n_rows, bt->indptr, bt->indices, gen->q0_ord, *gen, ad);
    }
}

// stage 1: enc-0 over this rank's item slab.  pre_only: leave the partial pre-activation in acts->h1.
struct Enc0Fwd {
    float* xd = nullptr;              // small slabs: the dense operand rows for the backward's W_q0 product as well
    bool touched = false;             // the caller ran the lazy clock's catch-up itself
    LtgGate started = LTG_NO_GATE;    // stored when the kernel starts
    LtgGate end_wait = LTG_NO_GATE;   // polled by one more block row, as the last thing the launch does
};
void fwd_stage_enc(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_g_route_info& r, const ltg_batch* bt, const ltg_fwd_opts* o,
                   const ltg_gen_acts* acts, int pre_only, hipStream_t st, const Enc0Fwd& a = {}) {
    const int R = bt->n_rows, I = cfg->n_items, H = cfg->h_enc;
    const Probe pr{o->probe, st};
    float* const xd = a.xd;
    const LtgGate end_wait = a.end_wait;
    if (!a.touched) q0_touch(cfg, gen, r, bt, st);
    if (r.enc0 == LTG_ENC0_FAST) {
        LTG_PROBED(pr, LTG_K_ENC0_FWD,
                   hipLaunchKernelGGL(fk_enc0_fwd, dim3((H / 4 + 63) / 64, R + (end_wait.word ? 1 : 0)), dim3(ENC_NT), xd ? (size_t)I * sizeof(float) : 0, st, H, I, bt->indptr,
                                      bt->indices, bt->values, o->drop_keep, o->keep_prob, cfg->seed, o->rng_step, gen->p[0], gen->p[4], acts->h1,
                                      acts->row_scale, bt->row_norm2, cfg->item_lo, Ig_of(cfg), pre_only, xd, o->rows_per_step, a.started, end_wait));
        return;
    }
    LTG_PROBED(pr, LTG_K_ENC0_FWD,
               hipLaunchKernelGGL(k_enc0_fwd, dim3(R), dim3(ENC_NT), (size_t)ENC_NW * H * sizeof(float), st, H, I, bt->indptr, bt->indices,
                                  bt->values, o->drop_keep, o->keep_prob, cfg->seed, o->rng_step, gen->p[0], gen->p[4], acts->h1,
                                  acts->row_scale, bt->row_norm2, cfg->item_lo, Ig_of(cfg), pre_only, o->rows_per_step));
}

// the streaming decoder forward (LTG_DEC_STREAM1 / LTG_DEC_STREAM2): logits of R <= 128 rows over the local slab; stat != NULL: per-group
// softmax statistics as well.  Returns the number of statistic groups.
// (Round 4, built and not run: 64-item tiles with the eight waves as 4 row groups x 2 item halves -- a wave then owns 32 batch rows, so
// every B fragment it reads from LDS feeds two MFMAs: half the LDS bytes per FLOP, the untested suspect for this kernel's 0.46 of the
// HBM rate -- needs two stationary fragment sets = 152 registers per lane: hipcc allocates 256 VGPRs + 776 bytes of scratch per lane for
// it as written, i.e. the variant spills in its inner loop; it would need SGPR-base addressing throughout to fit.)
// (Measured and not kept, round 3: the same loop as TWO independent 4-wave workgroups per CU -- half the batch rows each, 2 x 77 KB of
// LDS, 244 VGPRs, bit-identical outputs -- so that one half's loads overlap the other's MFMAs and stores: 110.4 vs 107.9 us per launch
// at 200 000 items on one box, min 81.8 vs 78.6; whole step 968-970 vs 965-968 us.  The serialisation is not inside the workgroup.)
int launch_dec1_fwd_stream(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_g_route_info& r, int R, const ltg_gen_acts* acts, float* stat, hipStream_t st) {
    const int I = cfg->n_items, H = cfg->h_enc;
    if (r.dec == LTG_DEC_STREAM2) {
        const int nt2 = (I + 31) / 32, G2 = nt2 < 256 ? nt2 : 256;
#define LTG_ST2(STATS, NTB) hipLaunchKernelGGL((k_dec1_fwd_stream2<STATS, NTB>), dim3(G2), dim3(ST_NT), (size_t)ST_KS * NTB * 64 * 16, st, R, I, H, acts->h2, gen->wp1t_bf16, gen->p[7], acts->logits, stat)
        if (stat) { if (R <= 112) LTG_ST2(true, 7); else LTG_ST2(true, 8); }
        else { if (R <= 112) LTG_ST2(false, 7); else LTG_ST2(false, 8); }
#undef LTG_ST2
        return G2;
    }
    const int ntiles = (I + ST_BN - 1) / ST_BN, G = ntiles < 256 ? ntiles : 256;
    const size_t lds = (size_t)2 * ST_BN * ST_LDW * 2;
    if (stat) hipLaunchKernelGGL(k_dec1_fwd_stream<true>, dim3(G), dim3(ST_NT), lds, st, R, I, H, acts->h2, gen->wp1t_bf16, gen->p[7], acts->logits, stat);
    else hipLaunchKernelGGL(k_dec1_fwd_stream<false>, dim3(G), dim3(ST_NT), lds, st, R, I, H, acts->h2, gen->wp1t_bf16, gen->p[7], acts->logits, (float*)nullptr);
    return G;
}

// stage 2: (bias + tanh of the all-reduced pre-activation,) enc-1, reparameterisation, dec-0, dec-1 over the local slab
// stat (optional scratch of segpart_floats()): the streaming decoder kernel leaves its per-workgroup softmax statistics there;
// returns the number of workgroups that wrote them (0: the caller reads the logits for the statistics)
int fwd_stage_rest(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_g_route_info& r, const ltg_batch* bt, const ltg_fwd_opts* o,
                   const ltg_gen_acts* acts, int apply_bias_tanh, hipStream_t st, float* stat = nullptr) {
    int stat_groups = 0;
    const int R = bt->n_rows, I = cfg->n_items, H = cfg->h_enc, Z = cfg->z_dim;
    const Probe pr{o->probe, st};
    const bool vz = r.mid_vec != 0;
    if (apply_bias_tanh) {
        hipLaunchKernelGGL(k_bias_tanh, grid1(R * H, 1024), dim3(NT), 0, st, R * H, H, gen->p[4], acts->h1);
    }
    if (r.mid == LTG_MID_FAST) {
        LTG_PROBED(pr, LTG_K_ENC1, hipLaunchKernelGGL(fk_enc1<false>, grid2(Z, R, 16, 16), dim3(ENC1_NT), 0, st, R, H, Z, acts->h1, gen->p[1], gen->p[5], o->eps, o->is_training,
                                                      cfg->seed, o->rng_step, acts->mulv, acts->z));
        LTG_PROBED(pr, LTG_K_DEC0, hipLaunchKernelGGL(fk_dec0, grid2(H, R, 16, 16), dim3(NT), 0, st, R, H, Z, acts->z, acts->mulv, gen->p[2], gen->p[6],
                                                      acts->kl_rows, acts->h2));
    } else {
    pr.before(LTG_K_ENC1);
    if (vz) hipLaunchKernelGGL((k_dense_fwd<0, true>), grid2(2 * Z, R, 32, 32), dim3(NT), 0, st, R, 2 * Z, H, acts->h1, gen->p[1], gen->p[5], acts->mulv);
    else hipLaunchKernelGGL((k_dense_fwd<0, false>), grid2(2 * Z, R, 32, 32), dim3(NT), 0, st, R, 2 * Z, H, acts->h1, gen->p[1], gen->p[5], acts->mulv);
    pr.after(LTG_K_ENC1);
    hipLaunchKernelGGL(k_reparam, dim3(R), dim3(NT), 0, st, Z, acts->mulv, o->eps, o->is_training, cfg->seed, o->rng_step,
                       acts->z, acts->kl_rows);
    pr.before(LTG_K_DEC0);
    if (vz) hipLaunchKernelGGL((k_dense_fwd<1, true>), grid2(H, R, 32, 32), dim3(NT), 0, st, R, H, Z, acts->z, gen->p[2], gen->p[6], acts->h2);
    else hipLaunchKernelGGL((k_dense_fwd<1, false>), grid2(H, R, 32, 32), dim3(NT), 0, st, R, H, Z, acts->z, gen->p[2], gen->p[6], acts->h2);
    pr.after(LTG_K_DEC0);
    }
    {
        const bool bf = cfg->precision == LTG_PREC_BF16, big = r.dec_tile == 128;
        pr.before(LTG_K_DEC1_FWD);
        if (r.dec == LTG_DEC_SMALL) {
            if (bf) hipLaunchKernelGGL(fk_dec1<true>, grid2(I, R, 16, 16), dim3(NT), 0, st, R, I, H, acts->h2, gen->p[3], gen->p[7], acts->logits);
            else hipLaunchKernelGGL(fk_dec1<false>, grid2(I, R, 16, 16), dim3(NT), 0, st, R, I, H, acts->h2, gen->p[3], gen->p[7], acts->logits);
        } else if (r.dec != LTG_DEC_TILE) {
            if (stat && r.stats == LTG_STATS_EPILOGUE) stat_groups = launch_dec1_fwd_stream(cfg, gen, r, R, acts, stat, st);
            else launch_dec1_fwd_stream(cfg, gen, r, R, acts, nullptr, st);
        } else if (bf && big) hipLaunchKernelGGL((k_dec1_fwd<true, true>), grid2(I, R, 64, 128), dim3(NT), 0, st, R, I, H, acts->h2, gen->p[3], gen->p[7], acts->logits);
        else if (bf) hipLaunchKernelGGL((k_dec1_fwd<true, false, true>), grid2(I, R, 32, 32), dim3(NT), 0, st, R, I, H, acts->h2, gen->p[3], gen->p[7], acts->logits);
        else if (big) hipLaunchKernelGGL((k_dec1_fwd<false, true>), grid2(I, R, 64, 128), dim3(NT), 0, st, R, I, H, acts->h2, gen->p[3], gen->p[7], acts->logits);
        else hipLaunchKernelGGL((k_dec1_fwd<false, false>), grid2(I, R, 32, 32), dim3(NT), 0, st, R, I, H, acts->h2, gen->p[3], gen->p[7], acts->logits);
        pr.after(LTG_K_DEC1_FWD);
    }
    return stat_groups;
}

// softmax statistics of the local logits into rowpart (the G step: with the batch's loss terms, RP floats per row) and / or lse: from the
// decoder kernel's epilogue (stat_groups > 0), by the segment pass, or row by row
void g_row_partial(const ltg_config* cfg, const ltg_g_route_info& r, const ltg_batch* bt, const ltg_pairs* fake, const ltg_gen_acts* acts,
                          float* rowpart, hipStream_t st, float* segpart = nullptr, float* lse = nullptr, int stat_groups = 0) {
    const int I = cfg->n_items, B = bt->n_rows;
    if (stat_groups > 0) {   // the decoder kernel left its statistics in segpart
        hipLaunchKernelGGL(k_row_stats_merge, dim3(B), dim3(NT), 0, st, B, stat_groups, I, cfg->item_lo, segpart, bt->indptr, bt->indices, bt->values,
                           acts->logits, fake ? fake->n : 0, fake ? fake->row : nullptr, fake ? fake->niche : nullptr, fake ? fake->pop : nullptr,
                           rowpart, lse);
        return;
    }
    if (segpart && r.seg_pass) {
        const int nseg = (I + RS_SEG - 1) / RS_SEG;
        hipLaunchKernelGGL(k_row_partial_seg, dim3(nseg, B), dim3(NT), 0, st, I, cfg->item_lo, bt->indptr, bt->indices, bt->values, acts->logits,
                           fake ? fake->n : 0, fake ? fake->row : nullptr, fake ? fake->niche : nullptr, fake ? fake->pop : nullptr, segpart);
        hipLaunchKernelGGL(k_row_partial_merge, dim3(B), dim3(64), 0, st, B, nseg, segpart, rowpart, lse);
        return;
    }
    hipLaunchKernelGGL(k_row_partial, dim3(bt->n_rows), dim3(NT), 0, st, cfg->n_items, cfg->item_lo, bt->indptr, bt->indices, bt->values,
                       acts->logits, fake ? fake->n : 0, fake ? fake->row : nullptr, fake ? fake->niche : nullptr,
                       fake ? fake->pop : nullptr, rowpart);
}

// bytes of the segment-partial scratch for `rows` rows (the first two carve entries of the workspace)
inline size_t segpart_bytes(const ltg_config* cfg, int rows) {
    return align_up((size_t)rows * RP * sizeof(float)) + align_up(segpart_floats(cfg->n_items, rows) * sizeof(float));
}

int vae_forward_impl(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_fwd_opts* o,
                     const ltg_gen_acts* acts, float* probs_out, hipStream_t st, void* ws = nullptr, size_t ws_bytes = 0) {
    const int R = bt->n_rows, I = cfg->n_items;
    if (R <= 0) return LTG_OK;
    const ltg_g_route_info r = g_route(cfg, gen, R, true);
    fwd_stage_enc(cfg, gen, r, bt, o, acts, 0, st);
    const bool have_scratch = ws && r.seg_pass && ws_bytes >= segpart_bytes(cfg, R);
    float* segpart = have_scratch ? reinterpret_cast<float*>((char*)ws + align_up((size_t)R * RP * sizeof(float))) : nullptr;
    const int sg = fwd_stage_rest(cfg, gen, r, bt, o, acts, 0, st, segpart);
    if (segpart) g_row_partial(cfg, r, bt, nullptr, acts, nullptr, st, segpart, acts->lse, sg);
    else hipLaunchKernelGGL(k_row_lse, dim3(R), dim3(NT), 0, st, I, acts->logits, acts->lse);
    if (probs_out) {
        const int gx = (I + NT - 1) / NT < 64 ? (I + NT - 1) / NT : 64;
        hipLaunchKernelGGL(k_softmax_write, dim3(gx, R), dim3(NT), 0, st, I, acts->logits, acts->lse, probs_out);
    }
    return check_launch();
}

#ifndef LTG_D_FORK_MIN_ROWS
#define LTG_D_FORK_MIN_ROWS 1024
#endif
#ifndef LTG_D_SPLIT_SET
#define LTG_D_SPLIT_SET 0xE      // l2, bwd1, bwd2 (l1: one 16 x 16 output per wave -- the split's 36 vector instructions per block buy 4 MFMAs of 32 cycles)
#endif
// fp8 discriminator with EVERY GEMM operand in operand format (ltg_fp8bwd.h).  Tuning-knob bit 19 (backward converts on the fly, the
// round-2 path) switches it off.
inline bool d_fp8_opfmt(const ltg_config* c, const ltg_disc_state* d) {
    return fast_on(c) && c->d_precision == LTG_PREC_FP8 && d->emb_fp8 && d->w1t_fp8 && d->w2t_fp8 && d->w3t_fp8 && d->w3_fp8 && (c->d_h0 % 128) == 0 &&
           ((c->d_h1 + c->d_h2) % 128) == 0 && (c->d_h3 % 128) == 0 && (c->d_h1 % 64) == 0 && (c->d_h2 % 64) == 0 && c->d_h3 <= 64 * D8_OUT_CM &&
           (c->tuning & (1 << 19)) == 0;
}
// The Adam sweep over `slab` (gradient slabs of stride `stride`; lrow: the per-row loss terms of the generic kernels, else the loss sits in
// slot P of the slabs): tile-wise with the operand-format shadows following the weights (k8_d_adam), or one flat float4 sweep (fk_d_adam)
// when the eight tensors (and moments) lie back to back -- and no operand-format shadows have to follow the weights (fp8 mode: k_d_adam
// rewrites the e4m3 copies of the three matrices it updates) --, else tensor by tensor (k_d_adam)
int d_adam_kind(const ltg_config* cfg, const ltg_disc_state* disc, int stride, const float* slab, bool lrow) {
    if (d_fp8_opfmt(cfg, disc)) return LTG_D_ADAM_FP8;
    const DLayout L = d_layout(cfg->d_h0, cfg->d_h1, cfg->d_h2, cfg->d_h3);
    bool flat = !lrow && (stride % 4) == 0 && !(cfg->d_precision == LTG_PREC_FP8 && disc->w1t_fp8);
    for (int i = 0; i < 7; ++i) {
        const size_t sz = (size_t)(L.off[i + 1] - L.off[i]);
        flat = flat && disc->p[i + 1] == disc->p[i] + sz && disc->m[i + 1] == disc->m[i] + sz && disc->v[i + 1] == disc->v[i] + sz;
    }
    flat = flat && ((uintptr_t)disc->p[0] % 16) == 0 && ((uintptr_t)disc->m[0] % 16) == 0 && ((uintptr_t)disc->v[0] % 16) == 0 && ((uintptr_t)slab % 16) == 0;
    return flat ? LTG_D_ADAM_FLAT : LTG_D_ADAM_TENSORS;
}

// ---- the discriminator's route: the kernels of a forward (with_bwd = false) or a step over n pair rows.  A pure function of its arguments,
// computed once per call (ltg_d_route hands it out: include/ltg.h has the fields).  has_aux: the caller gave an aux stream and device words;
// slab: where the step's gradient slabs will lie (the flat sweep needs them 16-byte aligned).
ltg_d_route_info d_route(const ltg_config* c, const ltg_disc_state* d, int n, bool with_bwd, bool has_aux = false, const float* slab = nullptr) {
    ltg_d_route_info r = {};
    const int h0 = c->d_h0, h1 = c->d_h1, h2 = c->d_h2, h3 = c->d_h3, h12 = h1 + h2, arith = c->d_arith & 3;
    const bool fast = fast_on(c), fp8 = c->d_precision == LTG_PREC_FP8;
    const bool fk = fast && c->d_precision == LTG_PREC_FP32 && !d_wide(c) && h3 <= 512 && (h0 % 4) == 0 && (h12 % 4) == 0 && (h3 % 4) == 0;
    r.mode = c->d_precision == LTG_PREC_BF16 ? 1 : (fp8 ? 2 : 0);
    if (!with_bwd && ft_wsp_capable(c) && arith != LTG_DARITH_FP32 && (c->tuning & (1 << 20)) == 0)
        r.kind = LTG_D_TOWER;   // forward only, split arithmetic (tuning-knob bit 20: the three launches of LTG_D_STAGED_FWD instead)
    else if (fk && !with_bwd && h0 >= 32 && h12 >= 32)
        r.kind = LTG_D_STAGED_FWD;   // (d_arith = fp32, tuning bit 20, or sizes the one-kernel tower does not take)
    else if (fk) r.kind = LTG_D_FAST;
    else if (fp8 && fast && d->emb_fp8 && d->w1t_fp8 && d->w2t_fp8 && d->w3t_fp8 && (h0 % 64) == 0 && (h12 % 64) == 0) {
        // operand-format storage: both forward layers read e4m3 bytes (embedding table, transposed weight shadows, A1 in e4m3);
        // LDS-staged tiles for 128-multiples, the register-resident block for 64- but not 128-multiples
        if (with_bwd && d_fp8_opfmt(c, d)) r.kind = LTG_D_FP8_OPFMT;
        else r.kind = ((h0 % 128) == 0 && (h12 % 128) == 0) ? LTG_D_FP8_STAGED : LTG_D_FP8_REG;
    } else r.kind = LTG_D_GENERIC;
    // tiles of the generic GEMM kernels: 32 = scalar loaders (latency-bound default sizes); 64 / 128 = 16-B vector loaders for a wide
    // discriminator (every dimension a multiple of 4), sized so that each launch still fills the 256 CUs
    if (d_wide(c) && (h0 % 4) == 0 && (h1 % 4) == 0 && (h2 % 4) == 0 && (h3 % 4) == 0) {
        r.tile[0] = r.tile[2] = 64;
        r.tile[1] = fp8 ? 64 : -32;   // l2 (N = h3 = 256): too few 64-tiles to fill the chip unless the loads are the bottleneck
        r.tile[3] = 128;
    } else {
        // default sizes (100/150/250/300): l2 and backward stage 1 only touch h12 = 400 and h3 = 300 wide rows -> 16-B
        // loaders on the 32 x 32 tiles; l1 / stage 2 index columns of width h1 = 150 (8-B aligned only) -> scalar
        r.tile[1] = r.tile[2] = ((h12 % 4) == 0 && (h3 % 4) == 0) ? -32 : 32;
        r.tile[0] = r.tile[3] = (h0 % 4) == 0 ? -33 : 32;   // embedding rows (operand A) in 16-B pieces
    }
    {   // backward stage 1 with > 1024 32 x 32 tiles is throughput-bound, not latency-bound: 64 x 64 tiles (measured -5 %)
        const int ks = (n + D_KCHUNK - 1) / D_KCHUNK;
        const long t32 = (long)((n + 31) / 32) * ((h12 + 31) / 32) + (long)ks * ((h12 + 32) / 32) * ((h3 + 31) / 32);
        if (r.tile[2] == -32 && t32 > 1024) r.tile[2] = 64;
    }
    // ltg_config.d_arith: SPL of fk_d_l1, fk_d_l2, fk_d_bwd1, fk_d_bwd2 of the config.ini-sized fp32 discriminator step -- 0 =
    // v_mfma_f32_16x16x4_f32, 6 / 4 = bf16 cross terms of the split operands (ltg_rgemm.h).  Bits 4-7 choose the kernels (measurements);
    // 0 = the library's set LTG_D_SPLIT_SET.
    // (the four-term form is cheap enough to pay in fk_d_l1 too: D phase 45.5 against 45.9 ms, profiles/r6_ab_d_arith.txt)
    const int set = ((c->d_arith >> 4) & 15) ? ((c->d_arith >> 4) & 15) : (arith == LTG_DARITH_BF16X4 ? 0xF : LTG_D_SPLIT_SET);
    for (int i = 0; i < 4; ++i) r.spl[i] = (arith == LTG_DARITH_FP32 || !((set >> i) & 1)) ? 0 : (arith == LTG_DARITH_BF16X4 ? 4 : 6);
    const bool padded = r.kind == LTG_D_FAST || r.kind == LTG_D_FP8_OPFMT;
    const int P = d_layout(h0, h1, h2, h3).off[8];
    r.adam = d_adam_kind(c, d, padded ? d_slab_stride(P) : P, slab, r.kind != LTG_D_FAST);
    // Jobs B / C on the aux stream (d_step_impl has the mechanism and its measurements):
    // (only with the FLAT tensor layout: the poison word reaches fk_d_adam alone -- separate tensors take k_d_adam, which has no early
    // return, so a direct C-ABI caller with that layout keeps the whole step on one stream)
    // (Round 6: only from LTG_D_FORK_MIN_ROWS pair rows.  At the ~300 rows per step of the synthetic tables the two jobs are one or two slabs of work and
    // the fork's two gate kernels and its poll cost more than they hide -- and not steadily: D step 32.6-38.9 us with the fork against 34.1 +- 0.1
    // without at 20 000 items, 34.1-38.2 against 32.4 at 200 000 -- profiles/r6_ab_d_fork_small.txt.  Either way the same kernels write the same slab
    // entries: same bits.)
    r.fork = has_aux && with_bwd && r.kind == LTG_D_FAST && n >= LTG_D_FORK_MIN_ROWS && r.adam == LTG_D_ADAM_FLAT;
    return r;
}

// forward of one or both towers into ws (A1, A3, y, ds, lrow)
#define LTG_D_DISPATCH3(KERNEL, MODE, TS, V, GRID, ST, ...)                                                          \
    do {                                                                                                             \
        if ((MODE) == 1) hipLaunchKernelGGL((KERNEL<1, TS, V>), GRID, dim3(NT), 0, ST, __VA_ARGS__);                 \
        else if ((MODE) == 2) hipLaunchKernelGGL((KERNEL<2, TS, V>), GRID, dim3(NT), 0, ST, __VA_ARGS__);            \
        else hipLaunchKernelGGL((KERNEL<0, TS, V>), GRID, dim3(NT), 0, ST, __VA_ARGS__);                             \
    } while (0)
// TSV: tile size; -32 = 32 x 32 tiles with 16-B vector loaders on both operands, -33 = on operand A only
#define LTG_D_DISPATCH(KERNEL, MODE, TSV, GRID, ST, ...)                                                             \
    do {                                                                                                             \
        if ((TSV) == 128) LTG_D_DISPATCH3(KERNEL, MODE, 128, 3, GRID, ST, __VA_ARGS__);                              \
        else if ((TSV) == 64) LTG_D_DISPATCH3(KERNEL, MODE, 64, 3, GRID, ST, __VA_ARGS__);                           \
        else if ((TSV) == -32) LTG_D_DISPATCH3(KERNEL, MODE, 32, 3, GRID, ST, __VA_ARGS__);                          \
        else if ((TSV) == -33) LTG_D_DISPATCH3(KERNEL, MODE, 32, 1, GRID, ST, __VA_ARGS__);                          \
        else LTG_D_DISPATCH3(KERNEL, MODE, 32, 0, GRID, ST, __VA_ARGS__);                                            \
    } while (0)

void disc_forward(const ltg_config* cfg, const ltg_disc_state* d, const ltg_d_route_info& r, PairView pv, DropView dA, DropView dB, DropView dC,
                  float keep, uint64_t step, const Workspace& w0, bool with_bwd, const ltg_probe* probe, hipStream_t st, float* y_dst = nullptr) {
    Workspace w = w0;
    if (y_dst) w.y = y_dst;   // y straight into the caller's buffer
    const Probe pr{probe, st};
    const int n = pv.nr + pv.nf, h0 = cfg->d_h0, h1 = cfg->d_h1, h2 = cfg->d_h2, h3 = cfg->d_h3, h12 = h1 + h2;
    const int nmax = h1 > h2 ? h1 : h2;
    if (r.kind == LTG_D_TOWER) {
        // forward only, split arithmetic: ONE kernel from the id lists to y, A1 stays in LDS (ltg_tower.h).  The weights are split first: 1 MB at config.ini's sizes, ~3 us, once per call.
        ltg_ft_u32x4* wsp = reinterpret_cast<ltg_ft_u32x4*>(w.wsp);
        const int nwv = (int)ft_wsp_triples(h0, h1, h2, h3);
        hipLaunchKernelGGL(fkt_split_weights, dim3((nwv + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, st, h0, h1, h2, h3, d->p[0], d->p[2], d->p[4], wsp);
        const dim3 g((n + FT_BM - 1) / FT_BM);
        const size_t lds = ft_lds_bytes(h12);
        pr.before(LTG_K_D_L1);
        const bool inj = dA.real || dA.fake || dB.real || dB.fake || dC.real || dC.fake;
#define LTG_FT_LAUNCH(SPLV, INJV)                                                                                                                              \
    hipLaunchKernelGGL((fkt_d_tower<SPLV, 5, INJV>), g, dim3(FT_NT), lds, st, pv, h0, h1, h2, h3, d->emb, wsp, d->p[1], d->p[3], d->p[5], d->p[6], d->p[7], dA, dB, dC, \
                       keep, cfg->seed, step, w.y)
        if ((cfg->d_arith & 3) == LTG_DARITH_BF16X4) { if (inj) LTG_FT_LAUNCH(4, true); else LTG_FT_LAUNCH(4, false); }
        else { if (inj) LTG_FT_LAUNCH(6, true); else LTG_FT_LAUNCH(6, false); }
#undef LTG_FT_LAUNCH
        pr.after(LTG_K_D_L1);
        return;
    }
    if (r.kind == LTG_D_STAGED_FWD) {
        // forward only (the fake tower of the G steps, one batch or -- ltg_fake_tower_batched -- 10^5 pair rows): LDS-staged 64 x 64
        // tiles.  The choice depends on the layer sizes only, so the tower inside a step and the batched tower run the same
        // kernels and produce the same bits.
        LTG_PROBED(pr, LTG_K_D_L1, hipLaunchKernelGGL(fks_d_l1, dim3((h1 + 63) / 64 + (h2 + 63) / 64, (n + 63) / 64), dim3(NT), 0, st, pv, h0, h1, h2, d->emb, d->p[0],
                                                      d->p[1], d->p[2], d->p[3], dA, dB, keep, cfg->seed, step, w.A1));
        LTG_PROBED(pr, LTG_K_D_L2, hipLaunchKernelGGL(fks_d_l2, dim3((h3 + 63) / 64, (n + 63) / 64), dim3(NT), 0, st, n, h12, h3, w.A1, d->p[4], d->p[5], d->p[6], dC, keep,
                                                      cfg->seed, step, w.spart));
        hipLaunchKernelGGL(fk_d_y, dim3((n + NT - 1) / NT), dim3(NT), 0, st, pv, 2 * ((h3 + 63) / 64), w.spart, d->p[7], w.y);
        return;
    }
    if (r.kind == LTG_D_FAST) {
        // A3, G3 (backward only) and the per-tile partial dot products of the output unit; y only when nothing else follows
        LTG_PROBED(pr, LTG_K_D_L1, LTG_D_SPL_LAUNCH(r.spl[0], fk_d_l1, grid2(nmax, n, 32, 32, 2), dim3(NT), 0, st, pv, h0, h1, h2, d->emb, d->p[0], d->p[1], d->p[2],
                                                    d->p[3], dA, dB, keep, cfg->seed, step, w.A1));
        LTG_PROBED(pr, LTG_K_D_L2, LTG_D_SPL_LAUNCH(r.spl[1], fk_d_l2, dim3(((h3 + 31) / 32) * ((n + 31) / 32)), dim3(DL2_NT), 0, st, n, h12, h3, w.A1, d->p[4], d->p[5], d->p[6], dC, keep,
                                                    cfg->seed, step, w.A3, with_bwd ? w.G3 : (float*)nullptr, w.spart));
        if (!with_bwd) hipLaunchKernelGGL(fk_d_y, dim3((n + NT - 1) / NT), dim3(NT), 0, st, pv, (h3 + 31) / 32, w.spart, d->p[7], w.y);
        return;
    }
    // fp8 with operand-format storage: both forward layers read e4m3 bytes (embedding table, transposed weight shadows, A1 in e4m3)
    const dim3 g8l1((h1 + 63) / 64 + (h2 + 63) / 64, (n + 63) / 64);
    if (r.kind == LTG_D_FP8_OPFMT) {
        // the step's own forward: the same products, and every activation the backward multiplies is left behind in e4m3 in the
        // orientation its GEMM contracts over (ltg_fp8bwd.h)
        const int NP = d8_np(n);
        hipLaunchKernelGGL(k8_gather_t, dim3(h0 / 64, NP / 64, 2), dim3(NT), 0, st, pv, h0, NP, d->emb_fp8, w.ET_8);
        // (Round 5, measured and removed: the branch layers' product on 128 x 64 / 128 x 128 tiles -- half the operand bytes through the L1s per
        // output -- ran 38.3 / 72.1 us against the 64 x 64 tiles' 30.1 us on the same box: the loop is bound by the latency of its staged K
        // blocks, which 720 small workgroups hide better than 360 / 180 large ones, not by L2 bandwidth.)
        LTG_PROBED(pr, LTG_K_D_L1, hipLaunchKernelGGL((fk8t_d_l1<64, 64>), dim3(g8l1.x, NP / 64), dim3(NT), 0, st, pv, h0, h1, h2, NP,
                                                      d->emb_fp8, d->w1t_fp8, d->p[1], d->w2t_fp8, d->p[3], dA, dB, keep, cfg->seed, step, w.dA1T_16, w.A1_8, w.A1T_8));
    } else if (r.kind == LTG_D_FP8_STAGED) {
        // 64 x 64 tiles: 696 workgroups of 37 KB LDS, three or four per CU hide each other's load latency (measured at 1 820 pair
        // rows: 30-32 us; 128 x 128 tiles = 180 workgroups, one per CU, 54 us; 128 x 64: 60 us; register-resident block: 52 us)
        LTG_PROBED(pr, LTG_K_D_L1, hipLaunchKernelGGL((fk8s_d_l1<64, 64>), g8l1, dim3(NT), 0, st, pv, h0, h1, h2,
                                                      d->emb_fp8, d->w1t_fp8, d->p[1], d->w2t_fp8, d->p[3], dA, dB, keep, cfg->seed, step, w.A1, w.A1_8));
    } else if (r.kind == LTG_D_FP8_REG) {
        LTG_PROBED(pr, LTG_K_D_L1, hipLaunchKernelGGL(fk8_d_l1, dim3(8 * ((g8l1.x + 7) / 8) * g8l1.y), dim3(NT), 0, st, pv, h0, h1, h2, d->emb_fp8, d->w1t_fp8, d->p[1],
                                                      d->w2t_fp8, d->p[3], dA, dB, keep, cfg->seed, step, w.A1, w.A1_8));
        LTG_PROBED(pr, LTG_K_D_L2, hipLaunchKernelGGL(fk8_d_l2, grid2(h3, n, 64, 64), dim3(NT), 0, st, n, h12, h3, w.A1_8, d->w3t_fp8, d->p[5], dC, keep,
                                                      cfg->seed, step, w.A3));
    } else {
        const int md = r.mode, ts = r.tile[0], ts2 = r.tile[1], t1 = ts < 0 ? 32 : ts, t2 = ts2 < 0 ? 32 : ts2;
        LTG_PROBED(pr, LTG_K_D_L1, LTG_D_DISPATCH(k_d_l1, md, ts, grid2(nmax, n, t1, t1, 2), st, pv, h0, h1, h2, d->emb, d->p[0], d->p[1], d->p[2],
                                                  d->p[3], dA, dB, keep, cfg->seed, step, w.A1));
        LTG_PROBED(pr, LTG_K_D_L2, LTG_D_DISPATCH(k_d_l2, md, ts2, grid2(h3, n, t2, t2), st, n, h12, h3, w.A1, d->p[4], d->p[5], dC, keep, cfg->seed, step, w.A3));
    }
    if (r.kind == LTG_D_FP8_OPFMT || r.kind == LTG_D_FP8_STAGED)
        LTG_PROBED(pr, LTG_K_D_L2, hipLaunchKernelGGL((fk8s_d_l2<64, 64>), grid2(h3, n, 64, 64), dim3(NT), 0, st, n, h12, h3, w.A1_8, d->w3t_fp8, d->p[5], dC, keep,
                                                      cfg->seed, step, w.A3));
    const dim3 go((n + NT / 64 - 1) / (NT / 64));
    if (r.kind == LTG_D_FP8_OPFMT)
        hipLaunchKernelGGL(k8_d_out, dim3(d8_np(n) / 16), dim3(NT), 0, st, pv, h3, d8_np(n), w.A3, d->p[6], d->p[7], keep, w.y, w.ds, w.lrow, w.dpre3_8, w.dpre3T_8);
    else if (with_bwd) hipLaunchKernelGGL(k_d_out<true>, go, dim3(NT), 0, st, pv, h3, w.A3, d->p[6], d->p[7], keep, w.y, w.ds, w.lrow, w.dpre3);
    else hipLaunchKernelGGL(k_d_out<false>, go, dim3(NT), 0, st, pv, h3, w.A3, d->p[6], d->p[7], keep, w.y, w.ds, w.lrow, w.dpre3);
}

}  // namespace

extern "C" {

int32_t ltg_abi_version(void) { return LTG_ABI_VERSION; }

size_t ltg_workspace_bytes(const ltg_config* cfg, int32_t max_rows, int32_t max_pairs) {
    if (!cfg_ok(cfg) || max_rows < 0 || max_pairs < 0) return 0;
    return carve(cfg, max_rows < 1 ? 1 : max_rows, max_pairs < 1 ? 1 : max_pairs, nullptr).bytes;
}
// The workspace of a call with `rows` batch rows and `pairs` pair rows in the caller's buffer, or LTG_EWORKSPACE when that is too small
static int carve_checked(const ltg_config* cfg, int rows, int pairs, void* ws, size_t ws_bytes, Workspace* w) {
    if (ltg_workspace_bytes(cfg, rows, pairs) > ws_bytes) return LTG_EWORKSPACE;
    *w = carve(cfg, rows, pairs, (char*)ws);
    return LTG_OK;
}

int ltg_vae_forward(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch, const ltg_fwd_opts* opts,
                    const ltg_gen_acts* acts, float* probs_out, void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !gen || !batch || !opts || !acts || batch->n_rows < 0) return LTG_EINVAL;
    if (!batch->indptr || !batch->indices || !acts->h1 || !acts->mulv || !acts->z || !acts->h2 || !acts->logits || !acts->lse ||
        !acts->kl_rows || !acts->row_scale)
        return LTG_EINVAL;
    if (opts->rows_per_step < 0 || (opts->rows_per_step > 0 && (opts->is_training != 0.f || opts->drop_keep))) return LTG_EINVAL;
    return vae_forward_impl(cfg, gen, batch, opts, acts, probs_out, (hipStream_t)stream, ws, ws_bytes);
}

size_t ltg_forward_scratch_bytes(const ltg_config* cfg, int32_t max_rows) {
    if (!cfg_ok(cfg) || max_rows <= 0) return 0;
    return segpart_bytes(cfg, max_rows);
}

int ltg_sample_pairs(const ltg_config* cfg, const ltg_sample_inputs* in, const float* logits, const float* lse,
                     int32_t* gen_out, int32_t* pop_out, int32_t* cnt_out, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !in || (!logits && !in->cand_logit) || !lse || !gen_out || !pop_out || !cnt_out) return LTG_EINVAL;
    if (in->n_rows < 0 || in->max_cand < 0) return LTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (in->rows_per_step < 0) return LTG_EINVAL;
    const int groups = in->rows_per_step > 0 ? (in->n_rows + in->rows_per_step - 1) / in->rows_per_step : 1;
    if (hipMemsetAsync(cnt_out, 0, sizeof(int32_t) * (size_t)(groups > 0 ? groups : 1), st) != hipSuccess) return LTG_ELAUNCH;
    if (in->n_rows == 0) return LTG_OK;
    const int max_cand = in->max_cand > 0 ? in->max_cand : 1;
    const size_t lds = (size_t)max_cand * sizeof(float);
    if (lds > 64 * 1024) return LTG_EINVAL;
    hipLaunchKernelGGL(k_sample_pairs, dim3(in->n_rows), dim3(SP_NT), lds, st, Ig_of(cfg), in->cand_ptr, in->cand_idx, in->pop_ptr,
                       in->pop_idx, in->n_sample, in->slot_ptr, in->valid_item, in->u_gumbel, in->u_pick, cfg->seed, in->rng_step,
                       logits, lse, gen_out, pop_out, cnt_out, in->cand_logit, in->rows_per_step);
    return check_launch();
}

// One Adam sweep of the discriminator (adam: LTG_D_ADAM_*, see d_adam_kind) from `ks` gradient slabs of stride `stride` (lrow: the
// per-row loss terms of the round-1 kernels, else the loss sits in slot P of the slabs)
static void d_apply(const ltg_config* cfg, const ltg_disc_state* disc, int adam, const DLayout& L, int ks, int stride, const float* slab, int n,
                    const float* lrow, const AdamC& ad, float* loss_out, const Probe& pr, hipStream_t st, const unsigned* poison = nullptr) {
    const int P = L.off[8];
    const bool flat = adam == LTG_D_ADAM_FLAT;
    int ga = ((flat ? P / 4 : P) + NT - 1) / NT;
    if (ga > 1024) ga = 1024;
    if (ga < 1) ga = 1;
    if (adam == LTG_D_ADAM_FP8) {
        // operand-format shadows follow the weights: tile-wise sweep with the transposed e4m3 copies written through LDS
        const int h0 = cfg->d_h0, h1 = cfg->d_h1, h2 = cfg->d_h2, h3 = cfg->d_h3;
        const int nt1 = (h0 / 64) * (h1 / 64), nt2 = (h0 / 64) * (h2 / 64), nt3 = ((h1 + h2) / 64) * (h3 / 64);
        const int nflat = (h1 + h2 + 2 * h3 + 1 + NT - 1) / NT;
        LTG_PROBED(pr, LTG_K_D_ADAM, hipLaunchKernelGGL(k8_d_adam, dim3(nt1 + nt2 + nt3 + nflat + 1), dim3(NT), 0, st, ks, L, stride, h0, h1, h2, h3, nt1, nt2, nt3, slab,
                                                        *disc, ad, n, lrow, loss_out));
        return;
    }
    pr.before(LTG_K_D_ADAM);
    if (flat) hipLaunchKernelGGL(fk_d_adam, dim3(ga + 1), dim3(NT), 0, st, ks, P, stride, slab, disc->p[0], disc->m[0], disc->v[0], ad, loss_out, poison);
    else hipLaunchKernelGGL(k_d_adam, dim3(ga), dim3(NT), 0, st, ks, L, stride, slab, *disc, ad, n, lrow, loss_out);
    pr.after(LTG_K_D_ADAM);
}

// forward + backward of the pair rows in `pv` into gradient slabs; then either the Adam sweep (grad_out == NULL: the
// whole step, train.py:300) or one summed gradient vector in grad_out (this rank's share: ltg_d_grad)
static int d_step_impl(const ltg_config* cfg, const ltg_disc_state* disc, PairView pv, DropView dA, DropView dB, DropView dC,
                       const ltg_d_opts* o, float* grad_out, float* loss_out, const Workspace& w, hipStream_t st) {
    const int n = pv.nr + pv.nf;
    const int h0 = cfg->d_h0, h1 = cfg->d_h1, h2 = cfg->d_h2, h3 = cfg->d_h3, h12 = h1 + h2;
    const ltg_d_route_info r = d_route(cfg, disc, n, true, o->aux_stream && o->sync && !grad_out, w.slab);
    disc_forward(cfg, disc, r, pv, dA, dB, dC, o->keep_prob, o->rng_step, w, true, o->probe, st);
    const Probe pr{o->probe, st};
    const AdamC ad = make_adam(cfg, o->adam_t > 0 ? o->adam_t : 1);
    const DLayout L = d_layout(h0, h1, h2, h3);
    const int ks = (n + D_KCHUNK - 1) / D_KCHUNK, P = L.off[8], SP = d_slab_stride(P);
    // what the sweep (or the gradient sum) behind the two backward stages reads: slabs, their stride, the per-row loss terms of n rows
    int n_slabs = ks, stride = SP, n_lrow = n;
    const float* lrow = w.lrow;
    const unsigned* poison = nullptr;
    if (r.kind == LTG_D_FAST) {
        const int ntile = (h3 + 31) / 32;
        const int nA = (((n + 31) / 32) * ((h12 + 31) / 32) + 7) & ~7;      // padded: job B starts on a multiple of 8 (XCD chunk map)
        const int nB = ks * ((h12 + 1 + 31) / 32) * ((h3 + 31) / 32);
        const int nC = ks * ((h3 + 2 + 31) / 32);
        // Jobs B / C (dw3, db3, dw4, db4, d_loss) need the forward only, not dpre1; job A -> stage 2 -> Adam is the critical chain.  With
        // ltg_d_opts.aux_stream + sync they run on the caller's AUX stream beside job A and stage 2, handed over through two device
        // words like the G step's forks (LTG_WORD_D_FWD_DONE, LTG_WORD_D_JOBS_DONE and the poison: include/ltg.h, enum ltg_word; once
        // poisoned the sweep returns at once).  (The jobs inside stage 2's launch: DESIGN.md 5.4, "Tried and not kept".)
        // (when it is taken: d_route)
        const bool fork = r.fork != 0;
        if (fork) poison = o->sync + LTG_WORD_POISON;
        const int spl1 = r.spl[2], spl2 = r.spl[3];
        LTG_PROBED(pr, LTG_K_D_BWD1, LTG_D_SPL_LAUNCH(spl1, fk_d_bwd1, dim3(fork ? nA : nA + nB + nC), dim3(NT), 0, st, pv, h12, h3, nA, nB, ntile, L, SP, w.A1, w.A3, w.G3,
                                                      w.spart, disc->p[7], disc->p[4], o->keep_prob, w.dpre1, w.slab,
                                                      fork ? gate_store(o->sync, LTG_WORD_D_FWD_DONE, o->seq) : LTG_NO_GATE));
        if (fork) {
            hipStream_t ax = (hipStream_t)o->aux_stream;
            hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, ax, gate_poll(o->sync, LTG_WORD_D_FWD_DONE, o->seq), LTG_NO_GATE);
            LTG_D_SPL_LAUNCH(spl1, fk_d_bwd1, dim3(nB + nC), dim3(NT), 0, ax, pv, h12, h3, 0, nB, ntile, L, SP, w.A1, w.A3, w.G3, w.spart, disc->p[7], disc->p[4],
                             o->keep_prob, w.dpre1, w.slab, LTG_NO_GATE);
            hipLaunchKernelGGL(k_gate_set, dim3(1), dim3(64), 0, ax, gate_store(o->sync, LTG_WORD_D_JOBS_DONE, o->seq), LTG_NO_GATE);
        }
        const int n2 = ks * ((h0 + 1 + 15) / 16) * ((h1 + 31) / 32 + (h2 + 31) / 32);
        LTG_PROBED(pr, LTG_K_D_BWD2, LTG_D_SPL_LAUNCH(spl2, fk_d_bwd2, dim3(n2 + (fork ? 1 : 0)), dim3(DB2_NT), 0, st, pv, h0, h1, h2, L, SP, disc->emb, w.dpre1, w.slab,
                                                      fork ? gate_poll(o->sync, LTG_WORD_D_JOBS_DONE, o->seq) : LTG_NO_GATE));
        n_lrow = 0;      // (the loss sits in slot P of the slabs)
        lrow = nullptr;
    } else if (r.kind == LTG_D_FP8_OPFMT) {
        // fp8 operands in operand format (ltg_fp8bwd.h): the forward left A1^T, dpre3, dpre3^T and the gathered embeddings^T behind
        const int NP = d8_np(n), ks8 = (NP + D8_KCHUNK - 1) / D8_KCHUNK;
        const int nA = (NP / 64) * ((h12 + 63) / 64);
        const int nB = ks8 * ((h12 + 1 + 63) / 64) * ((h3 + 63) / 64);
        const int nC = ks8 * ((h3 + 1 + 31) / 32);
        LTG_PROBED(pr, LTG_K_D_BWD1, hipLaunchKernelGGL(k8_d_bwd1, dim3(nA + nB + nC), dim3(NT), 0, st, n, NP, h12, h3, nA, nB, L, SP, w.dA1T_16, w.A3, w.ds, w.dpre3_8, w.dpre3T_8,
                                                        w.A1T_8, disc->w3_fp8, o->keep_prob, w.dpre1T_8, w.slab));
        const int n2 = ks8 * ((h0 + 1 + 63) / 64) * (h1 / 64 + h2 / 64);
        LTG_PROBED(pr, LTG_K_D_BWD2, hipLaunchKernelGGL(k8_d_bwd2, dim3(n2), dim3(NT), 0, st, NP, h0, h1, h2, L, SP, w.ET_8, w.dpre1T_8, w.slab));
        n_slabs = ks8;
    } else {
        // stage 1 (products with the OLD w3) and stage 2 only write gradient slabs; the single Adam sweep runs last
        const int md = r.mode, ts = r.tile[2], tsb = r.tile[3], ta = ts < 0 ? 32 : ts, tb = tsb < 0 ? 32 : tsb;
        auto tiles = [ta](int x) { return (x + ta - 1) / ta; };
        auto tilesb = [tb](int x) { return (x + tb - 1) / tb; };
        const int nA = tiles(n) * tiles(h12);
        const int nB = ks * tiles(h12 + 1) * tiles(h3);
        const int nC = ks * ((h3 + 1 + 31) / 32);
        LTG_PROBED(pr, LTG_K_D_BWD1, LTG_D_DISPATCH(k_d_bwd1, md, ts, dim3(nA + nB + nC), st, n, h12, h3, nA, nB, ks, L, w.A1, w.A3, w.ds, w.dpre3, disc->p[4],
                                                    o->keep_prob, w.dpre1, w.slab));
        const int n2 = ks * tilesb(h0 + 1) * (tilesb(h1) + tilesb(h2));
        LTG_PROBED(pr, LTG_K_D_BWD2, LTG_D_DISPATCH(k_d_bwd2, md, tsb, dim3(n2), st, pv, h0, h1, h2, ks, L, disc->emb, w.dpre1, w.slab));
        stride = P;      // (these kernels do not pad their slabs)
    }
    if (grad_out) hipLaunchKernelGGL(k_d_grad_sum, dim3(64), dim3(NT), 0, st, n_slabs, P, stride, w.slab, n_lrow, lrow, grad_out);
    else d_apply(cfg, disc, r.adam, L, n_slabs, stride, w.slab, n_lrow, lrow, ad, loss_out, pr, st, poison);
    return check_launch();
}


int ltg_d_step(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* real, const ltg_pairs* fake,
               const ltg_d_opts* o, float* loss_out, void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !disc || !real || !fake || !o || !loss_out || !ws || o->adam_t < 1) return LTG_EINVAL;
    const int n = real->n + fake->n;
    if (real->n < 0 || fake->n < 0) return LTG_EINVAL;
    Workspace w;
    if (carve_checked(cfg, 1, n, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return hipMemsetAsync(loss_out, 0, sizeof(float), st) == hipSuccess ? LTG_OK : LTG_ELAUNCH;
    PairView pv{real->n, fake->n, real->pop, real->niche, fake->pop, fake->niche};
    DropView dA{o->drop_real[0], o->drop_fake[0], real->n, 0}, dB{o->drop_real[1], o->drop_fake[1], real->n, 0},
        dC{o->drop_real[2], o->drop_fake[2], real->n, 0};
    return d_step_impl(cfg, disc, pv, dA, dB, dC, o, nullptr, loss_out, w, st);
}

size_t ltg_d_grad_floats(const ltg_config* cfg) {
    if (!cfg_ok(cfg)) return 0;
    return (size_t)d_slab_stride(d_layout(cfg->d_h0, cfg->d_h1, cfg->d_h2, cfg->d_h3).off[8]);
}

int ltg_d_grad(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* real, const ltg_pairs* fake, int32_t row_lo,
               int32_t row_hi, const ltg_d_opts* o, float* grad_out, void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !disc || !real || !fake || !o || !grad_out || !ws) return LTG_EINVAL;
    const int n = real->n + fake->n;
    if (real->n < 0 || fake->n < 0 || row_lo < 0 || row_hi < row_lo || row_hi > n) return LTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t gf = ltg_d_grad_floats(cfg);
    const int m = row_hi - row_lo;
    if (m == 0) return hipMemsetAsync(grad_out, 0, gf * sizeof(float), st) == hipSuccess ? LTG_OK : LTG_ELAUNCH;
    Workspace w;
    if (carve_checked(cfg, 1, m, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    // the sub-range [row_lo, row_hi) of the logical concatenation real | fake is again a (real, fake) pair of ranges
    const int r0 = row_lo < real->n ? row_lo : real->n, r1 = row_hi < real->n ? row_hi : real->n;
    const int f0 = (row_lo > real->n ? row_lo : real->n) - real->n, f1 = (row_hi > real->n ? row_hi : real->n) - real->n;
    PairView pv{r1 - r0, f1 - f0, real->pop + r0, real->niche + r0, fake->pop + f0, fake->niche + f0};
    const int wd[3] = {cfg->d_h1, cfg->d_h2, cfg->d_h3};
    DropView dv[3];
    for (int i = 0; i < 3; ++i) {
        dv[i].real = o->drop_real[i] ? o->drop_real[i] + (size_t)r0 * wd[i] : nullptr;
        dv[i].fake = o->drop_fake[i] ? o->drop_fake[i] + (size_t)f0 * wd[i] : nullptr;
        dv[i].nr = r1 - r0;
        dv[i].row0 = row_lo;
    }
    return d_step_impl(cfg, disc, pv, dv[0], dv[1], dv[2], o, grad_out, nullptr, w, st);
}

int ltg_d_apply(const ltg_config* cfg, const ltg_disc_state* disc, const float* grad, int32_t adam_t, float* loss_out, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !disc || !grad || !loss_out || adam_t < 1) return LTG_EINVAL;
    const DLayout L = d_layout(cfg->d_h0, cfg->d_h1, cfg->d_h2, cfg->d_h3);
    const Probe pr{nullptr, (hipStream_t)stream};
    const int stride = d_slab_stride(L.off[8]);
    d_apply(cfg, disc, d_adam_kind(cfg, disc, stride, grad, false), L, 1, stride, grad, 0, nullptr, make_adam(cfg, adam_t), loss_out, pr, (hipStream_t)stream);
    return check_launch();
}

// ---- generator step in four stages; between them an item-sharded run exchanges (1) the encoder
// pre-activation [B,H] (all-reduce), (2) the row partials [B,5] (all-gather), (3) dh2 [B,H] (all-reduce).
// ltg_g_step runs the same stages back to back with one "rank".

// The forward-only fake tower (y_data is pruned from the g_trainer fetch, train.py:326): y of the fake pairs into w.y, or y_dst
static void fake_tower(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* fake, DropView dA, DropView dB, DropView dC, float keep,
                       uint64_t step, const Workspace& w, const ltg_probe* probe, hipStream_t st, float* y_dst = nullptr) {
    const PairView pv{0, fake->n, nullptr, nullptr, fake->pop, fake->niche};
    disc_forward(cfg, disc, d_route(cfg, disc, fake->n, false), pv, dA, dB, dC, keep, step, w, false, probe, st, y_dst);
}
// ... of one G step: its masks (or injected keep flags) and its counter
static void fake_tower(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* fake, const ltg_g_opts* o, const Workspace& w,
                       const ltg_probe* probe, hipStream_t st) {
    fake_tower(cfg, disc, fake, DropView{nullptr, o->drop_fake[0], 0, 0}, DropView{nullptr, o->drop_fake[1], 0, 0}, DropView{nullptr, o->drop_fake[2], 0, 0},
               o->d_keep_prob, o->d_rng_step, w, probe, st);
}

static int g_stage_bwd_dec(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_disc_state* disc, const ltg_g_route_info& r, const ltg_batch* bt,
                           const ltg_pairs* fake, const ltg_g_opts* o, const ltg_gen_acts* acts, const float* rowpart_all,
                           int n_ranks, float* loss_out, const Workspace& w, float* dh2_out, hipStream_t st,
                           bool disc_done = false, const float* h2_for_da2 = nullptr) {
    const int B = bt->n_rows, I = cfg->n_items, H = cfg->h_enc, nf = fake->n;
    const Probe pr{o->probe, st};
    if (nf > 0 && !disc_done) fake_tower(cfg, disc, fake, o, w, o->probe, st);   // replicated on every rank
    if (r.loss != LTG_LOSS_GENERIC) {
#define LTG_DLC(D16)                                                                                                                                \
    hipLaunchKernelGGL(k_dlogits_combine<D16>, dim3((I + DL_SEG - 1) / DL_SEG, B), dim3(NT), 0, st, B, I, n_ranks, bt->indptr, bt->indices, bt->values, \
                       acts->logits, rowpart_all, acts->kl_rows, nf > 0 ? w.y : (const float*)nullptr, o->cnt, o->anneal, o->gan_lambda, nf,       \
                       fake->row, fake->niche, fake->pop, w.dlog, acts->lse, w.scal, loss_out, cfg->item_lo)
        if (r.dlog_bf16) LTG_DLC(true);
        else LTG_DLC(false);
#undef LTG_DLC
    } else {
    hipLaunchKernelGGL(k_g_combine, dim3(1), dim3(NT), 0, st, B, n_ranks, rowpart_all, nf, acts->kl_rows, nf > 0 ? w.y : nullptr, o->cnt,
                       o->anneal, o->gan_lambda, acts->lse, w.nb, w.Pb, w.scal, loss_out);
    hipLaunchKernelGGL(k_dlogits, dim3((I + DL_SEG - 1) / DL_SEG, B), dim3(NT), 0, st, B, I, bt->indptr, bt->indices, bt->values,
                       acts->logits, acts->lse, w.nb, w.Pb, w.scal, nf, fake->row, fake->niche, fake->pop, w.dlog, cfg->item_lo);
    }
    const int kchunk = r.dh2_chunk, nsplit = r.dh2_nsplit;
    const bool bf = cfg->precision == LTG_PREC_BF16;
    pr.before(LTG_K_DH2);
    if (r.dh2 == LTG_DH2_STREAM) {
        if (r.dlog_bf16) hipLaunchKernelGGL((k_dh2_stream<true, DH2_NH>), dim3(nsplit, DH2_NH), dim3(ST_NT), (size_t)2 * ST_BN * ST_LDW * 2, st, B, I, H, kchunk, w.dlog, gen->wp1t_bf16, w.part);
        else hipLaunchKernelGGL((k_dh2_stream<false, DH2_NH>), dim3(nsplit, DH2_NH), dim3(ST_NT), (size_t)2 * ST_BN * ST_LDW * 2, st, B, I, H, kchunk, w.dlog, gen->wp1t_bf16, w.part);
    } else if (r.dh2_tile == 128) {
        if (bf) hipLaunchKernelGGL((k_dh2_partial<true, true>), grid2(H, B, 64, 128, nsplit), dim3(NT), 0, st, B, I, H, kchunk, w.dlog, gen->p[3], w.part);
        else hipLaunchKernelGGL((k_dh2_partial<false, true>), grid2(H, B, 64, 128, nsplit), dim3(NT), 0, st, B, I, H, kchunk, w.dlog, gen->p[3], w.part);
    } else if (r.dh2_tile == -32) hipLaunchKernelGGL((k_dh2_partial<true, false, true>), grid2(H, B, 32, 32, nsplit), dim3(NT), 0, st, B, I, H, kchunk, w.dlog, gen->p[3], w.part);
    else if (bf) hipLaunchKernelGGL((k_dh2_partial<true, false>), grid2(H, B, 32, 32, nsplit), dim3(NT), 0, st, B, I, H, kchunk, w.dlog, gen->p[3], w.part);
    else hipLaunchKernelGGL((k_dh2_partial<false, false>), grid2(H, B, 32, 32, nsplit), dim3(NT), 0, st, B, I, H, kchunk, w.dlog, gen->p[3], w.part);
    pr.after(LTG_K_DH2);
    // slab sum; the single-GPU path folds the tanh derivative in (dh2_out is then already da2)
    hipLaunchKernelGGL(k_da2, grid1(B * H, 2048), dim3(NT), 0, st, B * H, nsplit, w.part, h2_for_da2, dh2_out);
    return check_launch();
}

// item -> gradient-row map of the batch: the caller's cache, or rebuilt in the workspace (ltg_batch.slot == NULL: no per-batch cache --
// n_batches x I ints at full scale)
static const int32_t* g_slot_map(const ltg_config* cfg, const ltg_batch* bt, const Workspace& w, hipStream_t st) {
    if (bt->slot) return bt->slot;
    const int I = cfg->n_items, nu = bt->n_unique;
    hipLaunchKernelGGL(k_fill_i32, grid1(I, 512), dim3(NT), 0, st, I, -1, w.slotmap);
    if (nu > 0) hipLaunchKernelGGL(k_slot_scatter, dim3((nu + NT - 1) / NT), dim3(NT), 0, st, nu, bt->uptr, bt->csr_pos, bt->indices, w.slotmap);
    return w.slotmap;
}
// grid of the sweep over W_q0 and its bias row (k_enc0_bwd_adam, or that job of fk_g_tail): a thread per float4, capped
static unsigned q0_sweep_grid(int I, int H) {
    const size_t total = (size_t)(I + 1) * (H / 4), gx = (total + NT - 1) / NT;
    return (unsigned)(gx > 262144 ? 262144 : gx);
}

// sparse gradient rows of W_q0 (+ partial bias rows) into w.gq0 (the latency path's kernels: LTG_MID_FAST chains only)
struct Enc0Grad {
    const ltg_gen_state* gen = nullptr;   // gen + ad: the lazy clock's Adam step on the batch's rows, fused
    const AdamC* ad = nullptr;
    bool row_waves = true;                // one wave per row (false: column-blocked)
    const unsigned* poison = nullptr;
    LtgGate started = LTG_NO_GATE;        // stored when the kernel starts
    LtgGate end_wait = LTG_NO_GATE;       // polled by one more block, as the last thing the launch does
    float* lr_slot = nullptr;             // the step's learning rate into the clock's ring here (the tail runs elsewhere)
};
static void g_enc0_grad(const ltg_config* cfg, const ltg_batch* bt, const ltg_g_opts* o, const ltg_gen_acts* acts, const Workspace& w,
                        hipStream_t st, const Enc0Grad& a) {
    const int B = bt->n_rows, I = cfg->n_items, H = cfg->h_enc, nu = bt->n_unique;
    const ltg_gen_state* gen = a.gen;
    const AdamC* ad = a.ad;
    const LtgGate end_wait = a.end_wait;
    const Probe pe{o->probe, st};
    pe.before(LTG_K_ENC0_GRAD);
    if (a.row_waves) {   // one wave per row over all columns: a third of the waves (see fk_enc0_grad_rows)
        const int ncb = (H / 4 + 63) / 64;
        const dim3 g((nu + ENC0_BIAS_PARTS + G0_NW - 1) / G0_NW + (end_wait.word ? 1 : 0));
#define LTG_G0_ROWS(N)                                                                                                                                   \
    hipLaunchKernelGGL(fk_enc0_grad_rows<N>, g, dim3(G0_NT), 0, st, B, I, H, nu, bt->uptr, bt->rowidx, bt->csr_pos, bt->indices, bt->values, o->fwd.drop_keep, \
                       o->fwd.keep_prob, cfg->seed, o->fwd.rng_step, acts->row_scale, w.da1, w.gq0, cfg->item_lo, Ig_of(cfg), gen ? *gen : ltg_gen_state{},     \
                       ad ? *ad : AdamC{}, (gen && ad) ? gen->q0_ord + 1 : 0, bt->uitem, a.poison, a.started, end_wait, a.lr_slot)
        if (ncb == 1) LTG_G0_ROWS(1);
        else if (ncb == 2) LTG_G0_ROWS(2);
        else LTG_G0_ROWS(3);
#undef LTG_G0_ROWS
    } else
        hipLaunchKernelGGL(fk_enc0_grad, dim3((H / 4 + 63) / 64, (nu + ENC0_BIAS_PARTS + G0_NW - 1) / G0_NW), dim3(G0_NT), 0, st, B, I, H, nu, bt->uptr, bt->rowidx, bt->csr_pos,
                           bt->indices, bt->values, o->fwd.drop_keep, o->fwd.keep_prob, cfg->seed, o->fwd.rng_step, acts->row_scale, w.da1, w.gq0,
                           cfg->item_lo, Ig_of(cfg), gen ? *gen : ltg_gen_state{}, ad ? *ad : AdamC{}, (gen && ad) ? gen->q0_ord + 1 : 0, bt->uitem);
    pe.after(LTG_K_ENC0_GRAD);
}

// Every Adam update of the step behind dz -> dh1 as jobs of ONE launch of fk_g_tail (see there): W_p0, W_q1, the scalars, and
struct TailJobs {
    const int32_t* slot = nullptr;    // W_q0: sweep + sparse rows through this map (NULL: the dense product)
    bool with_dec1 = false;           // W_p1t as well (small item slabs; large ones ran the streaming kernel before)
    float* loss_out = nullptr;
    bool no_q0 = false;               // no W_q0 job: a launch of its own follows
    bool q0_bias = false;             // only the bias row of W_q0: the lazy clock has the item rows
    const unsigned* poison = nullptr;
    LtgGate end_wait = LTG_NO_GATE;   // polled by one more block, as the last thing the launch does
    bool bias_from_da1 = false;       // q0_bias: the bias row by fk_q0_bias_from_da1 behind the tail instead
};
static void g_jobs(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_g_opts* o, const ltg_gen_acts* acts,
                   const Workspace& w, const AdamC& ad, hipStream_t st, const TailJobs& j) {
    const int B = bt->n_rows, I = cfg->n_items, H = cfg->h_enc, Z = cfg->z_dim;
    const int32_t* slot = j.slot;
    const bool with_dec1 = j.with_dec1, q0_bias = j.q0_bias, bias_from_da1 = j.bias_from_da1;
    TailArgs a;
    a.B = B; a.I = I; a.H = H; a.Z = Z; a.nu = bt->n_unique;
    a.nz = a.nh = 0;     // (dz / dh1 were launched on their own)
    a.n1 = with_dec1 ? ((I + 31) / 32) * ((H + 1 + LTG_TAIL_BN - 1) / LTG_TAIL_BN) : 0;
    a.n2 = ((Z + 1 + 31) / 32) * ((H + LTG_TAIL_BN - 1) / LTG_TAIL_BN);
    a.n3 = ((H + 1 + 31) / 32) * ((2 * Z + LTG_TAIL_BN - 1) / LTG_TAIL_BN);
    a.n4 = 0;
    if (!j.no_q0) a.n4 = slot ? (int)q0_sweep_grid(I, H) : ((I + 1 + 31) / 32) * ((H + LTG_TAIL_BN - 1) / LTG_TAIL_BN);
    a.q0_bias = 0;
    if (q0_bias) {   // lazy Adam clock: fk_enc0_grad updated the item rows, one block finishes the bias row
        a.n4 = bias_from_da1 ? 0 : 1;      // (bias_from_da1: fk_q0_bias_from_da1 follows on the same stream)
        a.q0_bias = bias_from_da1 ? 0 : 1;
    }
    a.n5 = with_dec1 ? 1 : 0;
    a.Wp0 = gen->p[2]; a.Wq1 = gen->p[1]; a.mulv = acts->mulv; a.eps = o->fwd.eps; a.is_training = o->fwd.is_training;
    a.seed = cfg->seed; a.step = o->fwd.rng_step; a.dmlv_out = w.dmlv; a.da1_out = w.da1;
    a.dlog = w.dlog; a.h2 = acts->h2; a.z = acts->z; a.da2 = w.da2; a.h1 = acts->h1; a.dmlv = w.dmlv; a.G = w.gq0;
    a.xd = (slot || q0_bias) ? nullptr : w.xd;
    a.da1 = w.da1;
    a.slot = slot; a.rowout = w.rowout; a.cnt = o->cnt; a.anneal = o->anneal; a.lam = o->gan_lambda;
    a.loss_out = w.scal; a.loss_out2 = j.loss_out;
    a.poison = j.poison; a.n_wait = j.end_wait.word ? 1 : 0; a.end_wait = j.end_wait;
    const Probe pr{o->probe, st};
    pr.before(LTG_K_G_TAIL);
    const dim3 g(a.nz + a.nh + a.n1 + a.n2 + a.n3 + a.n4 + a.n5 + a.n_wait);
    if (cfg->precision == LTG_PREC_BF16) hipLaunchKernelGGL(fk_g_tail<true>, g, dim3(NT), 0, st, a, *gen, ad);
    else hipLaunchKernelGGL(fk_g_tail<false>, g, dim3(NT), 0, st, a, *gen, ad);
    if (q0_bias && bias_from_da1)
        hipLaunchKernelGGL(fk_q0_bias_from_da1, dim3(((H >> 2) + Q0B_COLS - 1) / Q0B_COLS), dim3(NT), 0, st, B, H, w.da1, *gen, ad, j.poison);
    pr.after(LTG_K_G_TAIL);
}

// Adam step gen->q0_ord + 1 of W_q0 / b_q0 on the lazy clock: the batch's rows with their gradient rows (w.gq0), the bias
// row, then the rotating slice of untouched rows.
// Where the clock's work of a step runs: ltg_g_step with an aux stream sets on_aux (g_stage_bwd_rest then runs it there); everyone else
// leaves it in stream order behind the clock's step
struct ClockSched {
    bool on_aux = false;
};
// the rotating slice of G step gen->q0_ord + 1: rows i = ord (mod period) up to `target`
static void q0_slice_sweep(const ltg_config* cfg, const ltg_gen_state* gen, int target, hipStream_t st) {
    const int I = cfg->n_items, P = gen->q0_period, start = (gen->q0_ord + 1) % P;
    if (start < I) hipLaunchKernelGGL(k_q0_sweep, dim3((I - start + P - 1) / P), dim3(Q0_NT), 0, st, I, cfg->h_enc, start, P, target, *gen, make_adam(cfg, 1));
}
// ... of this step, behind the clock's update of the batch's rows and the bias row (unless ltg_g_step has the slice on its aux stream, up to ord - 1)
static void q0_slice_of_step(const ltg_config* cfg, const ltg_gen_state* gen, ClockSched clock, hipStream_t st) {
    if (!clock.on_aux) q0_slice_sweep(cfg, gen, gen->q0_ord + 1, st);
}

// The LTG_MID_FAST backward chain behind da2: dz -> dh1 -> (sparse W_q0 gradient) -> every remaining Adam update as one tail launch ->
// the W_q0 update where it is a launch of its own.  r.small: W_p1t and the step's scalars (loss_out) are jobs of the tail as well.
static void g_chain(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_g_route_info& r, const ltg_batch* bt, const ltg_g_opts* o,
                    const ltg_gen_acts* acts, const Workspace& w, const AdamC& ad, float* loss_out, hipStream_t st, ClockSched clock) {
    const int B = bt->n_rows, H = cfg->h_enc, Z = cfg->z_dim;
    const Probe pr{o->probe, st};
    // (the lazy clock needs no item -> gradient-row map: its update walks the batch's distinct items)
    const bool lazy = r.q0 == LTG_Q0_LAZY;
    const int32_t* slot = r.q0 == LTG_Q0_SWEEP ? g_slot_map(cfg, bt, w, st) : nullptr;
    LTG_PROBED(pr, LTG_K_DZ, hipLaunchKernelGGL(fk_dz, grid2(Z, B, 16, 16), dim3(NT), 0, st, B, Z, H, w.da2, gen->p[2], acts->mulv, o->fwd.eps,
                                                o->fwd.is_training, o->anneal, cfg->seed, o->fwd.rng_step, w.dmlv));
    LTG_PROBED(pr, LTG_K_DH1, hipLaunchKernelGGL(fk_dh1, grid2(H, B, 16, 16), dim3(NT), 0, st, B, H, 2 * Z, w.dmlv, gen->p[1], acts->h1, w.da1));
    if (lazy) g_enc0_grad(cfg, bt, o, acts, w, st, {.gen = gen, .ad = &ad, .row_waves = r.grad_rows != 0});   // Adam on the batch's rows inside the gradient kernel
    else if (slot) g_enc0_grad(cfg, bt, o, acts, w, st, {.row_waves = r.grad_rows != 0});
    g_jobs(cfg, gen, bt, o, acts, w, ad, st, {.slot = slot, .with_dec1 = r.small != 0, .loss_out = loss_out, .no_q0 = r.q0_own_launch != 0, .q0_bias = lazy});
    if (lazy) {   // (fk_enc0_grad applied the step to the batch's rows and fk_g_tail to the bias row)
        LTG_PROBED(pr, LTG_K_ENC0_BWD_ADAM, q0_slice_of_step(cfg, gen, clock, st));
    } else if (r.q0_own_launch) {
        LTG_PROBED(pr, LTG_K_ENC0_BWD_ADAM, hipLaunchKernelGGL(k_enc0_bwd_adam, dim3(q0_sweep_grid(cfg->n_items, H)), dim3(NT), 0, st, cfg->n_items, H, bt->n_unique, slot, w.gq0, *gen, ad));
    }
}

// which part of the backward behind the dh2 exchange a caller asks for, and how it is scheduled
struct BwdRest {
    const float* dh2 = nullptr;   // the exchanged dh2; NULL: da2 is ready (the slab sum wrote it)
    bool only_dec1 = false;       // the decoder weight update alone
    LtgH2Done hd = LtgH2Done{nullptr, nullptr, 0u, nullptr};   // the streaming update's hand-over words (one-call step)
    ClockSched clock = {};
};
static int g_stage_bwd_rest(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_g_route_info& r, const ltg_batch* bt, const ltg_g_opts* o,
                            const ltg_gen_acts* acts, const Workspace& w, hipStream_t st, const BwdRest& a) {
    const int B = bt->n_rows, I = cfg->n_items, H = cfg->h_enc, Z = cfg->z_dim;
    const AdamC ad = make_adam(cfg, o->adam_t);
    const bool bf = cfg->precision == LTG_PREC_BF16;
    const bool only_dec1 = a.only_dec1;
    const LtgH2Done hd = a.hd;
    const bool aux_sweep = a.clock.on_aux && r.q0 == LTG_Q0_LAZY;   // ltg_g_step: the lazy clock's work on the aux stream
    // Everything on `st` unless the lazy clock's chain runs beside the weight update (below).  (The other updates on the aux stream:
    // DESIGN.md 5.4, "Tried and not kept".)
    hipStream_t aux = (hipStream_t)o->aux_stream;
    hipEvent_t evf = (hipEvent_t)o->ev_fork;
    if (a.dh2 && !only_dec1) hipLaunchKernelGGL(k_da2, grid1(B * H, 1024), dim3(NT), 0, st, B * H, 1, a.dh2, acts->h2, w.da2);  // da2 = dh2 * (1 - h2^2)
    // persistent workgroups of the streaming decoder weight update (see launch_dw).  Slabs below 65 536 items: 160 -- the rest of the
    // step runs beside the update, and what a kernel of that chain costs there is mostly how many CUs the update leaves it (round 4,
    // same box, per-rank proxy at 25 024 items: 196 workgroups 173.3-174.1 us per step, 160: 170.1-170.5, 128: 184, 96: 205;
    // 20 000 items: 166.3 / 161.6 / 161.3-162.4 / 179; the update alone takes 89 / 92 / 110 / 122 us with 196 / 160 / 128 / 98)
    int dw_gmax = I / 32 < 2048 ? 160 : 224;
    auto launch_dw = [&]() {
        const Probe prs{o->probe, st};
        prs.before(LTG_K_DEC1_BWD_ADAM);
        if (r.dw == LTG_DW_STREAM) {
            const int ntl = I / 32;
            if (r.dlog_bf16) {   // (the field the producer, g_stage_bwd_dec, stored dlog under)
                // persistent workgroups: 224 = 28 per XCD (measured 657 us at 200 000 items; 256: 678, 240: 669, 192: 671) -- and 32 CUs
                // stay free for whatever runs beside it ...
                int gmax = dw_gmax;
                // ... and no more workgroups than the same number of rounds needs (782 tiles of a 25 024-item slab: 4 rounds with
                // 224 or with 196 workgroups -- 60 CUs left to the chain and the collective running beside it)
                if (ntl > gmax) gmax = (ntl + (ntl + gmax - 1) / gmax - 1) / ((ntl + gmax - 1) / gmax);
                hipLaunchKernelGGL(k_dec1_bwd_adam_stream<true>, dim3(ntl < gmax ? ntl : gmax), dim3(ST_NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, hd);
                if (r.dw_ragged)
                    hipLaunchKernelGGL((k_dec1_bwd_adam<true, 2, false, true>), grid2(H + 1, I - ntl * 32, 64, 64), dim3(NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, ntl * 32,
                                       hd.poison);
            } else {
                hipLaunchKernelGGL(k_dec1_bwd_adam_stream<false>, dim3(ntl < 256 ? ntl : 256), dim3(ST_NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad);
                if (r.dw_ragged)
                    hipLaunchKernelGGL((k_dec1_bwd_adam<true, 2>), grid2(H + 1, I - ntl * 32, 64, 64), dim3(NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, ntl * 32);
            }
        } else if (r.dw_tile == 64) {
            if (bf) hipLaunchKernelGGL((k_dec1_bwd_adam<true, 2>), grid2(H + 1, I, 64, 64), dim3(NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, 0);
            else hipLaunchKernelGGL((k_dec1_bwd_adam<false, 2>), grid2(H + 1, I, 64, 64), dim3(NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, 0);
        } else if (r.dw_tile == -32) hipLaunchKernelGGL((k_dec1_bwd_adam<true, 0, true>), grid2(H + 1, I, 32, 32), dim3(NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, 0);
        else if (bf) hipLaunchKernelGGL((k_dec1_bwd_adam<true, 0>), grid2(H + 1, I, 32, 32), dim3(NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, 0);
        else hipLaunchKernelGGL((k_dec1_bwd_adam<false, 0>), grid2(H + 1, I, 32, 32), dim3(NT), 0, st, B, I, H, w.dlog, acts->h2, *gen, ad, 0);
        prs.after(LTG_K_DEC1_BWD_ADAM);
    };
    if (aux_sweep && r.mid == LTG_MID_FAST && !only_dec1) {
        // ltg_g_step, large item slab, lazy Adam clock of W_q0.  The decoder weight update (HBM-bound, the largest kernel of the
        // step) needs only dlog and h2; everything else that is left -- dz -> dh1 -> sparse W_q0 gradient -> the other Adam
        // updates -> the clock's step and its rotating slice -- needs only da2.  The two run side by side: the weight update on
        // `st` with 224 of its 256 persistent workgroups (28 per XCD; measured FASTER than 256: 657 vs 678 us at 200 000 items),
        // the chain on the aux stream on the CUs that leaves free.  (Round 1 found no overlap here: the weight update then held
        // every CU.)  Joined by ev_sweep at the end of ltg_g_step.
        (void)hipEventRecord(evf, st);
        (void)hipStreamWaitEvent(aux, evf, 0);
        // 64 CUs to the chain when the update has many rounds anyway: with Adam moments in every row of W_q0 the clock's deferred
        // arithmetic makes the chain the longer side on 32 CUs (same box, 200 000 items, warm moments: 224 -> 673 ms per 640
        // steps, 208 -> 666, 192 -> 647, 176 -> 650, 160 -> 659; cold moments 629 vs 632)
        if (I / 32 >= 2048) dw_gmax = 192;
        if (!o->dec1_done) launch_dw();
        g_chain(cfg, gen, r, bt, o, acts, w, ad, nullptr, aux, ClockSched{});   // (the slice in the chain's own stream order, behind the clock's step)
        (void)hipEventRecord((hipEvent_t)o->ev_sweep, aux);
        return check_launch();
    }
    if (aux_sweep) {
        // (batches the middle-layer fast path does not serve) only the rotating slice on the aux stream, eligible together with the decoder weight update
        (void)hipEventRecord(evf, st);
        (void)hipStreamWaitEvent(aux, evf, 0);
        if (!o->dec1_done) launch_dw();
        q0_slice_sweep(cfg, gen, gen->q0_ord, aux);   // the batch's rows are at q0_ord already (q0_touch): skipped
        (void)hipEventRecord((hipEvent_t)o->ev_sweep, aux);
    } else if (!o->dec1_done) launch_dw();
    if (only_dec1) return check_launch();
    if (r.mid == LTG_MID_FAST) {
        g_chain(cfg, gen, r, bt, o, acts, w, ad, nullptr, st, a.clock);
        return check_launch();
    }
    const bool vz = r.mid_vec != 0;
    const Probe pc{o->probe, st};
    pc.before(LTG_K_DZ);
#define LTG_V2(KERNEL, ...)                                       \
    do {                                                          \
        if (vz) hipLaunchKernelGGL(KERNEL<true>, __VA_ARGS__);    \
        else hipLaunchKernelGGL(KERNEL<false>, __VA_ARGS__);      \
    } while (0)
    LTG_V2(k_dz, grid2(Z, B, 32, 32), dim3(NT), 0, st, B, Z, H, w.da2, gen->p[2], acts->mulv, o->fwd.eps, o->fwd.is_training,
           o->anneal, cfg->seed, o->fwd.rng_step, w.dmlv);
    pc.after(LTG_K_DZ);
    pc.before(LTG_K_WGRAD_P0);
    LTG_V2(k_wgrad_adam, grid2(H, Z + 1, 32, 32), dim3(NT), 0, st, B, Z, H, acts->z, w.da2, gen->p[2], gen->m[2], gen->v[2],
           gen->p[6], gen->m[6], gen->v[6], ad);
    pc.after(LTG_K_WGRAD_P0);
    pc.before(LTG_K_DH1);
    LTG_V2(k_dh1, grid2(H, B, 32, 32), dim3(NT), 0, st, B, H, 2 * Z, w.dmlv, gen->p[1], acts->h1, w.da1);
    pc.after(LTG_K_DH1);
    pc.before(LTG_K_WGRAD_Q1);
    LTG_V2(k_wgrad_adam, grid2(2 * Z, H + 1, 32, 32), dim3(NT), 0, st, B, H, 2 * Z, acts->h1, w.dmlv, gen->p[1], gen->m[1],
           gen->v[1], gen->p[5], gen->m[5], gen->v[5], ad);
#undef LTG_V2
    pc.after(LTG_K_WGRAD_Q1);
    const int nu = bt->n_unique;
    const Probe pe{o->probe, st};
    pe.before(LTG_K_ENC0_BWD_ADAM);
    hipLaunchKernelGGL(k_enc0_grad, dim3(nu + ENC0_BIAS_PARTS), dim3(NT), (size_t)4 * H * sizeof(float), st, B, I, H, nu, bt->uptr, bt->rowidx,
                       bt->csr_pos, bt->indices, bt->values, o->fwd.drop_keep, o->fwd.keep_prob, cfg->seed, o->fwd.rng_step,
                       acts->row_scale, w.da1, w.gq0, cfg->item_lo, Ig_of(cfg));
    if (r.q0 == LTG_Q0_LAZY) {
        hipLaunchKernelGGL(k_q0_step_touched, dim3(nu + 1), dim3(Q0_NT), 0, st, I, H, nu, bt->uptr, bt->csr_pos, bt->indices, w.gq0, gen->q0_ord + 1, *gen, ad);
        q0_slice_of_step(cfg, gen, a.clock, st);
    } else {
        const int32_t* slot = g_slot_map(cfg, bt, w, st);
        hipLaunchKernelGGL(k_enc0_bwd_adam, dim3(q0_sweep_grid(I, H)), dim3(NT), 0, st, I, H, nu, slot, w.gq0, *gen, ad);
    }
    pe.after(LTG_K_ENC0_BWD_ADAM);
    return check_launch();
}

static bool g_args_ok(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_gen_acts* acts) {
    return cfg_ok(cfg) && gen && bt && acts && bt->n_rows > 0 && bt->indptr && bt->indices;
}

int ltg_g_step(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_disc_state* disc, const ltg_batch* bt,
               const ltg_pairs* fake, const ltg_g_opts* o, const ltg_gen_acts* acts, float* loss_out, void* ws,
               size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !gen || !disc || !bt || !fake || !o || !acts || !loss_out || !ws || o->adam_t < 1) return LTG_EINVAL;
    if (!bt->uptr || !bt->rowidx || !bt->csr_pos || !o->cnt || !fake->row || bt->n_rows <= 0 || fake->n < 0) return LTG_EINVAL;
    if (bt->n_unique < 0 || (size_t)bt->n_unique > gq0_rows(cfg, bt->n_rows)) return LTG_EINVAL;
    const int B = bt->n_rows, nf = fake->n;
    Workspace w;
    if (carve_checked(cfg, B, nf, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const ltg_g_route_info r = g_route(cfg, gen, B);
    const bool have_y = o->y_pre != nullptr;   // y_generated of this batch came from ltg_fake_tower_batched: no tower in this step
    if (have_y) w.y = const_cast<float*>(o->y_pre);
    // lazy Adam clock of W_q0: the batch's rows up to date first; its rotating slice (rows NOT of this batch: arithmetic-bound,
    // 48 registers -- it fits beside the 2 x 232-register waves of the HBM-bound decoder kernels) then runs on the aux stream
    q0_touch(cfg, gen, r, bt, st);
    const bool aux_sweep = r.q0 == LTG_Q0_LAZY && o->aux_stream && o->ev_fork && o->ev_sweep;
    // fork: the fake tower (independent of the generator forward) runs on the caller's aux stream
    const bool fork = o->aux_stream && o->ev_fork && o->ev_join && nf > 0 && !have_y;
    if (fork || aux_sweep) {
        hipStream_t aux = (hipStream_t)o->aux_stream;
        if (hipEventRecord((hipEvent_t)o->ev_fork, st) != hipSuccess || hipStreamWaitEvent(aux, (hipEvent_t)o->ev_fork, 0) != hipSuccess)
            return LTG_ELAUNCH;
        if (fork) {
            fake_tower(cfg, disc, fake, o, w, nullptr, aux);
            if (hipEventRecord((hipEvent_t)o->ev_join, aux) != hipSuccess) return LTG_ELAUNCH;
        }
    }
    fwd_stage_enc(cfg, gen, r, bt, &o->fwd, acts, 0, st, {.xd = r.small ? w.xd : nullptr, .touched = true});
    const int sgroups = fwd_stage_rest(cfg, gen, r, bt, &o->fwd, acts, 0, st, r.small ? nullptr : w.segpart);
    if (r.small) {
        // small item slab: nine launches per step: enc0, enc1, dec0, dec1 | row softmax + dlogits, dh2, dz, dh1, Adam tail (dW_q0 = xd^T . da1 dense)
        const int I = cfg->n_items, H = cfg->h_enc;
        const Probe pr{o->probe, st};
        if (nf > 0 && !fork && !have_y) fake_tower(cfg, disc, fake, o, w, o->probe, st);
        if (fork && hipStreamWaitEvent(st, (hipEvent_t)o->ev_join, 0) != hipSuccess) return LTG_ELAUNCH;
        LTG_PROBED(pr, LTG_K_ROW_DLOGITS, hipLaunchKernelGGL(fk_row_dlogits, dim3(B), dim3(NT), 0, st, B, I, bt->indptr, bt->indices, bt->values, acts->logits,
                                                             acts->kl_rows, w.y, nf, o->cnt, o->gan_lambda, fake->row, fake->niche, fake->pop, w.dlog,
                                                             acts->lse, w.rowout));
        pr.before(LTG_K_DH2);
        if (cfg->precision == LTG_PREC_BF16) hipLaunchKernelGGL(fk_dh2<true>, grid2(H, B, 16, 16), dim3(DH2_NT), 0, st, B, I, H, w.dlog, gen->p[3], acts->h2, w.da2);
        else hipLaunchKernelGGL(fk_dh2<false>, grid2(H, B, 16, 16), dim3(DH2_NT), 0, st, B, I, H, w.dlog, gen->p[3], acts->h2, w.da2);
        pr.after(LTG_K_DH2);
        g_chain(cfg, gen, r, bt, o, acts, w, make_adam(cfg, o->adam_t), loss_out, st, ClockSched{});
        return check_launch();
    }
    g_row_partial(cfg, r, bt, fake, acts, w.rowpart, st, w.segpart, nullptr, sgroups);
    if (fork && hipStreamWaitEvent(st, (hipEvent_t)o->ev_join, 0) != hipSuccess) return LTG_ELAUNCH;
    // single GPU: the slab sum writes da2 directly (one launch less than the sharded stage pair)
    int rc = g_stage_bwd_dec(cfg, gen, disc, r, bt, fake, o, acts, w.rowpart, 1, loss_out, w, w.da2, st, fork || have_y, acts->h2);
    if (rc != LTG_OK) return rc;
    rc = g_stage_bwd_rest(cfg, gen, r, bt, o, acts, w, st, {.clock = {.on_aux = aux_sweep}});
    if (aux_sweep && hipStreamWaitEvent(st, (hipEvent_t)o->ev_sweep, 0) != hipSuccess) return LTG_ELAUNCH;   // join
    return rc;
}

/* ---- the same step cut at its three exchange points (item-sharded multi-GPU; include/ltg.h) ---- */
int ltg_g_fwd_enc(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_fwd_opts* opts,
                  const ltg_gen_acts* acts, ltg_stream stream) {
    clear_errors();
    if (!g_args_ok(cfg, gen, bt, acts) || !opts) return LTG_EINVAL;
    fwd_stage_enc(cfg, gen, g_route(cfg, gen, bt->n_rows, true), bt, opts, acts, 1, (hipStream_t)stream);
    return check_launch();
}

int ltg_g_fwd_rest(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_pairs* fake,
                   const ltg_fwd_opts* opts, const ltg_gen_acts* acts, float* rowpart_out, void* ws, size_t ws_bytes,
                   ltg_stream stream) {
    clear_errors();
    if (!g_args_ok(cfg, gen, bt, acts) || !opts || !rowpart_out) return LTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* segpart = (ws && ws_bytes >= segpart_bytes(cfg, bt->n_rows))
                         ? reinterpret_cast<float*>((char*)ws + align_up((size_t)bt->n_rows * RP * sizeof(float))) : nullptr;
    const ltg_g_route_info r = g_route(cfg, gen, bt->n_rows, true);
    const int sgroups = fwd_stage_rest(cfg, gen, r, bt, opts, acts, 1, st, segpart);
    g_row_partial(cfg, r, bt, (fake && fake->n > 0) ? fake : nullptr, acts, rowpart_out, st, segpart, nullptr, sgroups);
    return check_launch();
}

int ltg_rowstats_combine(const ltg_config* cfg, const float* rowpart_all, int32_t n_ranks, int32_t n_rows, float* lse_out,
                         void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !rowpart_all || !lse_out || n_ranks < 1 || n_rows < 1 || !ws) return LTG_EINVAL;
    Workspace w;
    if (carve_checked(cfg, n_rows, 1, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    hipLaunchKernelGGL(k_g_combine, dim3(1), dim3(NT), 0, (hipStream_t)stream, n_rows, n_ranks, rowpart_all, 0, (const float*)nullptr,
                       (const float*)nullptr, (const int32_t*)nullptr, 0.f, 0.f, lse_out, w.nb, w.Pb, (float*)nullptr, (float*)nullptr);
    return check_launch();
}

int ltg_g_bwd_dec(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_disc_state* disc, const ltg_batch* bt,
                  const ltg_pairs* fake, const ltg_g_opts* o, const ltg_gen_acts* acts, const float* rowpart_all,
                  int32_t n_ranks, float* loss_out, float* dh2_out, void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!g_args_ok(cfg, gen, bt, acts) || !disc || !fake || !o || !rowpart_all || n_ranks < 1 || !loss_out || !dh2_out || !ws) return LTG_EINVAL;
    if (!o->cnt || !fake->row || fake->n < 0) return LTG_EINVAL;
    Workspace w;
    if (carve_checked(cfg, bt->n_rows, fake->n, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    if (o->y_pre) w.y = const_cast<float*>(o->y_pre);   // y_generated from ltg_fake_tower_batched
    return g_stage_bwd_dec(cfg, gen, disc, g_route(cfg, gen, bt->n_rows, true), bt, fake, o, acts, rowpart_all, n_ranks, loss_out, w, dh2_out, (hipStream_t)stream,
                           (o->fake_done & 1) != 0 || o->y_pre != nullptr);
}

int ltg_g_fake_tower(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* fake, const ltg_g_opts* o, int32_t n_rows, void* ws,
                     size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !disc || !fake || !o || !ws || n_rows <= 0 || fake->n < 0) return LTG_EINVAL;
    Workspace w;   // same carve as ltg_g_bwd_dec: y lives there
    if (carve_checked(cfg, n_rows, fake->n, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    if (fake->n == 0) return LTG_OK;
    fake_tower(cfg, disc, fake, o, w, nullptr, (hipStream_t)stream);
    return check_launch();
}

/* ---- one-shot exchange over peer-mapped staging buffers (csrc/ltg_oneshot.h) ---- */
size_t ltg_oneshot_stage_bytes(int32_t n_ranks, size_t max_floats) {
    if (n_ranks < 1 || n_ranks > LTG_ONESHOT_MAX_RANKS) return 0;
    return os_data_off(n_ranks) + (size_t)2 * n_ranks * max_floats * sizeof(float);
}
size_t ltg_oneshot_expired_offset(int32_t n_ranks) { return ((size_t)2 * n_ranks + 2) * sizeof(uint32_t); }
static int oneshot_exchange(bool gather, const void* sendbuf, void* recvbuf, size_t count, int dtype, int op, void* comm, ltg_stream stream) {
    ltg_oneshot* os = static_cast<ltg_oneshot*>(comm);
    if (!os || !sendbuf || !recvbuf || dtype != LTG_NCCL_FLOAT32 || (!gather && op != LTG_NCCL_SUM) || os->n_ranks < 1 || os->n_ranks > LTG_ONESHOT_MAX_RANKS ||
        os->rank < 0 || os->rank >= os->n_ranks || count > os->max_floats)
        return LTG_EINVAL;
    if (count == 0) return LTG_OK;
    OsView v;
    for (int q = 0; q < LTG_ONESHOT_MAX_RANKS; ++q) v.stage[q] = q < os->n_ranks ? static_cast<char*>(os->stage[q]) : nullptr;
    for (int q = 0; q < os->n_ranks; ++q)
        if (!v.stage[q]) return LTG_EINVAL;
    os->seq += 1u;
    v.R = os->n_ranks;
    v.rank = os->rank;
    v.seq = os->seq;
    v.limit_ms = os->limit_ms;
    v.max_floats = os->max_floats;
    const int nb = (int)((count + OS_NT - 1) / OS_NT);
    const dim3 g(nb < OS_MAX_BLOCKS ? nb : OS_MAX_BLOCKS);
    // (in place: the all-gather's own block is written from `send` -- which may BE that block -- element by element by the thread that read it)
    if (gather) hipLaunchKernelGGL(k_oneshot_exchange<true>, g, dim3(OS_NT), 0, (hipStream_t)stream, v, (const float*)sendbuf, (float*)recvbuf, count);
    else hipLaunchKernelGGL(k_oneshot_exchange<false>, g, dim3(OS_NT), 0, (hipStream_t)stream, v, (const float*)sendbuf, (float*)recvbuf, count);
    return hipGetLastError() == hipSuccess ? LTG_OK : LTG_ELAUNCH;
}
int ltg_oneshot_all_reduce(const void* sendbuf, void* recvbuf, size_t count, int dtype, int op, void* comm, ltg_stream stream) {
    return oneshot_exchange(false, sendbuf, recvbuf, count, dtype, op, comm, stream);
}
int ltg_oneshot_all_gather(const void* sendbuf, void* recvbuf, size_t sendcount, int dtype, void* comm, ltg_stream stream) {
    return oneshot_exchange(true, sendbuf, recvbuf, sendcount, dtype, LTG_NCCL_SUM, comm, stream);
}

int ltg_fake_tower_batched(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* fake, const int32_t* seg_of,
                           const int32_t* seg_row0, const uint64_t* seg_step, float d_keep_prob, float* y_out, void* ws, size_t ws_bytes,
                           ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !disc || !fake || !seg_of || !seg_row0 || !seg_step || !y_out || !ws || fake->n < 0 || !fake->pop || !fake->niche) return LTG_EINVAL;
    if (fake->n == 0) return LTG_OK;
    Workspace w;
    if (carve_checked(cfg, 1, fake->n, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    DropView dv{nullptr, nullptr, 0, 0};
    dv.seg_of = seg_of;
    dv.seg_row0 = seg_row0;
    dv.seg_step = seg_step;
    fake_tower(cfg, disc, fake, dv, dv, dv, d_keep_prob, 0, w, nullptr, (hipStream_t)stream, y_out);
    return check_launch();
}

int ltg_g_bwd_rest(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_pairs* fake,
                   const ltg_g_opts* o, const ltg_gen_acts* acts, const float* dh2, void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!g_args_ok(cfg, gen, bt, acts) || !fake || !o || !dh2 || !ws || o->adam_t < 1) return LTG_EINVAL;
    if (!bt->uptr || !bt->rowidx || !bt->csr_pos) return LTG_EINVAL;
    if (bt->n_unique < 0 || (size_t)bt->n_unique > gq0_rows(cfg, bt->n_rows)) return LTG_EINVAL;
    Workspace w;   // same carve as ltg_g_bwd_dec: dlog lives there
    if (carve_checked(cfg, bt->n_rows, fake->n, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    return g_stage_bwd_rest(cfg, gen, g_route(cfg, gen, bt->n_rows, true), bt, o, acts, w, (hipStream_t)stream, {.dh2 = dh2});
}

int ltg_g_bwd_dec1(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_pairs* fake,
                   const ltg_g_opts* o, const ltg_gen_acts* acts, void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!g_args_ok(cfg, gen, bt, acts) || !fake || !o || !ws || o->adam_t < 1 || o->dec1_done) return LTG_EINVAL;
    Workspace w;   // same carve as ltg_g_bwd_dec: dlog lives there
    if (carve_checked(cfg, bt->n_rows, fake->n, ws, ws_bytes, &w) != LTG_OK) return LTG_EWORKSPACE;
    return g_stage_bwd_rest(cfg, gen, g_route(cfg, gen, bt->n_rows, true), bt, o, acts, w, (hipStream_t)stream, {.only_dec1 = true});
}

/* ---- the item-sharded step as ONE call, exchanges in-stream, weight update and clock slice beside the next step (include/ltg.h) ---- */
int ltg_g_step_sharded_ok(const ltg_config* cfg, const ltg_gen_state* gen, int32_t n_rows) {
    if (!cfg_ok(cfg) || !gen || n_rows <= 0) return 0;
    return g_route(cfg, gen, n_rows).sharded_ok;
}
/* ---- the routes themselves, for callers and tests (host-only; include/ltg.h) ---- */
int ltg_g_route(const ltg_config* cfg, const ltg_gen_state* gen, int32_t n_rows, ltg_g_route_info* out) {
    if (!cfg_ok(cfg) || !gen || n_rows <= 0 || !out) return 0;
    *out = g_route(cfg, gen, n_rows);
    return 1;
}
int ltg_d_route(const ltg_config* cfg, const ltg_disc_state* disc, int32_t n_pairs, int32_t with_bwd, int32_t has_aux, ltg_d_route_info* out) {
    if (!cfg_ok(cfg) || !disc || n_pairs < 0 || !out) return 0;
    *out = d_route(cfg, disc, n_pairs, with_bwd != 0, has_aux != 0);
    return 1;
}

// ltg_pipe.flags: the LTG_PIPE_* switches of include/ltg.h; a pipe with any other bit is refused
constexpr int32_t PIPE_FLAGS = LTG_PIPE_NO_DEC1_FORK | LTG_PIPE_NO_SLICE_FORK | LTG_PIPE_WIDE_GRAD | LTG_PIPE_EVENTS | LTG_PIPE_SLICE_IN_TOUCH | LTG_PIPE_TAIL_OWN;
static bool pipe_ok(const ltg_g_route_info& r, const ltg_pipe* pp) { return r.sharded_ok && (pp->flags & ~PIPE_FLAGS) == 0; }
// the catch-up ahead (include/ltg.h) beyond what the plan implies (device words, the slice on the side stream, the lazy clock): marks, batches
// with their distinct-item lists, a row per workgroup
static bool q0_ahead_capable(const ltg_config* cfg, const ltg_batch* bt, const ltg_pipe* pp) {
    return pp->q0_mark && bt->uitem && bt->uptr && bt->csr_pos && (cfg->h_enc >> 2) <= Q0_NT;
}
// how the pipe's streams meet: a function of the pipe alone (ltg_g_pipe_join has nothing else)
static int pipe_handover(const ltg_pipe* pp) {
    if (pp->flags & LTG_PIPE_NO_DEC1_FORK) return LTG_HAND_ORDER;
    return (pp->sync && (pp->flags & LTG_PIPE_EVENTS) == 0) ? LTG_HAND_WORDS : LTG_HAND_EVENTS;
}
// THE schedule of one ltg_g_step_sharded call (include/ltg.h: ltg_pipe_plan_info): where each stage runs and what it waits for.  Every stage
// below, ltg_g_step_sharded_plan and ltg_g_pipe_plan read this.  Besides it only pipe_ok (the refusal), pipe_handover (a term of it) and
// ltg_g_pipe_join (which has the pipe alone) look at ltg_pipe.flags.  For calls pipe_ok accepts.
static ltg_pipe_plan_info pipe_plan(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_pipe* pp) {
    const int fl = pp->flags;
    ltg_pipe_plan_info p{};
    p.handover = pipe_handover(pp);
    const bool words = p.handover == LTG_HAND_WORDS;
    // the lazy clock's slice of the previous step: on the side stream between this call's catch-up and the next one's (device words: two
    // more of them; beside enc-1 / dec-0 instead of inside the catch-up launch on the critical stream), in this call's catch-up launch
    // (events, or LTG_PIPE_SLICE_IN_TOUCH), or not deferred at all: at the end of its own step
    if (p.handover == LTG_HAND_ORDER || (fl & LTG_PIPE_NO_SLICE_FORK)) p.slice = LTG_SLICE_OWN_END;
    else p.slice = (words && (fl & LTG_PIPE_SLICE_IN_TOUCH) == 0) ? LTG_SLICE_SIDE : LTG_SLICE_IN_TOUCH;
    const bool side = p.slice == LTG_SLICE_SIDE;
    p.ahead = side && q0_ahead_capable(cfg, bt, pp);   // catch-up of the NEXT batch's rows during this call
    p.shadow = words && pp->shadow_out && gen->wp1t_bf16 && pp->shadow_out != gen->wp1t_bf16;   // the update writes the pipe's second shadow buffer
    // the Adam tail (W_p0, W_q1, the biases: it needs dh1's outputs only) on its OWN stream beside the sparse gradient kernel, the next
    // call's catch-up and enc-0; needs <= G0_LIGHT batch rows per partial bias row (its bias job then re-sums them in the same order).
    // OPT-IN (LTG_PIPE_TAIL_OWN).  It was the default without a communicator while the catch-up launch led the critical stream (20 000 items:
    // 146.0-147.1 against 150.9-151.9 us per step).  With the catch-up ahead and two shadow buffers the tail's own chain -- waiter, tail, bias
    // kernel, LTG_WORD_TAIL_END -- is what the next enc-0 then waits for: 20 000 items 142.0-143.6 on its own stream against 139.1-139.5 inline
    // (equal, 138.7-140.4 / 138.1-140.6, once the bias kernel was spread over 8 x as many threads), 200 000 items 802-825 against 745-767; with
    // the three RCCL calls in the stream (per-rank proxy) 154.4-157.0 against 154.6-155.1.
    // (The row bound is 128 rows, which is also the most the one-call step serves (g_route: sharded_ok): true for every accepted call today.)
    p.tail_own = side && pp->tail_stream && pp->ev_tail && (fl & LTG_PIPE_TAIL_OWN) != 0 && (fl & LTG_PIPE_WIDE_GRAD) == 0 &&
                 (bt->n_rows + ENC0_BIAS_PARTS - 1) / ENC0_BIAS_PARTS <= G0_LIGHT;
    // (a ragged slab's last I % 32 rows go through the generic tile kernel behind the streaming one, and that reads h2 throughout:
    // LTG_WORD_H2_READ then opens with LTG_WORD_UPDATE_END)
    p.h2_early = words && (cfg->n_items % 32) == 0;
    p.grad_rows = (fl & LTG_PIPE_WIDE_GRAD) == 0;
    p.poisonable = words;
    return p;
}
int ltg_g_pipe_plan(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_pipe* pp, ltg_pipe_plan_info* out) {
    if (!cfg_ok(cfg) || !gen || !bt || !pp || !out || bt->n_rows <= 0) return 0;
    const ltg_g_route_info r = g_route(cfg, gen, bt->n_rows);
    if (!pipe_ok(r, pp)) return 0;
    *out = pipe_plan(cfg, gen, bt, pp);
    return 1;
}
int ltg_g_step_sharded_plan(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* bt, const ltg_pipe* pp) {
    ltg_pipe_plan_info p;
    if (!ltg_g_pipe_plan(cfg, gen, bt, pp, &p)) return 0;
    return (p.ahead ? LTG_PLAN_AHEAD : 0) | (p.shadow ? LTG_PLAN_SHADOW : 0);
}

int ltg_g_pipe_probe(const ltg_pipe* pipe, ltg_stream stream) {
    clear_errors();
    if (!pipe || !pipe->sync || !pipe->side_stream) return LTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* const probe = pipe->sync + LTG_WORD_PROBE;
    // a waiter on the side stream FIRST, then its producer on `stream`: with one hardware queue under both, the producer cannot start
    // before the waiter has given up (5 ms).  The same for the tail stream when the pipe has one.
    // Pairs (waiter's stream, setter's stream): the caller's stream against each side stream, and -- when the pipe has both -- the tail
    // stream against the side stream: they never wait for each other, but in one queue the Adam tail would sit behind the ~100-us weight
    // update and the next call's enc-0, which polls for the tail's end, with it (seen in round 4: a process with many streams alive put
    // both onto one hardware queue: 180 instead of 147 us per step at 20 000 items).
    for (int which = 0; which < 3; ++which) {
        hipStream_t sd = (hipStream_t)(which == 0 ? pipe->side_stream : pipe->tail_stream);
        hipStream_t sp = which == 2 ? (hipStream_t)pipe->side_stream : st;
        if (!sd || (which == 2 && !pipe->side_stream)) continue;     // (`stream` itself may be the null stream: handle 0)
        unsigned zero[2] = {0u, 0u}, got[2] = {0u, 0u};
        if (hipStreamSynchronize(sd) != hipSuccess || hipStreamSynchronize(sp) != hipSuccess) return LTG_ELAUNCH;
        if (hipMemcpy(probe, zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess) return LTG_ELAUNCH;
        hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, sd, LtgGate{probe, 1u, probe + 1, 5});   // (gives up after 5 ms, counted in the word behind)
        hipLaunchKernelGGL(k_gate_set, dim3(1), dim3(64), 0, sp, LtgGate{probe, 1u, nullptr, 0});
        if (hipStreamSynchronize(sd) != hipSuccess || hipStreamSynchronize(sp) != hipSuccess) return LTG_ELAUNCH;
        if (hipMemcpy(got, probe, sizeof(got), hipMemcpyDeviceToHost) != hipSuccess) return LTG_ELAUNCH;
        if (check_launch() != LTG_OK) return LTG_ELAUNCH;
        if (!(got[0] == 1u && got[1] == 0u)) return 0;
    }
    return 1;
}

int ltg_g_pipe_join(const ltg_pipe* pipe, ltg_stream stream) {
    clear_errors();
    if (!pipe || !pipe->ev_dec1 || !pipe->side_stream) return LTG_EINVAL;
    // device words: nothing was recorded per call -- everything on the side stream so far.  (Not pipe_handover() == LTG_HAND_WORDS: a pipe with
    // words under LTG_PIPE_NO_DEC1_FORK, LTG_HAND_ORDER, has always had this record on its idle side stream, and keeps it.)
    if (pipe->sync && (pipe->flags & LTG_PIPE_EVENTS) == 0) {
        if (hipEventRecord((hipEvent_t)pipe->ev_dec1, (hipStream_t)pipe->side_stream) != hipSuccess) return LTG_ELAUNCH;
    }
    if (hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)pipe->ev_dec1, 0) != hipSuccess) return LTG_ELAUNCH;
    if (pipe->tail_stream && pipe->ev_tail) {   // the Adam tail of the last call (its own stream in the device-word mode)
        if (hipEventRecord((hipEvent_t)pipe->ev_tail, (hipStream_t)pipe->tail_stream) != hipSuccess) return LTG_ELAUNCH;
        if (hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)pipe->ev_tail, 0) != hipSuccess) return LTG_ELAUNCH;
    }
    return LTG_OK;
}

// ---- ltg_g_step_sharded, stage by stage.  A stage reads the call (GSharded) and what it needs of the route and the plan; the entry point runs them in this
// order, which IS the host's issue order of the launches.  What each device word means: include/ltg.h, enum ltg_word.  Every poll is made by
// ONE thread, either a one-wave kernel of the side stream or the last thread of the kernel in front of the one that needs the gate: no
// workgroup of a large launch ever holds a CU while it waits for a producer that still needs one.  Schedules that were measured and
// removed: DESIGN.md 5.4, "Tried and not kept".
struct GSharded {
    const ltg_config* cfg;
    const ltg_gen_state* gen;
    const ltg_disc_state* disc;
    const ltg_batch* bt;
    const ltg_pairs* fake;
    const ltg_g_opts* o;
    const ltg_gen_acts* acts;
    const ltg_comm* comm;
    const ltg_pipe* pp;
    float* loss_out;
    ltg_stream stream;         // the caller's stream as the collectives take it ...
    hipStream_t st, sd, stl;   // ... as HIP does; the side stream; the tail stream
    int R;                     // ranks
    Workspace w;
    float* rowpart;            // this rank's block of the all-gather buffer: the exchange is in place
    AdamC ad;
    const unsigned* poison;    // plan.poisonable: LTG_WORD_POISON
    Probe pr;
    // the pipe's words as gates of THIS call's ordinal (prev: the call before)
    LtgGate store(int word) const { return gate_store(pp->sync, word, pp->seq); }
    LtgGate poll(int word) const { return gate_poll(pp->sync, word, pp->seq); }
    LtgGate poll_prev(int word) const { return gate_poll(pp->sync, word, pp->seq - 1u); }
};
#define LTG_HIP(x) do { if ((x) != hipSuccess) return LTG_ELAUNCH; } while (0)
#define LTG_COMM(x) do { if ((x) != 0) return LTG_ELAUNCH; } while (0)

// the clock slice forked by the PREVIOUS call is done (it must not meet the catch-up on a row); the rows this batch reads
static void gs_catch_up(const GSharded& c, const ltg_g_route_info& r, const ltg_pipe_plan_info& p) {
    const ltg_gen_state* gen = c.gen;
    const ltg_batch* bt = c.bt;
    const int I = c.cfg->n_items, qP = gen->q0_period;
    if (p.slice == LTG_SLICE_IN_TOUCH && gen->q0_ord > 0 && gen->q0_ord % qP < I) {
        const int start = gen->q0_ord % qP, ns = (I - start + qP - 1) / qP;
        hipLaunchKernelGGL(k_q0_touch_slice, dim3(bt->n_unique + ns), dim3(Q0_NT), 0, c.st, I, c.cfg->h_enc, bt->n_unique, bt->uptr, bt->csr_pos, bt->indices, bt->uitem,
                           gen->q0_ord, start, qP, *gen, make_adam(c.cfg, 1));
    } else if (p.ahead && c.pp->caught_up) {
        // the previous call brought this batch's rows up to q0_ord on the side stream (k_q0_touch_ahead; its end is behind
        // LTG_WORD_SLICE_DONE, which that call's last kernel on this stream waited for) and marked them: no catch-up launch
    } else if (p.slice == LTG_SLICE_SIDE) {
        // (the previous call's last kernel waited for LTG_WORD_SLICE_DONE before it ended: ltg_gate_wait_tail in fk_g_tail)
        q0_touch(c.cfg, gen, r, bt, c.st, c.poison, p.ahead ? c.pp->q0_mark : nullptr, c.pp->seq);
    } else
        q0_touch(c.cfg, gen, r, bt, c.st, c.poison);
}

// forward, encoder half: enc-0 over the local slab (exchange 1 follows the side stream's launches: gs_forward)
static void gs_enc0(const GSharded& c, const ltg_g_route_info& r, const ltg_pipe_plan_info& p) {
    ltg_gen_acts a1 = *c.acts;
    a1.h1 = c.pp->h1pre;
    fwd_stage_enc(c.cfg, c.gen, r, c.bt, &c.o->fwd, &a1, 1, c.st, {.touched = true, .started = p.slice == LTG_SLICE_SIDE ? c.store(LTG_WORD_CATCHUP) : LTG_NO_GATE,
                                                                  .end_wait = p.tail_own ? c.poll_prev(LTG_WORD_TAIL_END) : LTG_NO_GATE});
}

// the side stream's clock work: the slice step t - 1 owes (rows i = ord (mod period) up to ord) between this call's catch-up and the next
// call's, then the catch-up ahead.  LTG_WORD_CATCHUP is opened by enc-0 when it starts (the catch-up in front of it is complete: the rows of
// this batch are at ord, the slice skips them whatever happens to them later), a one-wave kernel in front of the sweep polls for it;
// LTG_WORD_SLICE_DONE is opened by the side stream's next kernel (the waiter in front of the weight update) when it starts.  (Issued in the
// order the device needs them: the critical stream's kernels first.)
static void gs_side_clock(const GSharded& c, const ltg_pipe_plan_info& p) {
    if (p.slice != LTG_SLICE_SIDE) return;
    const ltg_gen_state* gen = c.gen;
    const ltg_pipe* pp = c.pp;
    const int I = c.cfg->n_items, H = c.cfg->h_enc, qP = gen->q0_period, start = gen->q0_ord % qP;
    hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, c.sd, c.poll(LTG_WORD_CATCHUP), LTG_NO_GATE);
    if (gen->q0_ord > 0 && start < I)
        hipLaunchKernelGGL(k_q0_sweep, dim3((I - start + qP - 1) / qP), dim3(Q0_NT), 0, c.sd, I, H, start, qP, gen->q0_ord, *gen, make_adam(c.cfg, 1), c.poison);
    if (p.ahead && pp->next_uitem && pp->next_nu > 0)
        hipLaunchKernelGGL(k_q0_touch_ahead, dim3(pp->next_nu), dim3(Q0_NT), 0, c.sd, H, pp->next_nu, pp->next_uitem, gen->q0_ord + 1, *gen, c.ad, pp->q0_mark,
                           pp->seq, c.poison);
}

// forward: exchange 1 -> enc-1 (bias + tanh in its loader), dec-0, local logits + statistics -> exchange 2
static int gs_forward(const GSharded& c, const ltg_g_route_info& r, const ltg_pipe_plan_info& p) {
    const ltg_config* cfg = c.cfg;
    const ltg_gen_state* gen = c.gen;
    const ltg_g_opts* o = c.o;
    const ltg_gen_acts* acts = c.acts;
    const ltg_comm* comm = c.comm;
    const ltg_pipe* pp = c.pp;
    const Probe& pr = c.pr;
    hipStream_t st = c.st;
    const int B = c.bt->n_rows, H = cfg->h_enc, Z = cfg->z_dim;
    const bool words = p.handover == LTG_HAND_WORDS;
    if (comm) LTG_PROBED(pr, LTG_K_EXCH_H1, LTG_COMM(comm->all_reduce(pp->h1pre, pp->h1pre, (size_t)B * H, LTG_NCCL_FLOAT32, LTG_NCCL_SUM, comm->comm, c.stream)));
    LTG_PROBED(pr, LTG_K_ENC1, hipLaunchKernelGGL(fk_enc1<true>, grid2(Z, B, 16, 16), dim3(ENC1_NT), 0, st, B, H, Z, pp->h1pre, gen->p[1], gen->p[5], o->fwd.eps,
                                                  o->fwd.is_training, cfg->seed, o->fwd.rng_step, acts->mulv, acts->z, gen->p[4], acts->h1,
                                                  words ? c.poll_prev(LTG_WORD_H2_READ) : LTG_NO_GATE));
    // (dec-0 overwrites h2, which the previous step's weight update reads in its prologue: enc-1's last thread polled for LTG_WORD_H2_READ --
    // or, with events, the stream waits for the whole update; the streaming forward behind dec-0 needs the update's END: LTG_WORD_UPDATE_END)
    if (p.handover == LTG_HAND_EVENTS) LTG_HIP(hipStreamWaitEvent(st, (hipEvent_t)pp->ev_dec1, 0));
    LTG_PROBED(pr, LTG_K_DEC0, hipLaunchKernelGGL(fk_dec0, grid2(H, B, 16, 16), dim3(NT), 0, st, B, H, Z, acts->z, acts->mulv, gen->p[2], gen->p[6], acts->kl_rows,
                                                  acts->h2, words ? c.poll_prev(LTG_WORD_UPDATE_END) : LTG_NO_GATE, c.poison));
    int G = 0;
    LTG_PROBED(pr, LTG_K_DEC1_FWD, G = launch_dec1_fwd_stream(cfg, gen, r, B, acts, c.w.segpart, st));
    g_row_partial(cfg, r, c.bt, c.fake->n > 0 ? c.fake : nullptr, acts, c.rowpart, st, c.w.segpart, nullptr, G);
    if (comm) LTG_PROBED(pr, LTG_K_EXCH_ROWPART, LTG_COMM(comm->all_gather(c.rowpart, pp->rowpart_all, (size_t)B * RP, LTG_NCCL_FLOAT32, comm->comm, c.stream)));
    return LTG_OK;
}

// backward: (fake tower when it was not evaluated ahead,) losses + dlogits
static void gs_losses(const GSharded& c) {
    const ltg_batch* bt = c.bt;
    const ltg_pairs* fake = c.fake;
    const ltg_g_opts* o = c.o;
    const Workspace& w = c.w;
    const int B = bt->n_rows, I = c.cfg->n_items, nf = fake->n;
    if (nf > 0 && !o->y_pre && !(o->fake_done & 1)) fake_tower(c.cfg, c.disc, fake, o, w, o->probe, c.st);
    hipLaunchKernelGGL(k_dlogits_combine<true>, dim3((I + DL_SEG - 1) / DL_SEG, B), dim3(NT), 0, c.st, B, I, c.R, bt->indptr, bt->indices, bt->values, c.acts->logits,
                       c.pp->rowpart_all, c.acts->kl_rows, nf > 0 ? w.y : (const float*)nullptr, o->cnt, o->anneal, o->gan_lambda, nf, fake->row, fake->niche, fake->pop,
                       w.dlog, c.acts->lse, w.scal, c.loss_out, c.cfg->item_lo);
}

// the dh2 product, then ONE fork behind it (the last reader of this step's W_p1t shadow) onto the side stream: the decoder weight update
// (needs dlogits and h2 only; joined before the NEXT step's dec-0), then the slab sum + exchange 3.
// Two shadow buffers (plan.shadow): the update of this call writes the OTHER buffer, so the dh2 product leaves the cycle update -> streaming
// forward -> dlogits -> [dh2 product] -> update that bounds the step at 20 000 - 25 000 items: LTG_WORD_DH2_DONE opens when the product
// STARTS (dlogits is complete), not when it has ended.
static int gs_dh2_update(const GSharded& c, const ltg_g_route_info& r, const ltg_pipe_plan_info& p) {
    const ltg_config* cfg = c.cfg;
    const ltg_gen_state* gen = c.gen;
    const ltg_pipe* pp = c.pp;
    const Workspace& w = c.w;
    hipStream_t st = c.st, sd = c.sd;
    const int B = c.bt->n_rows, I = cfg->n_items, H = cfg->h_enc, nsplit = r.dh2_nsplit, n_da2 = B * H;
    const bool words = p.handover == LTG_HAND_WORDS, events = p.handover == LTG_HAND_EVENTS;
    LTG_PROBED(c.pr, LTG_K_DH2, hipLaunchKernelGGL((k_dh2_stream<true, DH2_NH>), dim3(nsplit, DH2_NH), dim3(ST_NT), (size_t)2 * ST_BN * ST_LDW * 2, st, B, I, H, r.dh2_chunk,
                                                   w.dlog, gen->wp1t_bf16, w.part, p.shadow ? c.store(LTG_WORD_DH2_DONE) : LTG_NO_GATE));
    if (words) {
        // the slab sum first: it is the next kernel of the critical stream, the side stream's launches take the host ~30 us
        hipLaunchKernelGGL(k_da2, grid1(n_da2, 2048), dim3(NT), 0, st, n_da2, nsplit, w.part, (const float*)nullptr,
                           pp->dh2, p.shadow ? LTG_NO_GATE : c.store(LTG_WORD_DH2_DONE));
        // the side stream's work starts behind a one-wave kernel that polls the word the slab sum (or the product) sets when it starts
        hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, sd, c.poll(LTG_WORD_DH2_DONE), p.slice == LTG_SLICE_SIDE ? c.store(LTG_WORD_SLICE_DONE) : LTG_NO_GATE);
    } else if (events) {
        LTG_HIP(hipEventRecord((hipEvent_t)pp->ev_fork, st));
        LTG_HIP(hipStreamWaitEvent(sd, (hipEvent_t)pp->ev_fork, 0));
    }
    const LtgH2Done hd_last = p.h2_early ? LtgH2Done{pp->sync + LTG_WORD_H2_COUNT, pp->sync + LTG_WORD_H2_READ, pp->seq, c.poison} : LtgH2Done{nullptr, nullptr, 0u, c.poison};
    ltg_g_opts od = *c.o;
    od.dec1_done = 0;   // the one call always runs the update itself, whatever cut-point options the caller reuses say
    ltg_gen_state gen_dw = *gen;
    if (p.shadow) gen_dw.wp1t_bf16 = pp->shadow_out;   // (the caller exchanges the two pointers after the call)
    const int rc = g_stage_bwd_rest(cfg, &gen_dw, r, c.bt, &od, c.acts, w, p.handover == LTG_HAND_ORDER ? st : sd, {.only_dec1 = true, .hd = hd_last});
    if (rc != LTG_OK) return rc;
    if (words) hipLaunchKernelGGL(k_gate_set, dim3(1), dim3(64), 0, sd, c.store(LTG_WORD_UPDATE_END), p.h2_early ? LTG_NO_GATE : c.store(LTG_WORD_H2_READ));
    else if (events) LTG_HIP(hipEventRecord((hipEvent_t)pp->ev_dec1, sd));
    if (!words) hipLaunchKernelGGL(k_da2, grid1(n_da2, 2048), dim3(NT), 0, st, n_da2, nsplit, w.part, (const float*)nullptr, pp->dh2);
    if (c.comm) LTG_PROBED(c.pr, LTG_K_EXCH_DH2, LTG_COMM(c.comm->all_reduce(pp->dh2, pp->dh2, (size_t)B * H, LTG_NCCL_FLOAT32, LTG_NCCL_SUM, c.comm->comm, c.stream)));
    return LTG_OK;
}

// the replicated rest: dz (tanh derivative in its loader) -> dh1 -> sparse W_q0 gradient + its Adam step -> the other updates (the tail)
static void gs_rest(const GSharded& c, const ltg_pipe_plan_info& p) {
    const ltg_config* cfg = c.cfg;
    const ltg_gen_state* gen = c.gen;
    const ltg_g_opts* o = c.o;
    const ltg_gen_acts* acts = c.acts;
    const Workspace& w = c.w;
    hipStream_t st = c.st;
    const int B = c.bt->n_rows, I = cfg->n_items, H = cfg->h_enc, Z = cfg->z_dim;
    LTG_PROBED(c.pr, LTG_K_DZ, hipLaunchKernelGGL(fk_dz_dh2, grid2(Z, B, 16, 16), dim3(NT), 0, st, B, Z, H, c.pp->dh2, acts->h2, gen->p[2], acts->mulv, o->fwd.eps,
                                                  o->fwd.is_training, o->anneal, cfg->seed, o->fwd.rng_step, w.dmlv, w.da2));
    LTG_PROBED(c.pr, LTG_K_DH1, hipLaunchKernelGGL(fk_dh1, grid2(H, B, 16, 16), dim3(NT), 0, st, B, H, 2 * Z, w.dmlv, gen->p[1], acts->h1, w.da1));
    // the step's last kernel on the caller's stream waits for the clock's work on the side stream
    const LtgGate slice_done = p.slice == LTG_SLICE_SIDE ? c.poll(LTG_WORD_SLICE_DONE) : LTG_NO_GATE;
    if (p.tail_own) {
        g_enc0_grad(cfg, c.bt, o, acts, w, st, {.gen = gen, .ad = &c.ad, .row_waves = true, .poison = c.poison, .started = c.store(LTG_WORD_DH1_DONE),
                                               .end_wait = slice_done, .lr_slot = gen->q0_lr_hist + ((gen->q0_ord + 1) & (LTG_Q0_HIST - 1))});
        hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, c.stl, c.poll(LTG_WORD_DH1_DONE), LTG_NO_GATE);
        g_jobs(cfg, gen, c.bt, o, acts, w, c.ad, c.stl, {.no_q0 = true, .q0_bias = true, .poison = c.poison, .bias_from_da1 = true});
        hipLaunchKernelGGL(k_gate_set, dim3(1), dim3(64), 0, c.stl, c.store(LTG_WORD_TAIL_END), LTG_NO_GATE);
    } else {
        g_enc0_grad(cfg, c.bt, o, acts, w, st, {.gen = gen, .ad = &c.ad, .row_waves = p.grad_rows != 0, .poison = c.poison});
        g_jobs(cfg, gen, c.bt, o, acts, w, c.ad, st, {.no_q0 = true, .q0_bias = true, .poison = c.poison, .end_wait = slice_done});
    }
    if (p.slice == LTG_SLICE_OWN_END) {   // the slice of THIS step at its end, in program order (the cut-point schedule)
        const int qP = gen->q0_period, ord = gen->q0_ord + 1, start = ord % qP;
        if (start < I) hipLaunchKernelGGL(k_q0_sweep, dim3((I - start + qP - 1) / qP), dim3(Q0_NT), 0, st, I, H, start, qP, ord, *gen, make_adam(cfg, 1));
    }
}
#undef LTG_HIP
#undef LTG_COMM

int ltg_g_step_sharded(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_disc_state* disc, const ltg_batch* bt,
                       const ltg_pairs* fake, const ltg_g_opts* o, const ltg_gen_acts* acts, const ltg_comm* comm,
                       const ltg_pipe* pp, float* loss_out, void* ws, size_t ws_bytes, ltg_stream stream) {
    clear_errors();
    if (!g_args_ok(cfg, gen, bt, acts) || !disc || !fake || !o || !pp || !loss_out || !ws || o->adam_t < 1) return LTG_EINVAL;
    if (!bt->uptr || !bt->rowidx || !bt->csr_pos || !o->cnt || !fake->row || fake->n < 0) return LTG_EINVAL;
    if (bt->n_unique < 0 || (size_t)bt->n_unique > gq0_rows(cfg, bt->n_rows)) return LTG_EINVAL;
    const ltg_g_route_info r = g_route(cfg, gen, bt->n_rows);
    if (!pipe_ok(r, pp) || !pp->side_stream || !pp->ev_fork || !pp->ev_dec1 || !pp->h1pre || !pp->rowpart_all || !pp->dh2) return LTG_EINVAL;
    const int R = comm ? comm->n_ranks : 1, rank = comm ? comm->rank : 0;
    if (R < 1 || rank < 0 || rank >= R || (comm && (!comm->all_reduce || !comm->all_gather))) return LTG_EINVAL;
    const ltg_pipe_plan_info p = pipe_plan(cfg, gen, bt, pp);
    hipStream_t st = (hipStream_t)stream;
    GSharded c{cfg, gen, disc, bt, fake, o, acts, comm, pp, loss_out, stream, st, (hipStream_t)pp->side_stream, (hipStream_t)pp->tail_stream, R};
    if (carve_checked(cfg, bt->n_rows, fake->n, ws, ws_bytes, &c.w) != LTG_OK) return LTG_EWORKSPACE;
    if (o->y_pre) c.w.y = const_cast<float*>(o->y_pre);   // y_generated from ltg_fake_tower_batched
    c.rowpart = pp->rowpart_all + (size_t)rank * bt->n_rows * RP;
    c.ad = make_adam(cfg, o->adam_t);
    c.poison = p.poisonable ? pp->sync + LTG_WORD_POISON : nullptr;
    c.pr = Probe{o->probe, st};
    gs_catch_up(c, r, p);
    gs_enc0(c, r, p);
    gs_side_clock(c, p);
    if (const int rc = gs_forward(c, r, p)) return rc;
    gs_losses(c);
    if (const int rc = gs_dh2_update(c, r, p)) return rc;
    gs_rest(c, p);
    return check_launch();
}

int ltg_refresh_d_shadow(const ltg_config* cfg, const ltg_disc_state* d, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !d || !d->emb || !d->emb_fp8 || !d->w1t_fp8 || !d->w2t_fp8 || !d->w3t_fp8) return LTG_EINVAL;
    hipLaunchKernelGGL(k_d_shadow, dim3(2048), dim3(NT), 0, (hipStream_t)stream, cfg->d_feat, cfg->d_h0, cfg->d_h1, cfg->d_h2, cfg->d_h3, d->emb, d->p[0],
                       d->p[2], d->p[4], const_cast<uint8_t*>(d->emb_fp8), d->w1t_fp8, d->w2t_fp8, d->w3t_fp8, d->w3_fp8);
    return check_launch();
}

int ltg_g_flush(const ltg_config* cfg, const ltg_gen_state* gen, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !gen || !q0_lazy(cfg, gen)) return LTG_EINVAL;
    const int I = cfg->n_items;
    hipLaunchKernelGGL(k_q0_sweep, dim3(I < 65536 ? I : 65536), dim3(Q0_NT), 0, (hipStream_t)stream, I, cfg->h_enc, 0, 1, gen->q0_ord, *gen, make_adam(cfg, 1));
    return check_launch();
}

int ltg_refresh_shadow(const ltg_config* cfg, const ltg_gen_state* gen, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !gen || !gen->wp1t_bf16 || cfg->h_enc > ST_KP) return LTG_EINVAL;
    const size_t total = (size_t)cfg->n_items * ST_KP;
    size_t gx = (total + NT - 1) / NT;
    if (gx > 65536) gx = 65536;
    hipLaunchKernelGGL(k_refresh_shadow, dim3((unsigned)gx), dim3(NT), 0, (hipStream_t)stream, cfg->n_items, cfg->h_enc, gen->p[3], gen->wp1t_bf16);
    return check_launch();
}

int ltg_gather_cand_logits(const ltg_config* cfg, const ltg_sample_inputs* in, const float* logits, float* out, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !in || !logits || !out || in->n_rows < 0) return LTG_EINVAL;
    if (in->n_rows == 0) return LTG_OK;
    hipLaunchKernelGGL(k_gather_cand, dim3(in->n_rows), dim3(NT), 0, (hipStream_t)stream, cfg->n_items, cfg->item_lo, in->cand_ptr,
                       in->cand_idx, logits, out);
    return check_launch();
}

int ltg_rank_metrics(const ltg_config* cfg, const float* logits, const ltg_batch* tr, const ltg_batch* te, int32_t k_ndcg,
                     int32_t k_r1, int32_t k_r2, float* out, ltg_stream stream) {
    clear_errors();
    if (!cfg_ok(cfg) || !logits || !tr || !te || !out || tr->n_rows != te->n_rows || tr->n_rows < 0) return LTG_EINVAL;
    if (tr->n_rows == 0) return LTG_OK;
    const size_t lds = (size_t)((cfg->n_items + 31) / 32) * sizeof(unsigned);
    if (lds > 64 * 1024) return LTG_EINVAL;
    hipLaunchKernelGGL(k_rank_metrics, dim3(tr->n_rows), dim3(NT), lds, (hipStream_t)stream, cfg->n_items, cfg->item_lo, logits,
                       tr->indptr, tr->indices, te->indptr, te->indices, (const float*)nullptr, (int32_t*)nullptr, k_ndcg, k_r1, k_r2, out);
    return check_launch();
}

// ltg_topk and ltg_topk_groups: one launch of k_topk; labels == nullptr is the plain instantiation, which never reads the last two arguments.
// Every refusal comes before the first HIP call.
static int topk_launch(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, const uint8_t* labels,
                       uint32_t group_mask, float* score_out, int32_t* id_out, ltg_stream stream) {
    if (!cfg || !logits || !score_out || !id_out || cfg->n_items <= 0 || n_rows < 0 || k < 1 || k > 1024) return LTG_EINVAL;
    if (tr && (!tr->indptr || !tr->indices || tr->n_rows != n_rows)) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    // dynamic LDS: the fold-in bitset, then the candidate buffer (64-bit words; the largest power of two <= 4096 that fits, >= 1024)
    const size_t bits = (size_t)((cfg->n_items + 63) / 64) * 8;
    size_t cap = 4096;
    while (cap >= 1024 && bits + cap * 8 > 60 * 1024) cap >>= 1;
    if (cap < 1024) return LTG_EINVAL;
    const size_t lds = bits + cap * 8;
    clear_errors();
    const bool vec = (cfg->n_items % 4) == 0 && ((uintptr_t)logits % 16) == 0;
    auto kern = labels ? (vec ? k_topk<true, true> : k_topk<false, true>) : (vec ? k_topk<true, false> : k_topk<false, false>);
    hipLaunchKernelGGL(kern, dim3(n_rows), dim3(TK_NT), lds, (hipStream_t)stream, cfg->n_items, cfg->item_lo, logits,
                       tr ? tr->indptr : (const int32_t*)nullptr, tr ? tr->indices : (const int32_t*)nullptr, k, (int)cap, score_out, id_out,
                       labels, group_mask);
    return check_launch();
}

int ltg_topk(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, float* score_out, int32_t* id_out,
             ltg_stream stream) {
    return topk_launch(cfg, logits, tr, n_rows, k, nullptr, 0u, score_out, id_out, stream);
}

int ltg_topk_groups(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, const uint8_t* item_group,
                    int32_t n_items_global, uint32_t group_mask, float* score_out, int32_t* id_out, ltg_stream stream) {
    if (!cfg || !item_group || group_mask == 0u || group_mask > 0x1FFu || cfg->item_lo < 0 || cfg->n_items <= 0 ||
        (int64_t)cfg->item_lo + cfg->n_items > (int64_t)n_items_global)
        return LTG_EINVAL;
    return topk_launch(cfg, logits, tr, n_rows, k, item_group + cfg->item_lo, group_mask, score_out, id_out, stream);
}

int ltg_topk_merge(int32_t n_parts, int32_t n_rows, int32_t k_in, const float* score_in, const int32_t* id_in, int32_t k, float* score_out,
                   int32_t* id_out, ltg_stream stream) {
    clear_errors();
    if (!score_in || !id_in || !score_out || !id_out || n_parts < 1 || n_rows < 0 || k_in < 1 || k_in > 1024 || k < 1 || k > 1024)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    hipLaunchKernelGGL(k_topk_merge, dim3(n_rows), dim3(NT), 0, (hipStream_t)stream, n_parts, n_rows, k_in, score_in, id_in, k, score_out,
                       id_out);
    return check_launch();
}

// Exploration lists: the draw, the mass and the log-probabilities, cut where item shards exchange.  What ltg_topk refuses is
// refused here in the same words, and the dynamic LDS is sized as topk_launch sizes it (cap = 0: the slab is too long).
static bool explore_args_ok(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, float inv_temp,
                            const int32_t* excl_id, int32_t f_in, size_t* bits, size_t* cap) {
    if (!cfg || !logits || cfg->n_items <= 0 || cfg->item_lo < 0 || n_rows < 0 || k < 1 || k > 1024) return false;
    if (tr && (!tr->indptr || !tr->indices || tr->n_rows != n_rows)) return false;
    if (f_in < 0 || (f_in > 0 && !excl_id) || !std::isfinite(inv_temp) || !(inv_temp > 0.f)) return false;
    *bits = (size_t)((cfg->n_items + 63) / 64) * 8;
    *cap = 4096;
    while (*cap >= 1024 && *bits + *cap * 8 > 60 * 1024) *cap >>= 1;
    return *cap >= 1024;
}

int ltg_topk_sample(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t row_lo, int32_t k, float inv_temp,
                    uint64_t draw, const int32_t* excl_id, int32_t f_in, const float* g_noise, float* key_out, int32_t* id_out,
                    ltg_stream stream) {
    size_t bits, cap;
    if (!key_out || !id_out || row_lo < 0 || !explore_args_ok(cfg, logits, tr, n_rows, k, inv_temp, excl_id, f_in, &bits, &cap)) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    const bool vec = (cfg->n_items % 4) == 0 && ((uintptr_t)logits % 16) == 0;
    const uint64_t i_glob = (uint64_t)(cfg->n_items_global > 0 ? cfg->n_items_global : cfg->n_items);
    hipLaunchKernelGGL(vec ? k_topk_sample<true> : k_topk_sample<false>, dim3(n_rows), dim3(TK_NT), bits + cap * 8, (hipStream_t)stream,
                       cfg->n_items, cfg->item_lo, i_glob, logits, tr ? tr->indptr : (const int32_t*)nullptr,
                       tr ? tr->indices : (const int32_t*)nullptr, k, (int)cap, inv_temp, cfg->seed, draw, row_lo, excl_id, f_in, g_noise, key_out,
                       id_out);
    return check_launch();
}

int ltg_topk_sample_mass(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, float inv_temp,
                         const int32_t* excl_id, int32_t f_in, const int32_t* id_in, float* score_out, float* max_out, float* rest_out,
                         ltg_stream stream) {
    size_t bits, cap;
    if (!id_in || !score_out || !max_out || !rest_out || !explore_args_ok(cfg, logits, tr, n_rows, k, inv_temp, excl_id, f_in, &bits, &cap))
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    const bool vec = (cfg->n_items % 4) == 0 && ((uintptr_t)logits % 16) == 0;
    hipLaunchKernelGGL(vec ? k_topk_sample_mass<true> : k_topk_sample_mass<false>, dim3(n_rows), dim3(TK_NT), bits, (hipStream_t)stream,
                       cfg->n_items, cfg->item_lo, logits, tr ? tr->indptr : (const int32_t*)nullptr, tr ? tr->indices : (const int32_t*)nullptr, k,
                       inv_temp, excl_id, f_in, id_in, score_out, max_out, rest_out);
    return check_launch();
}

int ltg_topk_sample_finish(int32_t n_rows, int32_t k, const float* score, const float* M, const float* rest, float inv_temp, float* logp_out,
                           ltg_stream stream) {
    if (!score || !M || !rest || !logp_out || n_rows < 0 || k < 1 || k > 1024 || !std::isfinite(inv_temp) || !(inv_temp > 0.f)) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    hipLaunchKernelGGL(k_topk_sample_finish, dim3((n_rows + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, (hipStream_t)stream, n_rows, k, score, M, rest,
                       inv_temp, logp_out);
    return check_launch();
}

// Posterior-aware scores.  Every refusal comes before the first HIP call.
static bool post_samples_ok(int32_t s) { return s == 1 || s == 4 || s == 8 || s == 16 || s == 32; }
static bool post_args_ok(const ltg_config* cfg, const ltg_gen_state* gen, const uint16_t* image, int32_t n_rows, int32_t n_samples) {
    return cfg_ok(cfg) && cfg->item_lo >= 0 && gen && gen->p[3] && gen->p[7] && image && ((uintptr_t)image % 16) == 0 && n_rows >= 0 &&
           post_samples_ok(n_samples) && (int64_t)n_rows * n_samples < (int64_t)1 << 31;
}

int32_t ltg_posterior_ld(const ltg_config* cfg) { return cfg_ok(cfg) ? (cfg->h_enc + 31) / 32 * 32 : 0; }

size_t ltg_posterior_image_bytes(const ltg_config* cfg, int32_t n_rows, int32_t n_samples) {
    if (!cfg_ok(cfg) || n_rows < 0 || !post_samples_ok(n_samples) || (int64_t)n_rows * n_samples >= (int64_t)1 << 31) return 0;
    return (size_t)n_rows * n_samples * ltg_posterior_ld(cfg) * sizeof(uint16_t);
}

int ltg_posterior_h2(const ltg_config* cfg, const ltg_gen_state* gen, const float* mulv, int32_t n_rows, int32_t row_lo, int32_t n_samples,
                     uint64_t draw, const float* eps, uint16_t* image_out, float* z_out, ltg_stream stream) {
    if (!cfg_ok(cfg) || !gen || !gen->p[2] || !gen->p[6] || !mulv || !image_out || n_rows < 0 || row_lo < 0 || !post_samples_ok(n_samples) ||
        (int64_t)n_rows * n_samples >= (int64_t)1 << 31)
        return LTG_EINVAL;
    const size_t lds = (size_t)n_samples * cfg->z_dim * sizeof(float);
    if (lds > 64 * 1024) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
#define LTG_POST_H2(SV)                                                                                                                   \
    hipLaunchKernelGGL(k_post_h2<SV>, dim3(n_rows), dim3(PO_NT), lds, (hipStream_t)stream, cfg->z_dim, cfg->h_enc, ltg_posterior_ld(cfg), \
                       mulv, eps, cfg->seed, draw, row_lo, gen->p[2], gen->p[6], image_out, z_out)
    switch (n_samples) {
        case 1: LTG_POST_H2(1); break;
        case 4: LTG_POST_H2(4); break;
        case 8: LTG_POST_H2(8); break;
        case 16: LTG_POST_H2(16); break;
        default: LTG_POST_H2(32); break;
    }
#undef LTG_POST_H2
    return check_launch();
}

int ltg_posterior_scores(const ltg_config* cfg, const ltg_gen_state* gen, const uint16_t* image, int32_t n_rows, int32_t n_samples, float beta,
                         float* score_out, float* spread_out, ltg_stream stream) {
    if (!post_args_ok(cfg, gen, image, n_rows, n_samples) || !score_out || !std::isfinite(beta) || (n_samples == 1 && beta != 0.f))
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const int M = n_rows * n_samples, I = cfg->n_items, ld = ltg_posterior_ld(cfg);
    // item segments: enough workgroups to fill the chip when the row blocks alone do not
    const int rb = (M + PO_ROWS - 1) / PO_ROWS, steps = (I + PO_STEP - 1) / PO_STEP;
    int nseg = rb >= 1024 ? 1 : (1024 + rb - 1) / rb;
    if (nseg > steps) nseg = steps;
    const int seg_len = (steps + nseg - 1) / nseg * PO_STEP;
    nseg = (I + seg_len - 1) / seg_len;
    const size_t lds = (size_t)(ld / 32) * PO_RT * 64 * 16;
    const bool shadow = gen->wp1t_bf16 != nullptr && cfg->h_enc <= ST_KP;
    clear_errors();
#define LTG_POST_SC(SV, SH)                                                                                                           \
    hipLaunchKernelGGL((k_post_scores<SV, SH>), dim3(rb, nseg), dim3(PO_NT), lds, (hipStream_t)stream, M, I, cfg->h_enc, ld, seg_len, image, \
                       gen->wp1t_bf16, gen->p[3], gen->p[7], beta, score_out, spread_out)
#define LTG_POST_SC_S(SV)                                            \
    do {                                                             \
        if (shadow) LTG_POST_SC(SV, true); else LTG_POST_SC(SV, false); \
    } while (0)
    switch (n_samples) {
        case 1: LTG_POST_SC_S(1); break;
        case 4: LTG_POST_SC_S(4); break;
        case 8: LTG_POST_SC_S(8); break;
        case 16: LTG_POST_SC_S(16); break;
        default: LTG_POST_SC_S(32); break;
    }
#undef LTG_POST_SC_S
#undef LTG_POST_SC
    return check_launch();
}

int ltg_posterior_entries(const ltg_config* cfg, const ltg_gen_state* gen, const uint16_t* image, int32_t n_rows, int32_t n_samples,
                          const int32_t* id_in, int32_t k, float* mean_out, float* std_out, ltg_stream stream) {
    if (!post_args_ok(cfg, gen, image, n_rows, n_samples) || !id_in || !mean_out || !std_out || k < 1 || k > 1024) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const int64_t n_ent = (int64_t)n_rows * k;
    if (n_ent >= (int64_t)1 << 31) return LTG_EINVAL;
    const bool shadow = gen->wp1t_bf16 != nullptr && cfg->h_enc <= ST_KP;
    clear_errors();
    hipLaunchKernelGGL(shadow ? k_post_entries<true> : k_post_entries<false>, dim3((unsigned)((n_ent + PO_NT / 64 - 1) / (PO_NT / 64))), dim3(PO_NT),
                       0, (hipStream_t)stream, (int)n_ent, k, n_samples, cfg->n_items, cfg->h_enc, ltg_posterior_ld(cfg), cfg->item_lo, image,
                       gen->wp1t_bf16, gen->p[3], gen->p[7], id_in, mean_out, std_out);
    return check_launch();
}

int ltg_row_lse(const ltg_config* cfg, const float* logits, int32_t n_rows, float* lse_out, ltg_stream stream) {
    if (!cfg_ok(cfg) || !logits || !lse_out || n_rows < 0) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    hipLaunchKernelGGL(k_row_lse, dim3(n_rows), dim3(NT), 0, (hipStream_t)stream, cfg->n_items, logits, lse_out);
    return check_launch();
}

// Replay of an exploration log.  The temperatures are a HOST array: they travel as kernel arguments.
static_assert(RP_MAXG == LT_MAXG, "the replay groups are the report's");
static bool replay_temps_ok(int32_t n_pol, const float* inv_temp, rp_temps* out) {
    if (n_pol < 1 || n_pol > RP_MAXP || !inv_temp) return false;
    for (int p = 0; p < RP_MAXP; ++p) out->v[p] = 1.f;
    for (int p = 0; p < n_pol; ++p) {
        if (!std::isfinite(inv_temp[p]) || !(inv_temp[p] > 0.f)) return false;
        out->v[p] = inv_temp[p];
    }
    return true;
}

int ltg_list_mass(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, const int32_t* id_in, int32_t f_in,
                  const int32_t* excl_id, int32_t n_pol, const float* inv_temp, float* score_out, int32_t* state_out, float* max_out,
                  float* rest_out, ltg_stream stream) {
    size_t bits, cap;
    rp_temps it;
    if (!id_in || !score_out || !state_out || !max_out || !rest_out || !replay_temps_ok(n_pol, inv_temp, &it) ||
        !explore_args_ok(cfg, logits, tr, n_rows, k, it.v[0], excl_id, f_in, &bits, &cap) || f_in >= k)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    const bool vec = (cfg->n_items % 4) == 0 && ((uintptr_t)logits % 16) == 0;
    auto kern = n_pol == 1 ? (vec ? k_list_mass<true, 1> : k_list_mass<false, 1>)
                           : n_pol <= 4 ? (vec ? k_list_mass<true, 4> : k_list_mass<false, 4>) : (vec ? k_list_mass<true, 8> : k_list_mass<false, 8>);
    hipLaunchKernelGGL(kern, dim3(n_rows), dim3(TK_NT), bits, (hipStream_t)stream, cfg->n_items, cfg->item_lo, logits,
                       tr ? tr->indptr : (const int32_t*)nullptr, tr ? tr->indices : (const int32_t*)nullptr, n_rows, k, id_in, f_in, excl_id, n_pol,
                       it, score_out, state_out, max_out, rest_out);
    return check_launch();
}

int ltg_replay_rows(int32_t n_rows, int32_t k, int32_t n_pol, const float* inv_temp, int32_t f_in, const int32_t* head_id, const int32_t* id_in,
                    const float* logp0, const float* reward, const float* score, const int32_t* state, const float* M, const float* rest,
                    const uint8_t* item_group, int32_t n_groups, int32_t n_items_global, double clip, double* row_out, double* w_out,
                    int32_t* first_bad_out, float* logp1_out, ltg_stream stream) {
    rp_temps it;
    if (!id_in || !logp0 || !reward || !score || !state || !M || !rest || !item_group || !row_out || !w_out || !first_bad_out || n_rows < 0 ||
        k < 1 || k > 1024 || !replay_temps_ok(n_pol, inv_temp, &it) || f_in < 0 || f_in >= k || (f_in > 0 && !head_id) || !std::isfinite(clip) ||
        !(clip > 0.0) || n_groups < 1 || n_groups > RP_MAXG || n_items_global <= 0)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    hipLaunchKernelGGL(k_replay_rows, dim3((n_rows + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, (hipStream_t)stream, n_rows, k, n_pol, it, f_in, head_id,
                       id_in, logp0, reward, score, state, M, rest, item_group, n_groups, n_items_global, std::log(clip), row_out, w_out,
                       first_bad_out, logp1_out);
    return check_launch();
}

int ltg_topk_quota(int32_t n_rows, int32_t k_in, const float* score_all, const int32_t* id_all, int32_t n_lists, int32_t m_in,
                   const float* score_grp, const int32_t* id_grp, const int32_t* quota, int32_t k, float* score_out, int32_t* id_out,
                   ltg_stream stream) {
    if (!score_all || !id_all || !score_grp || !id_grp || !quota || !score_out || !id_out || n_rows < 0 || n_lists < 1 || n_lists > 8 ||
        m_in < 1 || m_in > 1024 || k < 1 || k > k_in || k_in > 1024)
        return LTG_EINVAL;
    tk_quota q = {};
    int64_t sum = 0;
    for (int j = 0; j < n_lists; ++j) {
        if (quota[j] < 0 || quota[j] > m_in) return LTG_EINVAL;
        q.q[j] = quota[j];
        sum += quota[j];
    }
    if (sum > k) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    hipLaunchKernelGGL(k_topk_quota, dim3(n_rows), dim3((k_in + 63) / 64 * 64), 0, (hipStream_t)stream, n_rows, k_in, score_all, id_all, n_lists, m_in,
                       score_grp, id_grp, q, k, score_out, id_out);
    return check_launch();
}

int ltg_topk_metrics(const int32_t* id_in, int32_t n_rows, int32_t k_in, const ltg_batch* te, const uint8_t* item_group,
                     int32_t n_items_global, int32_t n_groups, int32_t k_ndcg, int32_t k_r1, int32_t k_r2, int32_t k_exp, float* out,
                     int32_t* item_hits, ltg_stream stream) {
    if (!id_in || !te || !item_group || !out || n_rows < 0 || k_in < 1 || k_in > 1024 || n_groups < 1 || n_groups > LT_MAXG ||
        n_items_global <= 0 || te->n_rows != n_rows)
        return LTG_EINVAL;
    for (const int32_t k : {k_ndcg, k_r1, k_r2, k_exp})
        if (k < 1 || k > k_in) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    if (!te->indptr || !te->indices) return LTG_EINVAL;
    clear_errors();
    hipLaunchKernelGGL(k_topk_metrics, dim3(n_rows), dim3(NT), 0, (hipStream_t)stream, k_in, id_in, te->indptr, te->indices, item_group,
                       n_items_global, n_groups, k_ndcg, k_r1, k_r2, k_exp, out, item_hits);
    return check_launch();
}

// Item-to-item neighbours.  The segmentation is a function of (n_items, n_q, k) alone, so ltg_item_neighbors_ws_bytes and the
// call agree: enough (query block x segment) workgroups for two per CU, a segment at least 1 024 items, at most 64 segments.
static int nbr_plan(int I, int n_q, int k, int* seg_len) {
    const int rows = k <= 128 ? 32 : 16;
    const int nqb = (n_q + rows - 1) / rows;
    int want = (512 + nqb - 1) / nqb;
    const int most = (I + 1023) / 1024 < 64 ? (I + 1023) / 1024 : 64;
    want = want > most ? most : want;
    const int len = ((I + want - 1) / want + NB_STEP - 1) / NB_STEP * NB_STEP;
    *seg_len = len;
    return (I + len - 1) / len;
}
static bool nbr_cfg_ok(const ltg_config* cfg) {
    return cfg && cfg->n_items > 0 && cfg->h_enc >= 1 && cfg->h_enc <= ST_KP && cfg->item_lo >= 0 &&
           (int64_t)cfg->item_lo + cfg->n_items <= (int64_t)(cfg->n_items_global ? cfg->n_items_global : cfg->n_items) &&
           (size_t)cfg->n_items * (size_t)(ST_KP * 2) < ((size_t)1 << 32);
}

int ltg_item_pack(const ltg_config* cfg, const ltg_gen_state* gen, int32_t space, int32_t metric, uint16_t* image_out, ltg_stream stream) {
    if (!cfg || !gen || !image_out || cfg->n_items <= 0 || cfg->h_enc < 1 || cfg->h_enc > ST_KP ||
        (space != LTG_SPACE_DECODER && space != LTG_SPACE_ENCODER) || (metric != LTG_METRIC_COSINE && metric != LTG_METRIC_DOT))
        return LTG_EINVAL;
    const float* W = gen->p[space == LTG_SPACE_DECODER ? 3 : 0];
    if (!W) return LTG_EINVAL;
    clear_errors();
    const int gx = (cfg->n_items + NT / 64 - 1) / (NT / 64);
    auto kern = metric == LTG_METRIC_COSINE ? k_item_pack<true> : k_item_pack<false>;
    hipLaunchKernelGGL(kern, dim3(gx < 65536 ? gx : 65536), dim3(NT), 0, (hipStream_t)stream, cfg->n_items, cfg->h_enc, W, image_out);
    return check_launch();
}

size_t ltg_item_neighbors_ws_bytes(const ltg_config* cfg, int32_t n_q, int32_t k) {
    if (!nbr_cfg_ok(cfg) || n_q <= 0 || k < 1 || k > LTG_NBR_MAX_K) return 0;
    int seg_len;
    const int nseg = nbr_plan(cfg->n_items, n_q, k, &seg_len);
    return align_up((size_t)nseg * (size_t)n_q * (size_t)k * (sizeof(float) + sizeof(int32_t)));
}

int ltg_item_neighbors(const ltg_config* cfg, const uint16_t* table_image, const uint16_t* q_image, const int32_t* q_gid,
                       int32_t n_q, const uint8_t* item_group, uint32_t group_mask, int32_t k, float* score_out, int32_t* id_out,
                       void* workspace, size_t ws_bytes, ltg_stream stream) {
    if (!nbr_cfg_ok(cfg) || !table_image || !q_image || !q_gid || !score_out || !id_out || n_q < 0 || k < 1 || k > LTG_NBR_MAX_K)
        return LTG_EINVAL;
    if (item_group && (group_mask == 0u || group_mask > 0x1FFu)) return LTG_EINVAL;
    if (n_q == 0) return LTG_OK;
    if (!workspace) return LTG_EINVAL;
    if (ws_bytes < ltg_item_neighbors_ws_bytes(cfg, n_q, k)) return LTG_EWORKSPACE;
    int seg_len;
    const int nseg = nbr_plan(cfg->n_items, n_q, k, &seg_len);
    float* ws_score = (float*)workspace;
    int32_t* ws_id = (int32_t*)(ws_score + (size_t)nseg * n_q * k);
    const uint8_t* labels = item_group ? item_group + cfg->item_lo : nullptr;
    clear_errors();
#define LTG_NBR(NTB, GRP)                                                                                                                  \
    hipLaunchKernelGGL((k_item_neighbors<NTB, GRP>), dim3((n_q + 16 * NTB - 1) / (16 * NTB), nseg), dim3(NB_NT),                             \
                       (size_t)ST_KS * NTB * 64 * 16 + (size_t)NB_ENT * 8, (hipStream_t)stream, cfg->n_items, cfg->item_lo, n_q, seg_len, k, \
                       table_image, q_image, q_gid, labels, group_mask, ws_score, ws_id)
    if (k <= 128) { if (labels) LTG_NBR(2, true); else LTG_NBR(2, false); }
    else { if (labels) LTG_NBR(1, true); else LTG_NBR(1, false); }
#undef LTG_NBR
    if (hipGetLastError() != hipSuccess) return LTG_ELAUNCH;
    hipLaunchKernelGGL(k_topk_merge, dim3(n_q), dim3(NT), 0, (hipStream_t)stream, nseg, n_q, k, ws_score, ws_id, k, score_out, id_out);
    return check_launch();
}

// Niche companions.  The segmentation is a function of (n_q, n_c, k) alone, so ltg_pair_companions_ws_bytes and the call agree:
// enough (query block x segment) workgroups for two per CU (one is resident at a time), a segment at least 1 024 candidates and a multiple
// of the 64-candidate step, at most 64 segments; never fewer than one, so that n_c = 0 has a workspace size too.
static int pair_plan(int n_q, int n_c, int k, int* seg_len) {
    const int rows = k <= 128 ? 32 : 16;
    const int nqb = (n_q + rows - 1) / rows;
    int want = (512 + nqb - 1) / nqb;
    const int kib = (n_c + 1023) / 1024;
    const int most = kib < 1 ? 1 : kib < 64 ? kib : 64;
    want = want > most ? most : want;
    int len = ((n_c + want - 1) / want + PC_CT - 1) / PC_CT * PC_CT;
    len = len < PC_CT ? PC_CT : len;
    *seg_len = len;
    const int nseg = (n_c + len - 1) / len;
    return nseg < 1 ? 1 : nseg;
}
static bool pair_cfg_ok(const ltg_config* cfg) {
    return cfg && cfg->d_feat >= 1 && cfg->d_h0 >= 1 && cfg->d_h1 >= 1 && cfg->d_h2 >= 1 && cfg->d_h3 >= 1 && cfg->d_h3 <= PC_MAX_H3 &&
           (int64_t)cfg->d_h0 + (cfg->d_h1 > cfg->d_h2 ? cfg->d_h1 : cfg->d_h2) <= PK_MAX_H;
}

int32_t ltg_pair_ld(const ltg_config* cfg) { return pair_cfg_ok(cfg) ? (cfg->d_h3 + 3) / 4 * 4 : 0; }

int ltg_pair_pack(const ltg_config* cfg, const ltg_disc_state* disc, int32_t side, const int32_t* ids, int32_t n, float* image_out,
                  ltg_stream stream) {
    if (!pair_cfg_ok(cfg) || !disc || !ids || !image_out || n < 0 || (side != LTG_PAIR_POP && side != LTG_PAIR_NICHE)) return LTG_EINVAL;
    const bool niche = side == LTG_PAIR_NICHE;
    const float *wb = disc->p[niche ? 2 : 0], *bb = disc->p[niche ? 3 : 1], *w3 = disc->p[4], *b3 = disc->p[5];
    if (!disc->emb || !disc->p[0] || !disc->p[1] || !disc->p[2] || !disc->p[3] || !w3 || !b3) return LTG_EINVAL;
    if (n == 0) return LTG_OK;
    const int hb = niche ? cfg->d_h2 : cfg->d_h1;
    clear_errors();
    hipLaunchKernelGGL(k_pair_pack, dim3((n + PK_IDS - 1) / PK_IDS), dim3(NT), (size_t)PK_IDS * (cfg->d_h0 + hb) * sizeof(float), (hipStream_t)stream, n,
                       cfg->d_h0, hb, cfg->d_h3, ltg_pair_ld(cfg), disc->emb, wb, bb, niche ? w3 + (size_t)cfg->d_h1 * cfg->d_h3 : w3,
                       niche ? b3 : (const float*)nullptr, ids, image_out);
    return check_launch();
}

size_t ltg_pair_companions_ws_bytes(const ltg_config* cfg, int32_t n_q, int32_t n_c, int32_t k) {
    if (!pair_cfg_ok(cfg) || n_q <= 0 || n_c < 0 || k < 1 || k > LTG_PAIR_MAX_K) return 0;
    int seg_len;
    const int nseg = pair_plan(n_q, n_c, k, &seg_len);
    return align_up((size_t)nseg * (size_t)n_q * (size_t)k * (sizeof(float) + sizeof(int32_t)));
}

int ltg_pair_companions(const ltg_config* cfg, const ltg_disc_state* disc, const float* q_image, const int32_t* q_gid, int32_t n_q,
                        const float* c_image, const int32_t* c_gid, int32_t n_c, int32_t k, float* score_out, int32_t* id_out, void* ws,
                        size_t ws_bytes, ltg_stream stream) {
    if (!pair_cfg_ok(cfg) || n_q < 0 || n_c < 0 || k < 1 || k > LTG_PAIR_MAX_K) return LTG_EINVAL;
    if (n_q == 0) return LTG_OK;
    if (!disc || !disc->p[6] || !disc->p[7] || !q_image || !q_gid || !score_out || !id_out || !ws || (n_c > 0 && (!c_image || !c_gid)))
        return LTG_EINVAL;
    if (ws_bytes < ltg_pair_companions_ws_bytes(cfg, n_q, n_c, k)) return LTG_EWORKSPACE;
    clear_errors();
    if (n_c == 0) {
        const size_t n = (size_t)n_q * k;
        const size_t gx = (n + NT - 1) / NT;
        hipLaunchKernelGGL(k_pair_fill, dim3((unsigned)(gx < 4096 ? gx : 4096)), dim3(NT), 0, (hipStream_t)stream, n, score_out, id_out);
        return check_launch();
    }
    int seg_len;
    const int nseg = pair_plan(n_q, n_c, k, &seg_len);
    float* ws_score = (float*)ws;
    int32_t* ws_id = (int32_t*)(ws_score + (size_t)nseg * n_q * k);
    const int ld = ltg_pair_ld(cfg);
    const size_t lds = (size_t)PC_ENT * 8 + (size_t)PC_CT * (ld | 1) * sizeof(float);
#define LTG_PAIR(R)                                                                                                                          \
    hipLaunchKernelGGL((k_pair_companions<R>), dim3((n_q + 8 * R - 1) / (8 * R), nseg), dim3(PC_NT), lds, (hipStream_t)stream, n_q, n_c, seg_len, k, \
                       cfg->d_h3, ld, q_image, q_gid, c_image, c_gid, disc->p[6], disc->p[7], ws_score, ws_id)
    if (k <= 128) LTG_PAIR(4); else LTG_PAIR(2);
#undef LTG_PAIR
    if (hipGetLastError() != hipSuccess) return LTG_ELAUNCH;
    hipLaunchKernelGGL(k_topk_merge, dim3(n_q), dim3(NT), 0, (hipStream_t)stream, nseg, n_q, k, ws_score, ws_id, k, score_out, id_out);
    return check_launch();
}

// Item audiences.  The segmentation is a function of (n_rows, n_q, k) alone, so ltg_item_audience_ws_bytes and the call agree:
// enough (column block x row segment) workgroups for four per CU, a segment at least 1 024 rows, at most 32 segments (the merge of a
// column's segment lists stays short).  One segment needs no workspace: the kernel writes the outputs itself.
static int aud_blocks(int n_q, int k) {
    const int cols = k <= 128 ? 16 : 8;
    return (int)(((int64_t)n_q + cols - 1) / cols);
}
static int aud_plan(int n_rows, int n_q, int k, int* seg_len) {
    const int nqb = aud_blocks(n_q, k);
    int64_t want = (1024 + (int64_t)nqb - 1) / nqb;
    const int64_t most = ((int64_t)n_rows + 1023) / 1024 < 32 ? ((int64_t)n_rows + 1023) / 1024 : 32;
    want = want > most ? most : want;
    const int64_t len = (((int64_t)n_rows + want - 1) / want + AU_ROWS - 1) / AU_ROWS * AU_ROWS;
    *seg_len = (int)(len < 0x7FFFFF80 ? len : 0x7FFFFF80);
    return (int)(((int64_t)n_rows + *seg_len - 1) / *seg_len);
}
static bool aud_args_ok(const ltg_config* cfg, int32_t n_rows, int32_t n_q, int32_t k) {
    return cfg && cfg->n_items > 0 && n_rows >= 0 && n_q >= 0 && k >= 1 && k <= LTG_AUD_MAX_K;
}

size_t ltg_item_audience_ws_bytes(const ltg_config* cfg, int32_t n_rows, int32_t n_q, int32_t k) {
    if (!aud_args_ok(cfg, n_rows, n_q, k) || n_rows == 0 || n_q == 0) return 0;
    int seg_len;
    const int nseg = aud_plan(n_rows, n_q, k, &seg_len);
    return nseg > 1 ? align_up((size_t)nseg * (size_t)n_q * (size_t)k * (sizeof(float) + sizeof(int32_t))) : 0;
}

int ltg_item_audience(const ltg_config* cfg, const float* logits, const float* lse, const ltg_batch* tr, int32_t n_rows, int32_t row_lo,
                      const int32_t* q_col, int32_t n_q, int32_t k, float* score_out, int32_t* id_out, void* ws, size_t ws_bytes,
                      ltg_stream stream) {
    if (!aud_args_ok(cfg, n_rows, n_q, k) || !logits || !q_col || !score_out || !id_out || row_lo < 0 ||
        (int64_t)row_lo + (int64_t)n_rows > (int64_t)INT32_MAX)
        return LTG_EINVAL;
    if (tr && (!tr->indptr || !tr->indices || tr->n_rows != n_rows)) return LTG_EINVAL;
    const size_t need = ltg_item_audience_ws_bytes(cfg, n_rows, n_q, k);
    if (need > 0 && (!ws || ws_bytes < need)) return LTG_EINVAL;
    if (n_rows == 0 || n_q == 0) return LTG_OK;
    int seg_len;
    const int nseg = aud_plan(n_rows, n_q, k, &seg_len);
    float* list_s = nseg > 1 ? (float*)ws : score_out;
    int32_t* list_i = nseg > 1 ? (int32_t*)((float*)ws + (size_t)nseg * n_q * k) : id_out;
    clear_errors();
#define LTG_AUD(COLS, CAP)                                                                                                              \
    hipLaunchKernelGGL((k_item_audience<COLS, CAP>), dim3(aud_blocks(n_q, k), nseg), dim3(AU_NT), (size_t)COLS * CAP * 8,                     \
                       (hipStream_t)stream, cfg->n_items, n_rows, row_lo, n_q, seg_len, k, logits, lse,                                   \
                       tr ? tr->indptr : (const int32_t*)nullptr, tr ? tr->indices : (const int32_t*)nullptr, q_col, list_s, list_i)
    if (k <= 128) LTG_AUD(16, 256); else LTG_AUD(8, 512);
#undef LTG_AUD
    if (nseg == 1) return check_launch();
    if (hipGetLastError() != hipSuccess) return LTG_ELAUNCH;
    hipLaunchKernelGGL(k_topk_merge, dim3(n_q), dim3(NT), 0, (hipStream_t)stream, nseg, n_q, k, list_s, list_i, k, score_out, id_out);
    return check_launch();
}

// Exposure-capped top-K lists.  The workspace holds the thresholds, the per-item index (offsets, cursors, entry numbers), one
// active byte per candidate entry and one int32 per row; its layout is a function of (n_rows, c_in, n_items_global) alone.  Every refusal
// comes before the first HIP call.
// a workspace handed out piece by piece: take(bytes) -> the next aligned piece of `base`; on the null base of a size query nullptr, without
// arithmetic on it; `o` ends as the bytes the pieces need
struct Carve {
    char* base;
    size_t o = 0;
    char* take(size_t bytes) {
        char* p = base ? base + o : nullptr;
        o += align_up(bytes);
        return p;
    }
};
struct CapWs {
    uint64_t* thr;
    int32_t *off, *cur, *seg, *row_over;
    uint8_t* active;
    size_t bytes;
};
static bool cap_args_ok(int32_t n_rows, int32_t c_in, int32_t n_items_global) {
    return n_rows >= 0 && c_in >= 1 && c_in <= 1024 && n_items_global >= 1 && (int64_t)n_rows * (int64_t)c_in < ((int64_t)1 << 31);
}
static CapWs cap_carve(int32_t n_rows, int32_t c_in, int32_t n_items_global, char* base) {
    const size_t I = (size_t)n_items_global, E = (size_t)n_rows * (size_t)c_in;
    CapWs w;
    Carve ws{base};
    w.thr = (uint64_t*)ws.take(I * sizeof(uint64_t));
    w.off = (int32_t*)ws.take((I + 1) * sizeof(int32_t));
    w.cur = (int32_t*)ws.take(I * sizeof(int32_t));
    w.seg = (int32_t*)ws.take((E > 0 ? E : 1) * sizeof(int32_t));
    w.row_over = (int32_t*)ws.take(((size_t)n_rows > 0 ? (size_t)n_rows : 1) * sizeof(int32_t));
    w.active = (uint8_t*)ws.take(E > 0 ? E : 1);
    w.bytes = ws.o;
    return w;
}

// the per-item index of the candidates, a CSR over entry numbers (ltg_cap.h): zero, count, scan, scatter; words (the cap's thresholds, the
// floor's selection words) <- 0 and the state block <- 0 on the way
static void cap_enqueue_index(int32_t n_rows, int32_t c_in, const int32_t* cand_id, int32_t I, int32_t* state, int32_t* cur, int32_t* off,
                              int32_t* seg, uint64_t* words, hipStream_t st) {
    const int row_blocks = (n_rows + CP_NT / 64 - 1) / (CP_NT / 64);
    hipLaunchKernelGGL(k_cap_zero, dim3((I + CP_NT - 1) / CP_NT), dim3(CP_NT), 0, st, I, cur, state);
    hipLaunchKernelGGL(k_cap_count<false>, dim3(row_blocks), dim3(CP_NT), 0, st, n_rows, c_in, cand_id, I, cur, (const int32_t*)off, seg);
    hipLaunchKernelGGL(k_cap_scan, dim3(1), dim3(1024), 0, st, I, cur, off, words);
    hipLaunchKernelGGL(k_cap_count<true>, dim3(row_blocks), dim3(CP_NT), 0, st, n_rows, c_in, cand_id, I, cur, (const int32_t*)off, seg);
}

size_t ltg_cap_ws_bytes(int32_t n_rows, int32_t c_in, int32_t n_items_global) {
    return cap_args_ok(n_rows, c_in, n_items_global) ? cap_carve(n_rows, c_in, n_items_global, nullptr).bytes : 0;
}

int ltg_cap_index(int32_t n_rows, int32_t c_in, const int32_t* cand_id, int32_t n_items_global, int32_t* state, void* ws, size_t ws_bytes,
                  ltg_stream stream) {
    if (!cap_args_ok(n_rows, c_in, n_items_global) || !cand_id || !state || !ws ||
        ws_bytes < cap_carve(n_rows, c_in, n_items_global, nullptr).bytes)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const CapWs w = cap_carve(n_rows, c_in, n_items_global, (char*)ws);
    clear_errors();
    cap_enqueue_index(n_rows, c_in, cand_id, n_items_global, state, w.cur, w.off, w.seg, w.thr, (hipStream_t)stream);
    return check_launch();
}

int ltg_cap_rounds(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse, const int32_t* cap,
                   int32_t n_items_global, int32_t k, int32_t n_rounds, int32_t* state, void* ws, size_t ws_bytes, ltg_stream stream) {
    if (!cap_args_ok(n_rows, c_in, n_items_global) || !cand_score || !cand_id || !cap || !state || !ws || k < 1 || k > c_in || n_rounds < 1 ||
        n_rounds > LTG_CAP_MAX_ROUNDS || ws_bytes < cap_carve(n_rows, c_in, n_items_global, nullptr).bytes)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const CapWs w = cap_carve(n_rows, c_in, n_items_global, (char*)ws);
    const hipStream_t st = (hipStream_t)stream;
    const int row_blocks = (n_rows + CP_NT / 64 - 1) / (CP_NT / 64);
    clear_errors();
    for (int r = 0; r < n_rounds; ++r) {
        hipLaunchKernelGGL(k_cap_propose, dim3(row_blocks), dim3(CP_NT), 0, st, n_rows, c_in, k, cand_score, cand_id, lse, cap, n_items_global,
                           (const uint64_t*)w.thr, w.active, state);
        hipLaunchKernelGGL(k_cap_accept, dim3(n_items_global), dim3(CP_NT), 0, st, c_in, cand_score, lse, cap, (const int32_t*)w.off,
                           (const int32_t*)w.seg, (const uint8_t*)w.active, w.thr, state);
    }
    return check_launch();
}

int ltg_cap_finish(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, int32_t n_items_global, int32_t k,
                   float* score_out, int32_t* id_out, int32_t* state, void* ws, size_t ws_bytes, ltg_stream stream) {
    if (!cap_args_ok(n_rows, c_in, n_items_global) || !cand_score || !cand_id || !score_out || !id_out || !state || !ws || k < 1 || k > c_in ||
        ws_bytes < cap_carve(n_rows, c_in, n_items_global, nullptr).bytes)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const CapWs w = cap_carve(n_rows, c_in, n_items_global, (char*)ws);
    const hipStream_t st = (hipStream_t)stream;
    clear_errors();
    hipLaunchKernelGGL(k_cap_finish, dim3((n_rows + CP_NT / 64 - 1) / (CP_NT / 64)), dim3(CP_NT), 0, st, n_rows, c_in, k, cand_score, cand_id,
                       n_items_global, (const uint8_t*)w.active, score_out, id_out, w.row_over);
    hipLaunchKernelGGL(k_cap_stats, dim3(1), dim3(1024), 0, st, n_rows, k, (const int32_t*)id_out, (const int32_t*)w.row_over, state);
    return check_launch();
}

// Share-targeted top-K lists.  The workspace holds one 64-bit word per (row, step), two int32 per row, the 8 x 256 bins of the
// radix select and its selection block; its layout is a function of (n_rows, k) alone.  One call enqueues everything -- 2 + 2 x 8 + 1
// launches, no read-back in between -- and every refusal comes before the first HIP call.
struct ShareWs {
    uint64_t* words;
    int32_t *row_a, *row_kk, *bins;
    sh_sel* sel;
    size_t bytes;
};
static bool share_args_ok(int32_t n_rows, int32_t k) {
    return n_rows >= 0 && k >= 1 && k <= 1024 && (int64_t)n_rows * (int64_t)k < ((int64_t)1 << 31);
}
static ShareWs share_carve(int32_t n_rows, int32_t k, char* base) {
    const size_t R = (size_t)n_rows > 0 ? (size_t)n_rows : 1, E = R * (size_t)k;
    ShareWs w;
    Carve ws{base};
    w.words = (uint64_t*)ws.take(E * sizeof(uint64_t));
    w.row_a = (int32_t*)ws.take(R * sizeof(int32_t));
    w.row_kk = (int32_t*)ws.take(R * sizeof(int32_t));
    w.bins = (int32_t*)ws.take((size_t)SH_PASSES * 256 * sizeof(int32_t));
    w.sel = (sh_sel*)ws.take(sizeof(sh_sel));
    w.bytes = ws.o;
    return w;
}
// [p, p + n) and [q, q + m) (bytes) share a byte, or start at the same address
static bool share_overlap(const void* p, size_t n, const void* q, size_t m) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a == b || (a < b + m && b < a + n);
}

size_t ltg_share_ws_bytes(int32_t n_rows, int32_t k) { return share_args_ok(n_rows, k) ? share_carve(n_rows, k, nullptr).bytes : 0; }

int ltg_topk_share(int32_t n_rows, int32_t m_in, const float* score_pro, const int32_t* id_pro, const float* score_rest, const int32_t* id_rest,
                   int32_t k, int64_t want, float* score_out, int32_t* id_out, int32_t* state, void* ws, size_t ws_bytes, ltg_stream stream) {
    if (!score_pro || !id_pro || !score_rest || !id_rest || !score_out || !id_out || !state || !ws || m_in < 1 || m_in > 1024 || k < 1 ||
        k > m_in || !share_args_ok(n_rows, k) || want < 0 || ws_bytes < share_carve(n_rows, k, nullptr).bytes)
        return LTG_EINVAL;
    const size_t in_b = (size_t)n_rows * (size_t)m_in * 4, out_b = (size_t)n_rows * (size_t)k * 4;
    const void* ins[4] = {score_pro, id_pro, score_rest, id_rest};
    for (const void* in : ins)
        if (share_overlap(score_out, out_b, in, in_b) || share_overlap(id_out, out_b, in, in_b)) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const ShareWs w = share_carve(n_rows, k, (char*)ws);
    const hipStream_t st = (hipStream_t)stream;
    const int row_blocks = (n_rows + SH_NT / 64 - 1) / (SH_NT / 64);
    const size_t n_words = (size_t)n_rows * (size_t)k, per = (size_t)SH_NT * SH_HIST_PER;
    const int hist_blocks = (int)((n_words + per - 1) / per < 2048 ? (n_words + per - 1) / per : 2048);
    clear_errors();
    hipLaunchKernelGGL(k_share_zero, dim3(1), dim3(SH_NT), 0, st, state, w.bins, w.sel);
    hipLaunchKernelGGL(k_share_steps, dim3(row_blocks), dim3(SH_NT), 0, st, n_rows, m_in, k, score_pro, id_pro, score_rest, id_rest, w.words,
                       w.row_a, w.row_kk, state);
    for (int pass = 0; pass < SH_PASSES; ++pass) {
        hipLaunchKernelGGL(k_share_hist, dim3(hist_blocks), dim3(SH_NT), 0, st, n_words, pass, (int64_t)want, (const uint64_t*)w.words,
                           (const int32_t*)state, (const sh_sel*)w.sel, w.bins);
        hipLaunchKernelGGL(k_share_pick, dim3(1), dim3(256), 0, st, pass, (int64_t)want, state, w.sel, (const int32_t*)w.bins);
    }
    hipLaunchKernelGGL(k_share_finish, dim3(row_blocks), dim3(SH_NT), 0, st, n_rows, m_in, k, (int64_t)want, score_pro, id_pro, score_rest,
                       id_rest, (const uint64_t*)w.words, (const int32_t*)w.row_a, (const int32_t*)w.row_kk, (const sh_sel*)w.sel, score_out,
                       id_out, state);
    return check_launch();
}

// Exposure-floor top-K lists.  The workspace holds the selection words, the per-item index (offsets, cursors, entry numbers),
// the limits and one int32 per row, and the held counts; its layout is a function of (n_rows, c_in, n_items_global) alone.  Every refusal
// comes before the first HIP call.
static_assert(FL_STATE == LTG_FLOOR_STATE && CP_STATE == LTG_FLOOR_STATE, "the index zeroes the floor's state block with the cap's kernel");
struct FloorWs {
    uint64_t* sel;
    int32_t *off, *cur, *seg, *lim, *row_t, *held;
    size_t bytes;
};
static FloorWs floor_carve(int32_t n_rows, int32_t c_in, int32_t n_items_global, char* base) {
    const size_t I = (size_t)n_items_global, E = (size_t)n_rows * (size_t)c_in, N = (size_t)n_rows > 0 ? (size_t)n_rows : 1;
    FloorWs w;
    Carve ws{base};
    w.sel = (uint64_t*)ws.take(I * sizeof(uint64_t));
    w.off = (int32_t*)ws.take((I + 1) * sizeof(int32_t));
    w.cur = (int32_t*)ws.take(I * sizeof(int32_t));
    w.seg = (int32_t*)ws.take((E > 0 ? E : 1) * sizeof(int32_t));
    w.lim = (int32_t*)ws.take(N * sizeof(int32_t));
    w.row_t = (int32_t*)ws.take(N * sizeof(int32_t));
    w.held = (int32_t*)ws.take(I * sizeof(int32_t));
    w.bytes = ws.o;
    return w;
}
static bool floor_ws_ok(int32_t n_rows, int32_t c_in, int32_t n_items_global, const void* ws, size_t ws_bytes) {
    return cap_args_ok(n_rows, c_in, n_items_global) && ws && ws_bytes >= floor_carve(n_rows, c_in, n_items_global, nullptr).bytes;
}

size_t ltg_floor_ws_bytes(int32_t n_rows, int32_t c_in, int32_t n_items_global) {
    return cap_args_ok(n_rows, c_in, n_items_global) ? floor_carve(n_rows, c_in, n_items_global, nullptr).bytes : 0;
}

int ltg_floor_index(int32_t n_rows, int32_t c_in, const int32_t* cand_id, int32_t n_items_global, int32_t* state, void* ws, size_t ws_bytes,
                    ltg_stream stream) {
    if (!floor_ws_ok(n_rows, c_in, n_items_global, ws, ws_bytes) || !cand_id || !state) return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const FloorWs w = floor_carve(n_rows, c_in, n_items_global, (char*)ws);
    const hipStream_t st = (hipStream_t)stream;
    clear_errors();
    cap_enqueue_index(n_rows, c_in, cand_id, n_items_global, state, w.cur, w.off, w.seg, w.sel, st);
    hipLaunchKernelGGL(k_floor_lim, dim3((n_rows + FL_NT - 1) / FL_NT), dim3(FL_NT), 0, st, n_rows, c_in, w.lim);
    return check_launch();
}

int ltg_floor_rounds(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse, const int32_t* need,
                     int32_t n_items_global, int32_t k, int32_t reserve, int32_t n_rounds, int32_t* state, void* ws, size_t ws_bytes,
                     ltg_stream stream) {
    if (!floor_ws_ok(n_rows, c_in, n_items_global, ws, ws_bytes) || !cand_score || !cand_id || !need || !state || k < 1 || k > c_in ||
        reserve < 0 || reserve > k || n_rounds < 1 || n_rounds > LTG_FLOOR_MAX_ROUNDS)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const FloorWs w = floor_carve(n_rows, c_in, n_items_global, (char*)ws);
    const hipStream_t st = (hipStream_t)stream;
    const int row_blocks = (n_rows + FL_NT / 64 - 1) / (FL_NT / 64);
    clear_errors();
    for (int r = 0; r < n_rounds; ++r) {
        hipLaunchKernelGGL(k_floor_select, dim3(n_items_global), dim3(FL_NT), 0, st, c_in, k, reserve, cand_score, lse, need,
                           (const int32_t*)w.off, (const int32_t*)w.seg, (const int32_t*)w.lim, w.sel, (int32_t*)nullptr, state, 1);
        hipLaunchKernelGGL(k_floor_users, dim3(row_blocks), dim3(FL_NT), 0, st, n_rows, c_in, k, reserve, cand_score, cand_id, lse, need,
                           n_items_global, (const uint64_t*)w.sel, w.lim, state);
    }
    return check_launch();
}

int ltg_floor_finish(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse, const int32_t* need,
                     int32_t n_items_global, int32_t k, int32_t reserve, float* score_out, int32_t* id_out, uint8_t* active_out,
                     int32_t* held_out, int32_t* state, void* ws, size_t ws_bytes, ltg_stream stream) {
    if (!floor_ws_ok(n_rows, c_in, n_items_global, ws, ws_bytes) || !cand_score || !cand_id || !need || !score_out || !id_out || !state ||
        k < 1 || k > c_in || reserve < 0 || reserve > k)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    const FloorWs w = floor_carve(n_rows, c_in, n_items_global, (char*)ws);
    const hipStream_t st = (hipStream_t)stream;
    clear_errors();
    // the selection words once more, from the limits as they stand (after convergence: the same words), and held <- 0
    hipLaunchKernelGGL(k_floor_select, dim3(n_items_global), dim3(FL_NT), 0, st, c_in, k, reserve, cand_score, lse, need, (const int32_t*)w.off,
                       (const int32_t*)w.seg, (const int32_t*)w.lim, w.sel, w.held, state, 0);
    hipLaunchKernelGGL(k_floor_finish, dim3((n_rows + FL_NT / 64 - 1) / (FL_NT / 64)), dim3(FL_NT), 0, st, n_rows, c_in, k, reserve, cand_score,
                       cand_id, lse, need, n_items_global, (const uint64_t*)w.sel, (const int32_t*)w.lim, score_out, id_out, active_out, w.held,
                       w.row_t);
    hipLaunchKernelGGL(k_floor_stats, dim3(1), dim3(1024), 0, st, n_rows, n_items_global, need, (const int32_t*)w.held,
                       (const int32_t*)w.row_t, held_out, state);
    return check_launch();
}

// Diversified top-K lists: one launch, no workspace.  Every refusal comes before the first HIP call.
int ltg_topk_diversify(const uint16_t* image, int32_t image_lo, int32_t image_rows, int32_t n_rows, int32_t c_in, const float* score_in,
                       const int32_t* id_in, float lambda, int32_t k, float* score_out, int32_t* id_out, float* stat_out, ltg_stream stream) {
    if (!image || !score_in || !id_in || !score_out || !id_out || c_in < 1 || c_in > LTG_DIV_MAX_C || k < 1 || k > c_in ||
        !(lambda >= 0.f && lambda <= 1.f) || image_rows < 1 || image_lo < 0 || n_rows < 0 || ((uintptr_t)image % 16) != 0)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
#define LTG_DIV(CT)                                                                                                                      \
    hipLaunchKernelGGL((k_topk_diversify<CT>), dim3(n_rows), dim3(CT * 16), (size_t)(CT + CT * (CT + 1) / 2) * 1024, (hipStream_t)stream, \
                       image, image_lo, image_rows, c_in, score_in, id_in, lambda, k, score_out, id_out, stat_out)
    if (c_in <= 64) LTG_DIV(4);
    else if (c_in <= 128) LTG_DIV(8);
    else LTG_DIV(16);
#undef LTG_DIV
    return check_launch();
}

// Why a user got a list entry: one launch, no workspace.  Every refusal comes before the first HIP call.
int ltg_topk_explain(const uint16_t* image, int32_t image_lo, int32_t image_rows, const ltg_batch* tr, int32_t hist_lo, int32_t n_rows,
                     int32_t k_in, const int32_t* id_in, int32_t top, int32_t r, float* score_out, int32_t* id_out, ltg_stream stream) {
    if (!image || !tr || !tr->indptr || !tr->indices || !id_in || !score_out || !id_out || n_rows < 0 || tr->n_rows != n_rows || k_in < 1 ||
        k_in > 1024 || top < 1 || top > k_in || top > LTG_WHY_MAX_TOP || r < 1 || r > LTG_WHY_MAX_R || image_rows < 1 || image_lo < 0 ||
        hist_lo < 0 || ((uintptr_t)image % 16) != 0)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
#define LTG_WHY(CT)                                                                                                                        \
    hipLaunchKernelGGL((k_topk_explain<CT>), dim3(n_rows), dim3(EX_NT), (size_t)(CT + EX_HB / 16) * 1024 + (size_t)EX_HB * (CT * 16 + 4) * 4, \
                       (hipStream_t)stream, image, image_lo, image_rows, tr->indptr, tr->indices, hist_lo, k_in, id_in, top, r, score_out, \
                       id_out)
    if (top <= 64) LTG_WHY(4);
    else if (top <= 128) LTG_WHY(8);
    else LTG_WHY(16);
#undef LTG_WHY
    return check_launch();
}

// Calibrated top-K lists: the class histogram of the histories, and the composition of class lists.  One launch each, no
// workspace.  Every refusal comes before the first HIP call.
int ltg_hist_groups(const ltg_batch* tr, int32_t hist_lo, int32_t n_rows, const uint8_t* item_group, int32_t n_items_global, int32_t n_groups,
                    int32_t* count_out, ltg_stream stream) {
    if (!tr || !tr->indptr || !tr->indices || !item_group || !count_out || n_rows < 0 || tr->n_rows != n_rows || hist_lo < 0 ||
        n_items_global < 1 || n_groups < 1 || n_groups > LTG_CAL_MAX_CLASSES - 1)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    hipLaunchKernelGGL(k_hist_groups, dim3((n_rows + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, (hipStream_t)stream, n_rows, tr->indptr, tr->indices,
                       hist_lo, item_group, n_items_global, n_groups, count_out);
    return check_launch();
}

int ltg_topk_calibrate(int32_t n_rows, int32_t n_lists, int32_t m_in, const float* score_grp, const int32_t* id_grp, const int32_t* list_class,
                       int32_t n_groups, const int32_t* hist, float lambda, int32_t k, float* score_out, int32_t* id_out, float* stat_out,
                       ltg_stream stream) {
    if (!score_grp || !id_grp || !list_class || !hist || !score_out || !id_out || n_rows < 0 || n_groups < 1 ||
        n_groups > LTG_CAL_MAX_CLASSES - 1 || n_lists < 1 || n_lists > n_groups + 1 || m_in < 1 || m_in > 1024 || k < 1 || k > m_in ||
        !(lambda >= 0.f && lambda <= 1.f))
        return LTG_EINVAL;
    cal_map map;
    for (int c = 0; c < CAL_C; ++c) map.list_of[c] = -1;
    for (int j = 0; j < n_lists; ++j) {
        if (list_class[j] < 0 || list_class[j] > n_groups || (j > 0 && list_class[j] <= list_class[j - 1])) return LTG_EINVAL;
        map.list_of[list_class[j]] = j;
    }
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    // the lists of a wave's four rows in LDS when they leave room for five workgroups per CU, else the heads come from global memory
    const size_t lds = (size_t)n_lists * CAL_ROWS * m_in * (sizeof(float) + sizeof(int32_t));
    const bool stage = lds <= 32 * 1024;
    hipLaunchKernelGGL(stage ? k_topk_calibrate<true> : k_topk_calibrate<false>, dim3((n_rows + CAL_ROWS - 1) / CAL_ROWS), dim3(64),
                       stage ? lds : 0, (hipStream_t)stream, n_rows, n_lists, m_in, score_grp, id_grp, map, n_groups, hist, lambda, k, score_out,
                       id_out, stat_out);
    return check_launch();
}

// Critic-checked lists: one launch each, no workspace.  Every refusal comes before the first HIP call.
int ltg_pair_critic(const ltg_config* cfg, const ltg_disc_state* disc, const float* pop_image, int32_t n_pop, const float* niche_image,
                    int32_t n_niche, const int32_t* pop_row, const int32_t* niche_row, int32_t n_items_global, const ltg_batch* tr,
                    int32_t hist_lo, int32_t n_rows, int32_t k_in, const int32_t* id_in, int32_t top, int64_t* sum_out, int32_t* cnt_out,
                    float* best_s, int32_t* best_i, ltg_stream stream) {
    if (!pair_cfg_ok(cfg) || !disc || !disc->p[6] || !disc->p[7] || !pop_image || !niche_image || !pop_row || !niche_row || !tr || !tr->indptr ||
        !tr->indices || !id_in || !sum_out || !cnt_out || !best_s || !best_i || n_rows < 0 || tr->n_rows != n_rows || hist_lo < 0 ||
        n_items_global < 1 || n_pop < 0 || n_niche < 0 || k_in < 1 || k_in > 1024 || top < 1 || top > k_in || top > LTG_CRITIC_MAX_TOP)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    const int ld = ltg_pair_ld(cfg);
    hipLaunchKernelGGL(k_pair_critic, dim3(n_rows), dim3(CR_NT), ((size_t)CR_ET * (ld | 1) + (size_t)CR_AB * ld) * sizeof(float), (hipStream_t)stream,
                       cfg->d_h3, ld,
                       pop_image, n_pop, niche_image, n_niche, pop_row, niche_row, n_items_global, tr->indptr, tr->indices, hist_lo, k_in, id_in,
                       top, disc->p[6], disc->p[7], (long long*)sum_out, cnt_out, best_s, best_i);
    return check_launch();
}

int ltg_critic_finish(int32_t n_rows, int32_t k_in, const int32_t* id_in, int32_t top, const int32_t* niche_row, int32_t n_items_global,
                      int32_t n_niche, const int64_t* sum, const int32_t* cnt, float* crit_out, int32_t* scored_out, ltg_stream stream) {
    if (!id_in || !niche_row || !sum || !cnt || !crit_out || !scored_out || n_rows < 0 || n_items_global < 1 || n_niche < 0 || k_in < 1 ||
        k_in > 1024 || top < 1 || top > k_in || top > LTG_CRITIC_MAX_TOP)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    hipLaunchKernelGGL(k_critic_finish, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, k_in, id_in, top, niche_row, n_items_global, n_niche,
                       (const long long*)sum, cnt, crit_out, scored_out);
    return check_launch();
}

int ltg_topk_gate(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* crit, const int32_t* flag,
                  float tau, int32_t k, float* score_out, int32_t* id_out, int32_t* stat_out, ltg_stream stream) {
    if (!cand_score || !cand_id || !crit || !flag || !score_out || !id_out || !stat_out || n_rows < 0 || c_in < 1 || c_in > LTG_GATE_MAX_C ||
        k < 1 || k > c_in || tau != tau)
        return LTG_EINVAL;
    if (n_rows == 0) return LTG_OK;
    clear_errors();
    hipLaunchKernelGGL(k_topk_gate, dim3((n_rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, n_rows, c_in, cand_score, cand_id, crit, flag, tau, k,
                       score_out, id_out, stat_out);
    return check_launch();
}

int ltg_fp8_roundtrip(const float* in, float* out, int32_t n, ltg_stream stream) {
    clear_errors();
    if (!in || !out || n < 0) return LTG_EINVAL;
    if (n == 0) return LTG_OK;
    hipLaunchKernelGGL(k_fp8_roundtrip, dim3((n + NT - 1) / NT < 1024 ? (n + NT - 1) / NT : 1024), dim3(NT), 0, (hipStream_t)stream, n, in, out);
    return check_launch();
}

int ltg_debug_split(const float* in, float* out, int32_t n, ltg_stream stream) {
    clear_errors();
    if (!in || !out || n < 0 || (n % 4) != 0) return LTG_EINVAL;
    if (n == 0) return LTG_OK;
    const int n4 = n / 4;
    hipLaunchKernelGGL(k_debug_split, dim3((n4 + NT - 1) / NT < 1024 ? (n4 + NT - 1) / NT : 1024), dim3(NT), 0, (hipStream_t)stream, n4,
                       reinterpret_cast<const ltg_f32x4*>(in), out);
    return check_launch();
}

int ltg_debug_gemm(int32_t mode, int32_t M, int32_t N, int32_t K, const float* A, const float* B, float* C, ltg_stream stream) {
    clear_errors();
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || mode < 0 || mode > 2) return LTG_EINVAL;
    const dim3 g((N + 31) / 32, (M + 31) / 32);
    if (mode == 0) hipLaunchKernelGGL(k_debug_gemm<0>, g, dim3(NT), 0, (hipStream_t)stream, M, N, K, A, B, C);
    else if (mode == 1) hipLaunchKernelGGL(k_debug_gemm<1>, g, dim3(NT), 0, (hipStream_t)stream, M, N, K, A, B, C);
    else hipLaunchKernelGGL(k_debug_gemm<2>, g, dim3(NT), 0, (hipStream_t)stream, M, N, K, A, B, C);
    return check_launch();
}

int ltg_rank_scores(const ltg_config* cfg, const float* logits, const ltg_batch* tr, const ltg_batch* te, float* score_out,
                    ltg_stream stream) {
    clear_errors();
    if (!cfg || !logits || !tr || !te || !score_out || tr->n_rows != te->n_rows) return LTG_EINVAL;
    if (tr->n_rows == 0) return LTG_OK;
    hipLaunchKernelGGL(k_rank_scores, dim3(tr->n_rows), dim3(NT), 0, (hipStream_t)stream, cfg->n_items, cfg->item_lo, tr->n_rows, logits,
                       tr->indptr, tr->indices, te->indptr, te->indices, score_out);
    return check_launch();
}

int ltg_rank_counts(const ltg_config* cfg, const float* logits, const ltg_batch* tr, const ltg_batch* te, const float* score,
                    int32_t* count_out, ltg_stream stream) {
    clear_errors();
    if (!cfg || !logits || !tr || !te || !score || !count_out || tr->n_rows != te->n_rows) return LTG_EINVAL;
    if (tr->n_rows == 0) return LTG_OK;
    const size_t lds = (size_t)((cfg->n_items + 31) / 32) * sizeof(unsigned);
    if (lds > 64 * 1024) return LTG_EINVAL;
    hipLaunchKernelGGL(k_rank_metrics, dim3(tr->n_rows), dim3(NT), lds, (hipStream_t)stream, cfg->n_items, cfg->item_lo, logits,
                       tr->indptr, tr->indices, te->indptr, te->indices, score, count_out, 0, 0, 0, (float*)nullptr);
    return check_launch();
}

int ltg_rank_finish(const ltg_batch* te, const int32_t* counts, int32_t k_ndcg, int32_t k_r1, int32_t k_r2, float* out,
                    ltg_stream stream) {
    clear_errors();
    if (!te || !counts || !out) return LTG_EINVAL;
    if (te->n_rows == 0) return LTG_OK;
    hipLaunchKernelGGL(k_rank_finish, dim3((te->n_rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, te->n_rows, te->indptr, counts,
                       k_ndcg, k_r1, k_r2, out);
    return check_launch();
}

#ifdef LTG_STAMP
// MEASUREMENT BUILD ONLY: copies the phase stamps of the stamped kernel's last launch (ltg_rgemm.h) to the host
int ltg_debug_stamps(void* dst, int n_words) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(ltg_stamp_buf), (size_t)n_words * 8) == hipSuccess ? 0 : -1;
}
#endif
}  // extern "C"
