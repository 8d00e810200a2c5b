/*
 * ltg.h -- C ABI of the MI355X-native Long-Tail-GAN training path (libltg_hip.so).
 *
 * The reference (ash-shar/Long-Tail-GAN) has no FFI of its own: its execution boundary is the
 * five TensorFlow `sess.run` call sites of Codes/train.py / Codes/test.py.  Each entry point below
 * replaces one of them (cited per function).  Conventions:
 *
 *   - plain C: pointers + sizes, no torch / C++ types; every pointer is a DEVICE pointer unless
 *     the parameter name starts with `host_`;
 *   - the caller owns every buffer (parameters, Adam moments, activations, workspace); the library
 *     allocates nothing, keeps no global state and is asynchronous on the given HIP stream;
 *   - return value: 0 on success, a negative LTG_E* code on error; never throws;
 *   - randomness: every random tensor can be injected through an optional pointer; NULL selects the
 *     on-device counter RNG keyed by (cfg->seed, stream id, rng_step, element index), which the CPU
 *     oracle reproduces bit-for-bit (oracle/ltg_oracle.py rng_*).
 *
 * Layouts in HBM (all row-major, fp32 unless stated):
 *   W_q0  [I][H]      encoder layer 0   (TF shape [I,600],  MultiVAE.py:199)
 *   W_q1  [H][2Z]     encoder layer 1   (TF shape [600,400])
 *   W_p0  [Z][H]      decoder layer 0   (TF shape [200,600])
 *   W_p1t [I][H]      decoder layer 1 stored ITEM-MAJOR (transpose of TF's [600,I], MultiVAE.py:218)
 *   b_q0 [H], b_q1 [2Z], b_p0 [H], b_p1 [I]
 *   discriminator: emb [F][h0] (frozen), w1 [h0][h1], w2 [h0][h2], w3 [h1+h2][h3], w4 [h3], b*.
 */
#ifndef LTG_H
#define LTG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTG_ABI_VERSION 14

#define LTG_OK 0
#define LTG_EINVAL (-1)     /* bad argument (NULL pointer, negative size, unsupported dims) */
#define LTG_EWORKSPACE (-2) /* workspace too small */
#define LTG_ELAUNCH (-3)    /* HIP launch error (hipGetLastError != hipSuccess) */

#define LTG_PREC_BF16 0 /* decoder GEMM operands rounded to bf16, fp32 accumulate (MFMA 16x16x32 bf16) */
#define LTG_PREC_FP32 1 /* exact fp32 MFMA (16x16x4 f32) everywhere */
#define LTG_PREC_FP8 2  /* d_precision only: OCP e4m3 operands, static power-of-two scales, fp32 accumulate (16x16x32 fp8) */

#define LTG_DARITH_FP32 0   /* ltg_config.d_arith: exact fp32 MFMA (16x16x4 f32) */
#define LTG_DARITH_BF16X6 1 /* three-way bf16 split of every fp32 operand, six cross terms on the bf16 matrix pipe: fp32-accurate */
#define LTG_DARITH_BF16X4 2 /* two-way split, four cross terms: 2^-17 per product, opt-in */

typedef void* ltg_stream; /* hipStream_t */

/* Model / optimiser configuration.  Codes/config.ini:2-12, Codes/generator.py:13-18,
 * Codes/train.py:160 (AdamOptimizer defaults beta1=.9 beta2=.999 eps=1e-8). */
typedef struct ltg_config {
    int32_t n_items; /* I */
    int32_t h_enc;   /* H = p_dims[1] = 600 */
    int32_t z_dim;   /* Z = p_dims[0] = 200 */
    int32_t d_feat;  /* FEATURE_LEN: rows of the frozen embedding table */
    int32_t d_h0, d_h1, d_h2, d_h3; /* discriminator layer widths, each >= 1 (else LTG_EINVAL) */
    int32_t precision; /* LTG_PREC_* */
    /* kernel selection knob, 0 = auto; every setting computes the same function (ABI v14: was `reserved0`).  The host layer, bench.py --variant
     * and the parity tests select code paths with these bits; a configuration with any other bit set is refused (LTG_EINVAL):
     *   bit 14  the sparse W_q0 gradient in its column-blocked shape (three times the waves) instead of one wave per row over all columns
     *   bit 17 / 26  the streaming decoder forward: its second form (h2 resident in LDS, per-wave item tiles; default from 65 536 items) from
     *           8 192 items / its first form at every size
     *   bit 18  the generic (round-1, LDS-staged, any size) kernels instead of the latency path of csrc/ltg_fast.h
     *   bit 19  fp8 discriminator: the backward converts its operands on the fly (instead of operand-format storage)
     *   bit 20  the forward-only tower as three launches (fks_d_l1 -> fks_d_l2 -> fk_d_y) instead of the one-kernel tower of csrc/ltg_tower.h
     *   bit 21 / 22  softmax statistics from a second pass over the logits / fp32 instead of bf16 dlogits on the streaming path
     * (The A/B bits of closed experiments -- 0-3, 6, 9-13, 15, 16, 23-25, 27-30 -- are retired; profiles/README.md keeps their measurements.) */
    int32_t tuning;
    /* item shard of this rank: it owns global items [item_lo, item_lo + n_items); n_items_global = 0 means
     * unsharded (n_items_global = n_items, item_lo = 0).  W_q0 / W_p1t / b_p1 and their Adam moments hold
     * only the local rows; CSR indices are local; fake-pair and candidate ids stay global. */
    int32_t item_lo;
    int32_t n_items_global;
    /* operand precision of the discriminator GEMMs (forward and backward; discriminator.py:16-55 is fp32):
     * LTG_PREC_FP32 = the reference's arithmetic (default of the host layer), LTG_PREC_BF16, LTG_PREC_FP8
     * (BASELINE config 5).  Accumulation, activations, loss, Adam and the master weights are fp32 in every mode. */
    int32_t d_precision;
    /* arithmetic of the fp32 discriminator's GEMMs (d_precision = LTG_PREC_FP32, config.ini-sized layers; discriminator.py:23-55, train.py:142-143,163):
     * LTG_DARITH_FP32 = v_mfma_f32_16x16x4_f32, the exact fp32 fma chain; LTG_DARITH_BF16X6 = every fp32 operand split into three bf16 terms
     * (x = hi + mid + lo exactly) and the six leading cross terms multiplied on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- leaves out
     * 2^-26 |a b| per product, below fp32's own rounding of it; LTG_DARITH_BF16X4 = two terms per operand, four cross terms (2^-17 per product:
     * NOT fp32-accurate, opt-in).  Bits 4-7 (measurements only): which of the step's four GEMM kernels take the split form (l1, l2, bwd1, bwd2;
     * 0 = the library's choice). */
    int32_t d_arith;
    float lr, beta1, beta2, adam_eps;
    uint64_t seed;
} ltg_config;

/* Generator parameters + Adam moments, reference order (MultiVAE.py:129-141):
 * 0 W_q0, 1 W_q1, 2 W_p0, 3 W_p1t, 4 b_q0, 5 b_q1, 6 b_p0, 7 b_p1. */
typedef struct ltg_gen_state {
    float* p[8];
    float* m[8];
    float* v[8];
    /* optional bf16 shadow of W_p1t: [n_items][608] bf16 (row = item, K zero-padded to 608), rebuilt by
     * ltg_refresh_shadow and kept in step by the Adam epilogue of the G step.  When present (and n_items >=
     * 8192, n_items % 8 == 0, bf16 precision, <= 128 rows) the decoder forward and the dh2 product stream it
     * (1216 B/item instead of 2400 B/item).  NULL: the fp32 rows are converted on the fly. */
    uint16_t* wp1t_bf16;
    /* optional lazy Adam clock of W_q0 (item slabs of 8192 items or more).  tf.train.AdamOptimizer (train.py:160-164) moves
     * every row of W_q0 every step, but a row's gradient is zero unless one of the batch's users holds the item, and a
     * zero-gradient step is a function of (W, m, v, lr_t) of that row alone: it can be applied LATER, step by step, with the
     * same arithmetic -- before the row is next read.  q0_last[i] = ordinal of the last G step applied to row i; q0_ord =
     * ordinal of the last G step issued (HOST value: the caller adds 1 after every ltg_g_step / ltg_g_bwd_rest);
     * q0_lr_hist[j % LTG_Q0_HIST] = lr_t of G step j (written by the library).  Every G step applies itself to the batch's
     * rows (caught up first), and catches up the rows i = ord (mod q0_period), so that no row lags more than q0_period steps
     * (1 <= q0_period <= LTG_Q0_HIST / 2).  Every forward catches up the rows it reads.  ltg_g_flush brings all rows to
     * q0_ord (before W_q0 / its moments are read by anything else: checkpoints, host copies).  Results are bit-identical
     * to the dense sweep.  q0_last == NULL: dense sweep every step. */
    int32_t* q0_last;
    float* q0_lr_hist;
    int32_t q0_ord;
    int32_t q0_period;
} ltg_gen_state;
#define LTG_Q0_HIST 1024

/* Discriminator: emb is read-only (discriminator.py:14 is not in d_params, :47).
 * Trainable order (discriminator.py:47): 0 w1, 1 b1, 2 w2, 3 b2, 4 w3, 5 b3, 6 w4, 7 b4. */
typedef struct ltg_disc_state {
    const float* emb;
    float* p[8];
    float* m[8];
    float* v[8];
    /* optional OPERAND-FORMAT shadows for d_precision = LTG_PREC_FP8 (all four or none; every layer size a multiple of 64):
     * OCP e4m3 bytes with the mode's static scales (embeddings and weights 2^8), k-contiguous for the forward GEMMs --
     * emb_fp8 [F][h0], w1t_fp8 [h1][h0], w2t_fp8 [h2][h0], w3t_fp8 [h3][h1+h2] (the weight shadows TRANSPOSED).  Built by
     * ltg_refresh_d_shadow, kept in step by the Adam sweep of ltg_d_step / ltg_d_apply.  When present the two forward layers
     * read 1 byte per operand element instead of converting 4-byte values on the fly. */
    const uint8_t* emb_fp8;
    uint8_t* w1t_fp8;
    uint8_t* w2t_fp8;
    uint8_t* w3t_fp8;
    /* optional fifth shadow (ABI v10): w3 in its OWN layout [h1+h2][h3] in e4m3 -- the operand of the backward product
     * dpre1 = dpre3 . w3^T, which contracts over h3.  With it (and h0, h1+h2, h3 multiples of 128, h1, h2 multiples of 64) every
     * backward GEMM of the step reads e4m3 bytes in operand format as well (csrc/ltg_fp8bwd.h); without it they convert fp32
     * operands on the fly.  Same values either way. */
    uint8_t* w3_fp8;
} ltg_disc_state;

/* A batch of user rows in CSR form (replaces the dense [B,I] float32 feed of train.py:194-198).
 * indptr holds absolute offsets into indices/values.  The transposed view (the batch's entries grouped
 * by item) is only required by the G step (sparse gradient of W_q0):
 *   uitem[u]  = u-th distinct item of the batch (ascending),  uptr[u..u+1] = its entry range,
 *   rowidx/csr_pos = per entry: local row, index into indices[];  slot[i] = u or -1 for every item i. */
typedef struct ltg_batch {
    int32_t n_rows;
    int32_t n_unique;       /* number of distinct items in the batch */
    const int32_t* indptr;  /* [n_rows+1] */
    const int32_t* indices; /* item ids, ascending within a row */
    const float* values;    /* NULL => 1.0f */
    const int32_t* slot;    /* [n_items] item -> index into uitem / the gradient rows, or -1.  May be NULL: the library then builds the
                             * map of the batch in its workspace each step (no n_batches x n_items cache on the caller's side) */
    const int32_t* uptr;    /* [n_unique+1] offsets into rowidx/csr_pos (relative to 0) */
    const int32_t* rowidx;  /* local row of each transposed entry */
    const int32_t* csr_pos; /* index of that entry in indices[] */
    const float* row_norm2; /* optional [n_rows]: sum x^2 over the FULL row (needed when the items are sharded) */
    const int32_t* uitem;   /* optional [n_unique] (ABI v11): the distinct items themselves, ascending.  The same value as
                             * indices[csr_pos[uptr[u]]] -- with it the kernels that walk the distinct items (catch-up of the lazy Adam
                             * clock, sparse W_q0 gradient) learn the item in ONE dependent load instead of three and can request its
                             * weight / moment rows before the gather has returned */
} ltg_batch;

/* Activations of one generator forward; caller-owned, sizes for n_rows rows.
 * logits/lse are what the sampler, the G step and the metrics consume. */
typedef struct ltg_gen_acts {
    float* h1;      /* [n_rows][H]   tanh(enc0) */
    float* mulv;    /* [n_rows][2Z]  mu | logvar */
    float* z;       /* [n_rows][Z] */
    float* h2;      /* [n_rows][H]   tanh(dec0) */
    float* logits;  /* [n_rows][I] */
    float* lse;     /* [n_rows]      log-sum-exp of the row */
    float* kl_rows; /* [n_rows]      per-row KL (MultiVAE.py:161) */
    float* row_scale; /* [n_rows]    1/(keep*||x||_2) */
} ltg_gen_acts;

/* Optional timing probe: the library records the two HIP events (hipEvent_t) around the launch of the
 * kernel `kernel_id` on the call's stream.  Measurement only; NULL = off. */
#define LTG_K_ENC0_FWD 1
#define LTG_K_ENC1 2
#define LTG_K_DEC0 3
#define LTG_K_DEC1_FWD 4
#define LTG_K_D_L1 5
#define LTG_K_D_L2 6
#define LTG_K_D_BWD1 7
#define LTG_K_D_BWD2 8
#define LTG_K_D_ADAM 9
#define LTG_K_DH2 10
#define LTG_K_DEC1_BWD_ADAM 11
#define LTG_K_ENC0_BWD_ADAM 12
#define LTG_K_DZ 13
#define LTG_K_DH1 14
#define LTG_K_WGRAD_P0 15
#define LTG_K_WGRAD_Q1 16
#define LTG_K_ROW_DLOGITS 17 /* softmax statistics + losses + dlogits of a row (small item slabs) */
#define LTG_K_ENC0_GRAD 18   /* sparse gradient rows of W_q0 */
#define LTG_K_G_TAIL 19      /* the generator's Adam updates as jobs of one launch */
#define LTG_K_EXCH_H1 20      /* ltg_g_step_sharded: the three in-stream exchanges (events around the collective call on the step's stream) */
#define LTG_K_EXCH_ROWPART 21
#define LTG_K_EXCH_DH2 22
#define LTG_K_COUNT 23
typedef struct ltg_probe {
    int32_t kernel_id;
    int32_t reserved0;
    void* ev_start;
    void* ev_stop;
} ltg_probe;

typedef struct ltg_fwd_opts {
    float keep_prob;   /* keep_prob_ph, default 0.75 (MultiVAE.py:31) -- ON at inference too (Q3) */
    float is_training; /* is_training_ph (MultiVAE.py:101) */
    uint64_t rng_step; /* counter for the on-device RNG */
    const uint8_t* drop_keep; /* optional keep flags, indexed like indices[] (drop_keep[e] belongs to indices[e]) */
    const float* eps;         /* optional [n_rows][Z] */
    const ltg_probe* probe;   /* optional */
    /* ltg_vae_forward over SEVERAL batches at once (phase C / evaluation need no weight update in between): rows
     * [k * rows_per_step, (k + 1) * rows_per_step) draw their dropout with counter rng_step + k and row index r - k * rows_per_step,
     * i.e. exactly what k separate calls with consecutive rng_step values draw.  0 = one batch.  Needs is_training == 0. */
    int32_t rows_per_step;
    int32_t reserved0;
} ltg_fwd_opts;

/* Fake/real (popular, niche) id pairs.  Rows with id < 0 are holes (dropped pairs, Q9/Q10). */
typedef struct ltg_pairs {
    int32_t n;              /* number of slots */
    int32_t reserved0;
    const int32_t* pop;     /* [n] popular item id */
    const int32_t* niche;   /* [n] niche / generated item id */
    const int32_t* row;     /* [n] local user row of the pair (fake pairs; may be NULL for real) */
} ltg_pairs;

typedef struct ltg_d_opts {
    float keep_prob;    /* 0.7 (train.py:300) */
    int32_t adam_t;     /* shared Adam step AFTER this update (t >= 1), Q5 */
    uint64_t rng_step;
    const uint8_t* drop_real[3]; /* optional keep flags [n_real][h1], [n_real][h2], [n_real][h3] */
    const uint8_t* drop_fake[3];
    const ltg_probe* probe; /* optional */
    /* optional (ABI v12; ltg_d_step at the fp32 default sizes): jobs B / C of the backward's first stage -- dw3, db3, dw4, db4, d_loss: they
     * need the forward only -- run on `aux_stream` beside the critical chain job A -> stage 2, handed over through device words like
     * ltg_pipe's: sync = 4 zeroed words owned by the caller (LTG_WORD_D_FWD_DONE: forward complete, LTG_WORD_D_JOBS_DONE: jobs B / C ended, LTG_WORD_POISON: polls that gave up:
     * the Adam sweep then returns at once and the caller must treat it as fatal), seq = the call's ordinal on these words (+ 1 per
     * call, starting at 1).  The two streams must run concurrently (ltg_g_pipe_probe tests a pair).  NULL: one stream, five launches. */
    ltg_stream aux_stream;
    uint32_t* sync;
    uint32_t seq;
    int32_t reserved0;
} ltg_d_opts;

typedef struct ltg_g_opts {
    ltg_fwd_opts fwd;   /* keep 0.75, is_training 1 (train.py:326) */
    float anneal;       /* anneal_ph */
    float gan_lambda;   /* gen_lambda */
    float d_keep_prob;  /* 0.7 */
    int32_t adam_t;     /* shared Adam step AFTER this update */
    uint64_t d_rng_step;
    const uint8_t* drop_fake[3]; /* optional */
    const int32_t* cnt;  /* device scalar: sampled_cnt (number of valid fake pairs) */
    const ltg_probe* probe; /* optional (the forward part uses fwd.probe) */
    /* optional fork/join: run the fake-tower forward on aux_stream concurrently with the generator forward.
     * ev_fork / ev_join are caller-created hipEvent_t (the library allocates nothing); all three or none. */
    ltg_stream aux_stream;
    void* ev_fork;
    void* ev_join;
    /* item-sharded runs: ltg_g_bwd_dec1 already updated W_p1t / b_p1 of this step (issued while the dh2 all-reduce was in
     * flight), ltg_g_bwd_rest must not do it again */
    int32_t dec1_done;
    /* item-sharded runs: ltg_g_fake_tower already left the fake tower's forward in the workspace (issued on another stream
     * beside the generator forward and its exchanges), ltg_g_bwd_dec must not run it again.  0 or 1. */
    int32_t fake_done;
    /* optional third caller-created hipEvent_t (with aux_stream): ltg_g_step then runs the rotating slice of the lazy Adam
     * clock of W_q0 (arithmetic-bound) on aux_stream, beside the HBM-bound decoder kernels, and joins it at the end */
    void* ev_sweep;
    /* optional y_generated of this batch's fake pairs [fake->n], computed ahead by ltg_fake_tower_batched with this step's
     * d_rng_step: the step then runs no fake tower at all */
    const float* y_pre;
} ltg_g_opts;

/* Static per-user sampling inputs for a batch (results of the index path, data_processing.py). */
typedef struct ltg_sample_inputs {
    int32_t n_rows;
    int32_t max_cand;         /* max candidate-set length in this batch (sizes the LDS key buffer; <= 16384) */
    const int32_t* cand_ptr;  /* [n_rows+1]  USER_TAGS_TO_SAMPLE (data_processing.py:170-224) */
    const int32_t* cand_idx;  /* ascending candidate item ids */
    const int32_t* pop_ptr;   /* [n_rows+1]  user's popular list in file order (data_processing.py:72-96) */
    const int32_t* pop_idx;
    const int32_t* n_sample;  /* [n_rows] to_sample = len(user niche list); 0 => invalid user (Q8) */
    const int32_t* slot_ptr;  /* [n_rows+1] prefix sum of n_sample: output slot range per user */
    const uint8_t* valid_item;/* [I] 1 if the id is in ITEM_FEATURE_DICT (Q9) */
    uint64_t rng_step;
    const float* u_gumbel;    /* optional [n_cand total] uniforms aligned with cand_idx */
    const float* u_pick;      /* optional [n_slots] uniforms aligned with slots */
    const float* cand_logit;  /* optional, aligned with cand_idx: replaces the [B,I] logits (item-sharded runs) */
    /* several batches in one call (see ltg_fwd_opts.rows_per_step): rows of group k = r / rows_per_step draw with counter
     * rng_step + k and row index r % rows_per_step, and add their valid pairs to cnt_out[k].  0 = one batch. */
    int32_t rows_per_step;
    int32_t reserved0;
} ltg_sample_inputs;

int32_t ltg_abi_version(void);

/* Bytes of workspace needed by any entry point for at most max_rows user rows and max_pairs
 * discriminator rows (real+fake) per call. */
size_t ltg_workspace_bytes(const ltg_config* cfg, int32_t max_rows, int32_t max_pairs);
/* Bytes of the optional scratch of ltg_vae_forward (its ws argument) for at most max_rows rows: row statistics of large item
 * slabs in one pass.  Without it (ws == NULL or smaller) the forward computes them row by row. */
size_t ltg_forward_scratch_bytes(const ltg_config* cfg, int32_t max_rows);

/* Generator forward: replaces sess.run(generator_out, {input_ph: X}) -- Codes/train.py:200, :339,
 * Codes/test.py:146 (graph: MultiVAE.py:145-186, softmax :143).  Fills `acts`; if probs_out != NULL
 * also writes softmax probabilities [n_rows][I] (Q1). */
int ltg_vae_forward(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch,
                    const ltg_fwd_opts* opts, const ltg_gen_acts* acts, float* probs_out,
                    void* ws, size_t ws_bytes, ltg_stream stream);

/* Fake-pair sampling for one batch: replaces the Python loop Codes/train.py:212-251 including
 * sample_from_generator_new (Codes/sample.py:40-67).  Reads logits/lse of ltg_vae_forward.
 * Writes gen_out/pop_out [n_slots] (-1 = hole) and cnt_out[0] = number of valid pairs. */
int ltg_sample_pairs(const ltg_config* cfg, const ltg_sample_inputs* in, const float* logits,
                     const float* lse, int32_t* gen_out, int32_t* pop_out, int32_t* cnt_out,
                     ltg_stream stream);

/* Discriminator update: replaces sess.run([d_trainer, d_loss_mean]) -- Codes/train.py:300
 * (graph discriminator.py:3-58, loss train.py:142, Adam train.py:160-163).
 * loss_out[0] = d_loss (device). */
int ltg_d_step(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* real,
               const ltg_pairs* fake, const ltg_d_opts* opts, float* loss_out, void* ws,
               size_t ws_bytes, ltg_stream stream);

/* ---- The discriminator step cut at its exchange point, for multi-GPU runs that split the PAIR ROWS over ranks:
 * the logical pair batch is the concatenation real | fake (rows 0 .. real->n + fake->n); a rank runs forward + backward over
 * rows [row_lo, row_hi) with the full step's dropout draw (the counter RNG is indexed by the global row) and gets ONE
 * gradient vector: ltg_d_grad_floats(cfg) floats = the eight trainable tensors in discriminator.py:47 order back to back
 * (w1, b1, w2, b2, w3, b3, w4, b4), then this rank's share of d_loss (train.py:142), padded to whole float4.  The host
 * all-reduces (sum) that vector with RCCL; ltg_d_apply then runs the identical TF-Adam sweep on every rank and writes
 * d_loss.  ltg_d_step == ltg_d_grad over all rows + ltg_d_apply.  opts->adam_t is ignored by ltg_d_grad. */
size_t ltg_d_grad_floats(const ltg_config* cfg);
int ltg_d_grad(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* real, const ltg_pairs* fake, int32_t row_lo,
               int32_t row_hi, const ltg_d_opts* opts, float* grad_out, void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_d_apply(const ltg_config* cfg, const ltg_disc_state* disc, const float* grad, int32_t adam_t, float* loss_out,
                ltg_stream stream);

/* Generator update: replaces sess.run([g_trainer, g_loss_mean, g_vae_loss, gan_loss]) --
 * Codes/train.py:326 (losses train.py:145-157, Adam :164).  The dense mask feed `generated_tags`
 * is replaced by the (row, gen id) list of `fake`.  loss_out (device, >= 8 floats): [0..2] = g_loss,
 * vae_loss, gan_loss; [3] = sum_S p, [4] = sum_j y_j, [5] = c = lambda/cnt * sum_j y_j. */
int ltg_g_step(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_disc_state* disc,
               const ltg_batch* batch, const ltg_pairs* fake, const ltg_g_opts* opts,
               const ltg_gen_acts* acts, float* loss_out, void* ws, size_t ws_bytes,
               ltg_stream stream);

/* ---- The generator step cut at its three exchange points, for item-sharded multi-GPU runs (one process per
 * GPU; the collectives between the stages are issued by the host with RCCL, the library itself never
 * communicates).  ltg_g_step == the four stages back to back with n_ranks = 1.
 *   ltg_g_fwd_enc   enc-0 over the local item slab -> acts->h1 = partial PRE-activation   [all-reduce sum h1]
 *   ltg_g_fwd_rest  bias+tanh, enc-1, reparam, dec-0, local logits, row partials [n_rows][5] [all-gather]
 *   ltg_g_bwd_dec   combine partials (lse, losses), fake tower, dlogits, local dh2 [n_rows][H] [all-reduce sum]
 *   ltg_g_bwd_rest  Adam on the local W_p1t/b_p1 rows, replicated middle layers, local W_q0 rows
 * ltg_rowstats_combine: lse of the full rows from all-gathered partials (phase C / evaluation).
 * ltg_gather_cand_logits: this rank's candidate logits, 0 elsewhere (all-reduce -> ltg_sample_inputs.cand_logit). */
int ltg_g_fwd_enc(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch, const ltg_fwd_opts* opts,
                  const ltg_gen_acts* acts, ltg_stream stream);
int ltg_g_fwd_rest(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch, const ltg_pairs* fake,
                   const ltg_fwd_opts* opts, const ltg_gen_acts* acts, float* rowpart_out, void* ws, size_t ws_bytes,
                   ltg_stream stream);
int ltg_rowstats_combine(const ltg_config* cfg, const float* rowpart_all, int32_t n_ranks, int32_t n_rows, float* lse_out,
                         void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_g_bwd_dec(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_disc_state* disc, const ltg_batch* batch,
                  const ltg_pairs* fake, const ltg_g_opts* opts, const ltg_gen_acts* acts, const float* rowpart_all,
                  int32_t n_ranks, float* loss_out, float* dh2_out, void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_g_bwd_rest(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch, const ltg_pairs* fake,
                   const ltg_g_opts* opts, const ltg_gen_acts* acts, const float* dh2, void* ws, size_t ws_bytes,
                   ltg_stream stream);
/* The part of ltg_g_bwd_rest that does not need the all-reduced dh2: Adam on the local W_p1t / b_p1 rows (reads dlogits and
 * h2 of ltg_g_bwd_dec).  Issue it right after starting the dh2 all-reduce, then call ltg_g_bwd_rest with opts->dec1_done = 1. */
/* The fake tower's forward of a G step (replicated on every rank; needs only the fake pairs and the discriminator) into the
 * workspace ltg_g_bwd_dec reads it from: same cfg / n_rows / fake / ws as that call, any stream -- the caller orders it
 * after the previous step's ltg_g_bwd_dec and before this step's, and sets ltg_g_opts.fake_done = 1. */
int ltg_g_fake_tower(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* fake, const ltg_g_opts* o, int32_t n_rows, void* ws,
                     size_t ws_bytes, ltg_stream stream);
/* The fake tower's forward (discriminator.py:52-55 on x_popular_g / x_generated; the only part of the discriminator the g_trainer
 * fetch needs, train.py:326) for MANY pair batches in one pass -- the discriminator does not move during phase G (train.py:307-329)
 * and the fake pairs are fixed for the epoch, so every y_generated of a sub-epoch is known before its first G step.
 * fake = the concatenated slots of the batches; seg_of[fake->n] = index s of the batch each slot belongs to, seg_row0[s] = first
 * slot of batch s (the dropout RNG sees a slot's row INSIDE its batch), seg_step[s] = the d_rng_step the G step of batch s will
 * use: the same draws, the same bits as the tower inside ltg_g_step.  y_out[fake->n] (0 for holes); the G steps take their slice
 * through ltg_g_opts.y_pre.  ws: ltg_workspace_bytes(cfg, 1, fake->n). */
int ltg_fake_tower_batched(const ltg_config* cfg, const ltg_disc_state* disc, const ltg_pairs* fake, const int32_t* seg_of,
                           const int32_t* seg_row0, const uint64_t* seg_step, float d_keep_prob, float* y_out, void* ws, size_t ws_bytes,
                           ltg_stream stream);
int ltg_g_bwd_dec1(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch, const ltg_pairs* fake,
                   const ltg_g_opts* opts, const ltg_gen_acts* acts, void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_gather_cand_logits(const ltg_config* cfg, const ltg_sample_inputs* in, const float* logits, float* out,
                           ltg_stream stream);

/* ---- The item-sharded generator step as ONE call (ABI v10): every launch of the step AND its three exchanges issued in-stream,
 * with the two off-critical-path pieces of step t running beside step t + 1.  Replaces the five-call sequence ltg_g_fwd_enc ..
 * ltg_g_bwd_rest (one sess.run per step in the reference, train.py:326) for the configuration every large item slab runs in:
 * bf16 decoder operands with the W_p1t shadow, the lazy Adam clock of W_q0, n_items >= 8192, n_items % 8 == 0, <= 128 rows
 * (ltg_g_step_sharded_ok tells; other configurations use the cut-point calls above).
 *
 * Collectives: the library links no communication library.  The caller hands in its communicator and the two entry points with
 * the signatures of ncclAllReduce / ncclAllGather (rccl.h:611, :678; enums passed as int: LTG_NCCL_FLOAT32 = ncclFloat32,
 * LTG_NCCL_SUM = ncclSum) -- on a GPU node the addresses of RCCL's own functions, so the exchanges are RCCL kernels on the
 * caller's stream between the library's kernels (no host round trip); a test rig may pass host functions that synchronise
 * the stream and reduce through another backend.  comm == NULL: no exchange (one GPU); a communicator of ONE rank still gets its
 * three calls (the single-GPU proxy of a rank's step measures them).
 *
 * Pipeline (ltg_pipe: ONE caller-created side stream, two events and the exchange buffers; the library allocates nothing).
 * One fork per step, behind the dh2 product of step t (the last reader of the W_p1t shadow), puts onto the side stream the Adam update
 * of the local W_p1t / b_p1 rows of step t (HBM-bound, the largest kernel; needs only dlogits and h2): it runs beside the rest of
 * step t's backward and the encoder half of step t + 1's forward.  The rotating slice of the lazy Adam clock that step t - 1 owes (rows
 * i = ord (mod q0_period) up to ordinal ord = t - 1) runs on the side stream too, between the catch-up of call t and that of call t + 1.
 *
 * Hand-over between the two streams: a cross-stream event pair costs ~12 us per direction on this hardware and ~6 us of bubble on the
 * recording stream (scripts/micro/sync_cost.hip), so the streams meet through words of device memory (ltg_pipe.sync; `seq` = the
 * call's ordinal) -- no packet waits on the caller's stream at all:
 *   (enum ltg_word below names every word and says who stores it and who polls for it)
 * Every poll is made by ONE thread: a one-wave kernel of the side stream, or -- on the caller's stream -- the last thread of the kernel
 * IN FRONT of the one that needs the word (enc-1 for H2_READ, dec-0 for UPDATE_END, enc-0 for TAIL_END, the step's last kernel for SLICE_DONE): stream order then
 * gates the consumer whatever its size, and no workgroup of a large launch holds a CU while it waits for a producer that may still
 * need one.  Once LTG_WORD_POISON is non-zero every kernel of the step that writes h2 or the model returns at once, so the model stays what it
 * was when the wait expired; the caller checks that word before it reads the model out (end of a phase, checkpoint) and treats it as fatal.
 * LTG_PIPE_SLICE_IN_TOUCH keeps the slice in the catch-up launch of call t (one launch over the batch's rows and the slice's rows; a
 * row in both sets goes to whichever workgroup's atomic max on its clock comes first).  LTG_PIPE_EVENTS (or sync == NULL) selects event
 * pairs instead of words: stream waits on events recorded by the PREVIOUS call (a never-recorded event does not block), the slice in
 * the catch-up launch.  A pipe is used in ONE mode between two joins, seq increases by 1 per call; the two streams of the device-word
 * mode must be concurrent (ltg_g_pipe_probe).  After a call that FAILED the caller synchronises, zeroes the words and restarts seq at 0.
 * Before anything else reads W_p1t / W_q0 / their moments (ltg_g_flush, ltg_vae_forward, a checkpoint) the caller runs
 * ltg_g_pipe_join on the stream that will read them.  Results equal ltg_g_step's / the cut-point sequence's bit for bit (same
 * kernels, same order of additions; the slice only runs later).
 *
 * Catch-up AHEAD (ABI v13; device-word mode with the slice on the side stream, batches that carry `uitem`, h_enc <= 768): the catch-up
 * of the lazy clock -- the rows of W_q0 the batch reads, brought up to the caller's clock before enc-0 -- is the FIRST kernel of the
 * step's critical chain and moves 24 B per parameter of every distinct row.  A caller that knows the NEXT batch sets
 * ltg_pipe.next_uitem / next_nu: call t then brings those rows up to ordinal t ON THE SIDE STREAM, behind its slice (so LTG_WORD_SLICE_DONE covers
 * it), beside its own forward -- every row except the ones batch t itself holds (those get step t's gradient from the sparse gradient
 * kernel and are at t with it).  Which rows batch t holds is read from ltg_pipe.q0_mark (one int32 per local item, zeroed once by the
 * caller and with every reset of seq): the catch-up -- or the ahead kernel of the call before -- stores the call's ordinal there.  The
 * zero-gradient steps are the same expressions in the same order, only earlier: results do not change by a bit.  Call t + 1 on the
 * SAME batch the pipe announced, with nothing else having moved gen->q0_ord in between, sets ltg_pipe.caught_up = 1 and the library
 * launches no catch-up.  ltg_g_step_sharded_plan says whether a call with these arguments runs the ahead kernel. */
#define LTG_NCCL_FLOAT32 7
#define LTG_NCCL_SUM 0
typedef struct ltg_comm {
    void* comm;      /* ncclComm_t */
    int32_t n_ranks; /* >= 1 */
    int32_t rank;
    int (*all_reduce)(const void* sendbuf, void* recvbuf, size_t count, int dtype, int op, void* comm, ltg_stream stream);
    int (*all_gather)(const void* sendbuf, void* recvbuf, size_t sendcount, int dtype, void* comm, ltg_stream stream);
} ltg_comm;

/* One-shot exchange over peer-mapped staging buffers: a second transport with ltg_comm's entry-point signatures (csrc/ltg_oneshot.h;
 * correctness only -- RCCL is the transport of every measurement).  The caller allocates ltg_oneshot_stage_bytes() bytes of ZEROED device
 * memory per rank, shares them between the ranks (hipIpcGetMemHandle / hipIpcOpenMemHandle: stage[q] = rank q's buffer as mapped into this
 * process, stage[rank] = its own), and puts &ltg_oneshot into ltg_comm.comm with ltg_oneshot_all_reduce / ltg_oneshot_all_gather as the
 * entry points.  HOST structure: the library advances `seq` with every exchange (all ranks issue the same sequence of exchanges); counts up
 * to max_floats (all-gather: per rank); float32 / sum only.  Replaces nothing in the reference (Codes/train.py has no distributed code). */
#define LTG_ONESHOT_MAX_RANKS 16
typedef struct ltg_oneshot {
    int32_t n_ranks;
    int32_t rank;
    uint32_t seq;      /* exchanges issued so far; 0 at start */
    uint32_t limit_ms; /* bound of a device-side wait for a peer's message (0 = 30 s); a wait that gives up counts in `expired` of the stage */
    size_t max_floats;
    void* stage[LTG_ONESHOT_MAX_RANKS];
} ltg_oneshot;
size_t ltg_oneshot_stage_bytes(int32_t n_ranks, size_t max_floats);
/* byte offset of the `expired` counter (uint32) inside a rank's stage: the host reads it after a synchronisation */
size_t ltg_oneshot_expired_offset(int32_t n_ranks);
int ltg_oneshot_all_reduce(const void* sendbuf, void* recvbuf, size_t count, int dtype, int op, void* comm, ltg_stream stream);
int ltg_oneshot_all_gather(const void* sendbuf, void* recvbuf, size_t sendcount, int dtype, void* comm, ltg_stream stream);

/* The device words of a pipe (indices into ltg_pipe.sync; `seq` = the ordinal of the call that stores the word).  THE description of each:
 * who stores it, who polls for it.  ltg_d_step's fork (ltg_d_opts.sync) has two words of its own and the same poison index. */
enum ltg_word {
    LTG_WORD_DH2_DONE = 0,   /* the dh2 product of call seq is complete (stored by the slab sum when it starts -- with two shadow buffers by the
                              * product itself when it starts: dlogits is complete; a one-wave kernel in front of the weight update polls) */
    LTG_WORD_H2_READ = 1,    /* the weight update of call seq has READ h2 -- it reads h2 in its prologue only: its workgroups count themselves
                              * in LTG_WORD_H2_COUNT behind it and the last one stores the ordinal (ragged slabs: the generic tile kernel on the
                              * last n_items % 32 rows reads h2 throughout, the word is stored with LTG_WORD_UPDATE_END).  Polled by the last
                              * thread of call seq + 1's enc-1, in front of dec-0, which overwrites h2 */
    LTG_WORD_POISON = 2,     /* polls that gave up (each is bounded: 30 s) = the pipe's POISON: every kernel of the step that writes h2 or the
                              * model returns at once when it is set */
    LTG_WORD_PROBE = 3,      /* ltg_g_pipe_probe's gate, and in the word behind it (4) its own count of polls that gave up */
    LTG_WORD_CATCHUP = 5,    /* enc-0 of call seq has started = the catch-up of the batch's rows is complete (a one-wave kernel in front of the
                              * clock slice on the side stream polls) */
    LTG_WORD_SLICE_DONE = 6, /* the clock's work beside call seq -- its slice and, ABI v13, the catch-up of the next batch's rows -- has ended
                              * (stored by the next kernel of the side stream, the waiter in front of the weight update, when it starts).  Polled
                              * by the last thread of call seq's OWN last kernel on the caller's stream: the catch-up of call seq + 1 must not
                              * meet the slice on a row */
    LTG_WORD_UPDATE_END = 7, /* the weight update of call seq has ENDED (one wave behind it).  Polled by the last thread of call seq + 1's dec-0,
                              * in front of the streaming forward, which reads the shadow rows and the bias the update writes */
    LTG_WORD_H2_COUNT = 8,   /* the update's workgroups that are past their prologue (see LTG_WORD_H2_READ) */
    LTG_WORD_DH1_DONE = 9,   /* dh1 of call seq is complete (stored by the sparse gradient kernel when it starts; a one-wave kernel in front of
                              * the Adam tail on ltg_pipe.tail_stream polls) */
    LTG_WORD_TAIL_END = 10,  /* that tail has ended (one wave behind it).  Polled by the last thread of call seq + 1's enc-0, in front of enc-1,
                              * which reads what the tail updates */
    /* ltg_d_opts.sync */
    LTG_WORD_D_FWD_DONE = 0, /* the forward is complete (stored by job A's launch when it starts, polled by one wave in front of jobs B / C) */
    LTG_WORD_D_JOBS_DONE = 1 /* jobs B / C have ended (one wave behind them; polled by an extra block of stage 2 in front of the Adam sweep) */
};

typedef struct ltg_pipe {
    ltg_stream side_stream;
    void* ev_fork; /* hipEvent_t x 2, timing disabled (LTG_PIPE_EVENTS and ltg_g_pipe_join) */
    void* ev_dec1;
    void* ev_tail; /* hipEvent_t, timing disabled: ltg_g_pipe_join's join of tail_stream (NULL: no tail stream) */
    float* h1pre;       /* [n_rows][H]  exchange 1: partial encoder pre-activation, all-reduced in place */
    float* rowpart_all; /* [n_ranks][n_rows][5]  exchange 2: all-gather IN PLACE (this rank writes block `rank`, n_rows = the call's batch) */
    float* dh2;         /* [n_rows][H]  exchange 3: local dh2, all-reduced in place */
    int32_t flags;      /* LTG_PIPE_* measurement switches, 0 = the shipped schedule */
    uint32_t seq;       /* ordinal of this call on this pipe: the caller adds 1 before every ltg_g_step_sharded call (starting at 1) */
    uint32_t* sync;     /* [16] device words, zeroed once by the caller: the hand-overs of enum ltg_word.
                         * NULL: the hand-overs are events (ev_fork / ev_dec1), as with LTG_PIPE_EVENTS */
    ltg_stream tail_stream; /* optional THIRD stream (ABI v12; device-word mode only): the step's Adam tail -- W_p0, W_q1 and the biases; it needs
                             * the backward's dh1 only -- runs there beside the sparse W_q0 gradient, the next call's catch-up and enc-0
                             * (LTG_WORD_DH1_DONE / LTG_WORD_TAIL_END); used with LTG_PIPE_TAIL_OWN only.  NULL: the tail is the step's last kernel on the caller's stream */
    /* catch-up ahead (ABI v13; all optional, see above) */
    int32_t* q0_mark;           /* [n_items] int32, zeroed by the caller (and again whenever seq restarts): ordinal of the last call whose batch holds the row */
    const int32_t* next_uitem;  /* the NEXT call's ltg_batch.uitem (its distinct local items) or NULL */
    int32_t next_nu;            /* ... and its n_unique */
    int32_t caught_up;          /* 1: the previous call on this pipe was given THIS batch as next_uitem / next_nu and gen->q0_ord moved by that call only */
    /* second shadow buffer (ABI v13; optional, device-word mode): [n_items][608] bf16 like gen->wp1t_bf16, K padding zero.  The weight update
     * of the call writes the new shadow rows HERE instead of in place, so it starts when dlogits is complete -- beside the dh2 product, the
     * last reader of gen->wp1t_bf16 -- instead of behind it.  AFTER the call the caller exchanges gen->wp1t_bf16 and shadow_out. */
    uint16_t* shadow_out;
} ltg_pipe;
#define LTG_PIPE_NO_DEC1_FORK 1  /* everything on the caller's stream, in program order */
#define LTG_PIPE_NO_SLICE_FORK 2 /* the lazy clock's slice on the caller's stream, at the end of its own step */
#define LTG_PIPE_SLICE_IN_TOUCH 32 /* with device words: the slice step t - 1 owes in the catch-up launch of call t (as with events) instead of on the
                                      side stream between the catch-up of call t and that of call t + 1 */
#define LTG_PIPE_EVENTS 16       /* fork and join of the weight update as hipEventRecord / hipStreamWaitEvent pairs instead of device words */
#define LTG_PIPE_WIDE_GRAD 8     /* the sparse W_q0 gradient in its column-blocked shape (three times the waves) although it runs beside the update */
#define LTG_PIPE_TAIL_OWN 128    /* the Adam tail on ltg_pipe.tail_stream (default: the step's last kernel on the caller's stream -- measured, see csrc: pipe_plan) */
/* a flags bit outside these: ltg_g_step_sharded returns LTG_EINVAL */

int ltg_g_step_sharded_ok(const ltg_config* cfg, const ltg_gen_state* gen, int32_t n_rows);
/* What ltg_g_step_sharded will do with this batch and this pipe (the caller's bookkeeping depends on it): two fields of
 * ltg_g_pipe_plan's struct (below) as bits:
 *   LTG_PLAN_AHEAD   it brings the rows announced in next_uitem up to date and honours caught_up
 *   LTG_PLAN_SHADOW  its weight update writes pipe->shadow_out (the caller exchanges it with gen->wp1t_bf16 after the call)
 * 0 also when the call would be refused. */
#define LTG_PLAN_AHEAD 1
#define LTG_PLAN_SHADOW 2
int ltg_g_step_sharded_plan(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch, const ltg_pipe* pipe);
int ltg_g_step_sharded(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_disc_state* disc, const ltg_batch* batch,
                       const ltg_pairs* fake, const ltg_g_opts* opts, const ltg_gen_acts* acts, const ltg_comm* comm,
                       const ltg_pipe* pipe, float* loss_out, void* ws, size_t ws_bytes, ltg_stream stream);

/* ---- kernel routes (additive in ABI v14).  Which kernels a call with this configuration, this state and this many rows runs: the library decides it
 * once per call, in one place (csrc/ltg_kernels.hip: g_route / d_route), and every stage switches on the result.  The two queries below
 * hand that decision out, so that a test can say which route a shape reaches.  Host-only: they look at the PRESENCE of the pointers in
 * the structs they are handed (and, for the Adam sweep, at whether the tensors lie back to back) and dereference none of them; 1 = *out
 * is filled, 0 = the configuration is refused (or an argument is missing). */
enum { LTG_ENC0_GENERIC = 0, LTG_ENC0_FAST };                   /* k_enc0_fwd | fk_enc0_fwd */
enum { LTG_MID_DENSE = 0, LTG_MID_FAST };                       /* k_dense_fwd pair (+ k_reparam; backward: five launches) | fk_enc1 / fk_dec0 (backward: fk_g_tail jobs) */
enum { LTG_DEC_TILE = 0, LTG_DEC_SMALL, LTG_DEC_STREAM1, LTG_DEC_STREAM2 };   /* k_dec1_fwd | fk_dec1 | k_dec1_fwd_stream | k_dec1_fwd_stream2 */
enum { LTG_STATS_ROW = 0, LTG_STATS_SEGMENT, LTG_STATS_EPILOGUE };            /* k_row_lse / k_row_partial | segment pass | the streaming decoder's epilogue */
enum { LTG_LOSS_GENERIC = 0, LTG_LOSS_COMBINE, LTG_LOSS_ROW };  /* k_g_combine + k_dlogits | k_dlogits_combine | fk_row_dlogits (small slab) */
enum { LTG_DH2_PARTIAL = 0, LTG_DH2_SMALL, LTG_DH2_STREAM };    /* k_dh2_partial | fk_dh2 | k_dh2_stream */
enum { LTG_DW_TILE = 0, LTG_DW_TAIL_JOB, LTG_DW_STREAM };       /* k_dec1_bwd_adam | a job of fk_g_tail (small slab) | k_dec1_bwd_adam_stream */
enum { LTG_Q0_DENSE = 0, LTG_Q0_SWEEP, LTG_Q0_LAZY };           /* dense product in the tail | slot-map sweep | lazy clock */
typedef struct ltg_g_route_info {
    int32_t enc0;        /* LTG_ENC0_* */
    int32_t small;       /* 1: the small-slab step (one launch per stage, dense enc-0 operand rows) */
    int32_t mid;         /* LTG_MID_*: middle layers forward, and the backward chain behind dh2 */
    int32_t mid_vec;     /* LTG_MID_DENSE: 16-byte loaders */
    int32_t dec;         /* LTG_DEC_* */
    int32_t dec_tile;    /* LTG_DEC_TILE: 128 = 64 x 128 tiles, 32 = 32 x 32 */
    int32_t stats;       /* LTG_STATS_*, given scratch for them (without: LTG_STATS_ROW) */
    int32_t seg_pass;    /* 1: the slab is long enough for the segment pass (forward-only calls ask for scratch only then) */
    int32_t loss;        /* LTG_LOSS_* */
    int32_t dlog_bf16;   /* 1: dlogits stored as bf16 (producer and both consumers read this one field) */
    int32_t dh2;         /* LTG_DH2_* */
    int32_t dh2_tile;    /* LTG_DH2_PARTIAL: 128 = 64 x 128 tiles, -32 = 32 x 32 with 16-byte loads, 32 = 32 x 32 */
    int32_t dh2_chunk;   /* items per partial slab, and how many of them */
    int32_t dh2_nsplit;
    int32_t dw;          /* LTG_DW_* */
    int32_t dw_tile;     /* LTG_DW_TILE: 64, -32 (16-byte loads), 32 */
    int32_t dw_ragged;   /* 1: LTG_DW_STREAM with the generic tile kernel on the last n_items % 32 rows */
    int32_t q0;          /* LTG_Q0_* */
    int32_t q0_own_launch; /* 1: the W_q0 update is a launch of its own, not a job of the tail */
    int32_t grad_rows;   /* 1: the sparse W_q0 gradient one wave per row (0: column-blocked) */
    int32_t sharded_ok;  /* 1: ltg_g_step_sharded serves this (= ltg_g_step_sharded_ok) */
} ltg_g_route_info;
int ltg_g_route(const ltg_config* cfg, const ltg_gen_state* gen, int32_t n_rows, ltg_g_route_info* out);

/* ---- the pipe's schedule (additive in ABI v14).  Where each stage of ltg_g_step_sharded runs and what it waits for, decided once per call in
 * one place (csrc/ltg_kernels.hip: pipe_plan) from ltg_pipe.flags and the PRESENCE of pointers; every stage, ltg_g_step_sharded_plan and
 * ltg_g_pipe_join read the result.  Host-only like the routes: nothing is dereferenced on the device; 1 = *out is filled, 0 = the call
 * would be refused (a flags bit outside LTG_PIPE_*, a configuration ltg_g_step_sharded_ok refuses, a missing argument). */
enum { LTG_HAND_ORDER = 0,   /* LTG_PIPE_NO_DEC1_FORK: one stream, program order */
       LTG_HAND_EVENTS,      /* fork and join of the weight update are event pairs (LTG_PIPE_EVENTS, or no sync words) */
       LTG_HAND_WORDS };     /* ... device words (enum ltg_word) */
enum { LTG_SLICE_OWN_END = 0, /* the lazy clock's slice of step t at the end of step t, on the caller's stream */
       LTG_SLICE_IN_TOUCH,    /* the slice step t - 1 owes in the catch-up launch of call t */
       LTG_SLICE_SIDE };      /* ... on the side stream, between the catch-up of call t and that of call t + 1 */
typedef struct ltg_pipe_plan_info {
    int32_t handover;    /* LTG_HAND_* */
    int32_t slice;       /* LTG_SLICE_* */
    int32_t ahead;       /* 1: the call brings the rows announced in next_uitem up to date and honours caught_up (LTG_PLAN_AHEAD) */
    int32_t shadow;      /* 1: the weight update writes pipe->shadow_out (LTG_PLAN_SHADOW) */
    int32_t tail_own;    /* 1: the Adam tail runs on pipe->tail_stream */
    int32_t h2_early;    /* 1: LTG_WORD_H2_READ opens behind the update's prologue (0: with its end) */
    int32_t grad_rows;   /* 1: the sparse W_q0 gradient one wave per row (0: column-blocked, LTG_PIPE_WIDE_GRAD) */
    int32_t poisonable;  /* 1: the step's kernels look at LTG_WORD_POISON */
} ltg_pipe_plan_info;
int ltg_g_pipe_plan(const ltg_config* cfg, const ltg_gen_state* gen, const ltg_batch* batch, const ltg_pipe* pipe, ltg_pipe_plan_info* out);

enum { LTG_D_GENERIC = 0,    /* k_d_*<mode> */
       LTG_D_TOWER,          /* forward only: the one-kernel tower */
       LTG_D_STAGED_FWD,     /* forward only: fks_d_l1 -> fks_d_l2 -> fk_d_y */
       LTG_D_FAST,           /* fk_d_* */
       LTG_D_FP8_OPFMT,      /* fp8, every operand in operand format (the step) */
       LTG_D_FP8_STAGED,     /* fp8 LDS-staged forward (+ generic backward) */
       LTG_D_FP8_REG };      /* fp8 register-block forward (+ generic backward) */
enum { LTG_D_ADAM_TENSORS = 0, LTG_D_ADAM_FLAT, LTG_D_ADAM_FP8 };   /* k_d_adam | fk_d_adam | k8_d_adam */
typedef struct ltg_d_route_info {
    int32_t kind;        /* LTG_D_* */
    int32_t mode;        /* template mode of the generic kernels: 0 fp32, 1 bf16, 2 fp8 */
    int32_t tile[4];     /* generic kernels l1, l2, bwd1, bwd2: 128 / 64 / -32 (32 x 32, 16-byte loads) / -33 (on operand A only) / 32 */
    int32_t spl[4];      /* LTG_D_FAST: bf16 terms per product of fk_d_l1, fk_d_l2, fk_d_bwd1, fk_d_bwd2 (0 = fp32 MFMA) */
    int32_t adam;        /* LTG_D_ADAM_*: the step's sweep */
    int32_t fork;        /* 1: jobs B / C of the backward run on the aux stream */
} ltg_d_route_info;
int ltg_d_route(const ltg_config* cfg, const ltg_disc_state* disc, int32_t n_pairs, int32_t with_bwd, int32_t has_aux, ltg_d_route_info* out);
/* 1: `stream` and pipe->side_stream (and pipe->tail_stream, and those two with each other) run concurrently (a waiter on one does not hold
 * up the other), as the device-word hand-over needs;
 * 0: they share a hardware queue (HIP maps streams onto a few of them) -- use another side stream, or LTG_PIPE_EVENTS; < 0: error.
 * Synchronises both streams; uses LTG_WORD_PROBE and the word behind it.  Call it once per (stream, side stream) pair before the first step. */
int ltg_g_pipe_probe(const ltg_pipe* pipe, ltg_stream stream);
/* `stream` waits for the forked pieces of the last ltg_g_step_sharded call (dec1_stream, q0_stream). */
int ltg_g_pipe_join(const ltg_pipe* pipe, ltg_stream stream);
/* (re)build gen->wp1t_bf16 from gen->p[3] (after initialisation or after loading weights). */
int ltg_refresh_shadow(const ltg_config* cfg, const ltg_gen_state* gen, ltg_stream stream);
/* lazy Adam clock of W_q0 (ltg_gen_state.q0_last): apply every deferred zero-gradient step, all rows up to gen->q0_ord */
int ltg_g_flush(const ltg_config* cfg, const ltg_gen_state* gen, ltg_stream stream);
/* (re)build the e4m3 operand shadows of the discriminator (ltg_disc_state.emb_fp8 ... w3t_fp8) from the fp32 tensors. */
int ltg_refresh_d_shadow(const ltg_config* cfg, const ltg_disc_state* disc, ltg_stream stream);

/* Ranking metrics on device: replaces pred[X.nonzero()] = -inf (Codes/train.py:341) +
 * NDCG_binary_at_k_batch / Recall_at_k_batch (Codes/eval_functions.py:11-62).
 * tr = fold-in rows (masked), te = held-out rows, same n_rows.  out [n_rows][4] =
 * {ndcg@k_ndcg, recall@k_r1, recall@k_r2, valid flag (IDCG != 0)}. */
int ltg_rank_metrics(const ltg_config* cfg, const float* logits, const ltg_batch* tr,
                     const ltg_batch* te, int32_t k_ndcg, int32_t k_r1, int32_t k_r2, float* out,
                     ltg_stream stream);

/* The same metrics cut at their two exchange points for item-sharded runs (cfg->item_lo / n_items = this rank's
 * slab; tr holds LOCAL column ids of the slab, te GLOBAL ids; score/count arrays are indexed like te->indices, i.e.
 * by the absolute entry positions te->indptr holds):
 *   ltg_rank_scores  score_out[e] = logit of held-out entry e if this rank owns the item (-inf if it is a fold-in
 *                    item of that row, train.py:341), 0 otherwise                       -> all-reduce(sum)
 *   ltg_rank_counts  count_out[e] = #{local items ranked before entry e} (ties: lower GLOBAL id first, like
 *                    ltg_rank_metrics)                                                  -> all-reduce(sum)
 *   ltg_rank_finish  NDCG / Recall per row from the summed counts (eval_functions.py:24-38, :54-62). */
int ltg_rank_scores(const ltg_config* cfg, const float* logits, const ltg_batch* tr, const ltg_batch* te,
                    float* score_out, ltg_stream stream);
int ltg_rank_counts(const ltg_config* cfg, const float* logits, const ltg_batch* tr, const ltg_batch* te,
                    const float* score, int32_t* count_out, ltg_stream stream);
int ltg_rank_finish(const ltg_batch* te, const int32_t* counts, int32_t k_ndcg, int32_t k_r1, int32_t k_r2,
                    float* out, ltg_stream stream);

/* Top-K recommendations on device (the reference ranks users' items only to score them, Codes/test.py:135-171).
 * ltg_topk: per row of logits [n_rows][cfg->n_items] (this rank's slab; global id = cfg->item_lo + column) the k best
 * items, fold-in items of tr (LOCAL column ids, like ltg_rank_metrics; ascending per row; tr may be NULL = no fold-in)
 * excluded: score_out [n_rows][k] = the logits, id_out [n_rows][k] = GLOBAL ids.  Order: score descending, equal scores
 * lower global id first (the rank ltg_rank_metrics counts, so Recall@k from the ids equals its Recall@k); -0.0 == +0.0;
 * -inf logits are eligible; a row with fewer than k eligible items is padded with id -1 / score -inf; NaN logits are
 * outside the contract.  1 <= k <= 1024, n_items <= 360 448; bit-identical from run to run.
 * ltg_topk_merge: the top-k of the union of n_parts lists per row, score_in / id_in [n_parts][n_rows][k_in], each list
 * sorted and padded as ltg_topk writes it, over disjoint item sets (the slabs of an item-sharded run, gathered): for
 * slabs cut from one row it equals ltg_topk on the whole row bit for bit.  1 <= k_in, k <= 1024. */
int ltg_topk(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, float* score_out,
             int32_t* id_out, ltg_stream stream);
int ltg_topk_merge(int32_t n_parts, int32_t n_rows, int32_t k_in, const float* score_in, const int32_t* id_in, int32_t k,
                   float* score_out, int32_t* id_out, ltg_stream stream);

/* Minimum slots per item group at serve time (additive in ABI v14).
 * ltg_topk_groups: ltg_topk with one more condition of eligibility.  item_group [n_items_global] uint8 = the report's labels, one per
 * GLOBAL item id (the label of column c is item_group[cfg->item_lo + c]); bit g of group_mask (g = 0..7) admits label g, bit 8
 * every label >= 8.  An item is eligible iff it is not a fold-in item of tr and its label's bit is set.  Everything else is ltg_topk's
 * contract: the order, the padding (a row with fewer than k eligible items, down to none), 1 <= k <= 1024, n_items <= 360 448,
 * bit-identical from run to run; group_mask = 0x1FF gives ltg_topk's lists bit for bit.  LTG_EINVAL before any HIP call: item_group
 * NULL, group_mask 0 or > 0x1FF, item_lo < 0 or item_lo + n_items > n_items_global, and whatever ltg_topk refuses.
 * ltg_topk_quota: the list with at least quota[j] entries of reserved list j, composed from lists alone.  score_all / id_all
 * [n_rows][k_in] = the plain lists (ltg_topk / ltg_topk_merge); score_grp / id_grp [n_lists][n_rows][m_in] = one reserved list per
 * group (ltg_topk_groups with a single-bit mask, so pairwise disjoint per row), all sorted and padded as ltg_topk writes them;
 * quota [n_lists] is a HOST array, read before the call returns.  Per row, with U = the first quota[j] entries of every list j
 * (padding ignored): out [n_rows][k] = U + the first (k - |U|) entries of the plain list that are not in U, in ltg_topk's order,
 * padded with id -1 / score -inf.  With 0 <= quota[j] <= m_in and sum quota <= k <= k_in this is, walking the row's full ranking
 * from the top, "take an item if its group still owes slots, or if a slot is left that no group's outstanding minimum claims"
 * (a group with fewer eligible items than its quota hands the rest to the free slots); quota all 0 = the first k of the plain
 * list, quota[j] = k = list j.  Scores are copied, never recomputed; ids are never used as an index.  1 <= n_lists <= 8,
 * 1 <= m_in <= 1024, 1 <= k <= k_in <= 1024; anything else, and a NULL pointer, is LTG_EINVAL before any HIP call; n_rows = 0
 * returns 0.  score_out / id_out must not alias any input.  No workspace, no global atomics, run-to-run identical. */
int ltg_topk_groups(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k,
                    const uint8_t* item_group, int32_t n_items_global, uint32_t group_mask, float* score_out, int32_t* id_out,
                    ltg_stream stream);
int ltg_topk_quota(int32_t n_rows, int32_t k_in, const float* score_all, const int32_t* id_all, int32_t n_lists, int32_t m_in,
                   const float* score_grp, const int32_t* id_grp, const int32_t* quota, int32_t k, float* score_out,
                   int32_t* id_out, ltg_stream stream);

/* Long-tail report from top-K lists (additive in ABI v14): per user and item group NDCG@k_ndcg / Recall@k_r1 / Recall@k_r2, and
 * the exposure counts, without another scan of the logits.  id_in [n_rows][k_in] as ltg_topk / ltg_topk_merge write it (GLOBAL
 * ids in rank order, distinct, padding -1); te = held-out rows, GLOBAL ids ascending per row, te->n_rows == n_rows; item_group
 * [n_items_global] uint8 labels, a label >= n_groups belongs to no group; 1 <= n_groups <= 8; every cutoff in [1, k_in],
 * 1 <= k_in <= 1024.  out [n_rows][n_groups + 1][4] = {ndcg, recall@k_r1, recall@k_r2, valid} per slot: slot g < n_groups counts
 * the held-out items with label g (valid = the user has one), slot n_groups every held-out item.  With rank(h) = position of h
 * in the list: ndcg = sum_{rank(h) < k_ndcg} 1/log2(rank(h)+2) / sum_{r < min(|H|, k_ndcg)} 1/log2(r+2), recall@k =
 * #{rank(h) < k} / min(k, |H|) (eval_functions.py:11-62 on the held-out matrix restricted to the group's columns).
 * item_hits [n_items_global] int32 (may be NULL) is ADDED to: +1 for every item among a user's first k_exp list entries; the
 * caller zeroes it once per split.  Ids outside [0, n_items_global) are never used as an index.
 * For rows with finite logits and disjoint fold-in / held-out sets, slot n_groups equals ltg_rank_metrics bit for bit and slot g
 * equals ltg_rank_metrics on the held-out CSR filtered to group g; otherwise (a held-out fold-in item, -inf logits inside the
 * first k_in) they may differ.  Inherits ltg_topk's limits (n_items per slab <= 360 448, k <= 1024).  No floating-point atomics. */
int ltg_topk_metrics(const int32_t* id_in, int32_t n_rows, int32_t k_in, const ltg_batch* te, const uint8_t* item_group,
                     int32_t n_items_global, int32_t n_groups, int32_t k_ndcg, int32_t k_r1, int32_t k_r2, int32_t k_exp,
                     float* out, int32_t* item_hits, ltg_stream stream);

/* Item-to-item neighbours: fused cosine / dot top-K over an item table (additive in ABI v14).
 * Space: LTG_SPACE_DECODER = the rows of W_p1t (gen->p[3]), LTG_SPACE_ENCODER = the rows of W_q0 (gen->p[0]; the caller runs ltg_g_flush
 * first when the lazy clock is in use).  Metric: LTG_METRIC_COSINE or LTG_METRIC_DOT.
 * ltg_item_pack: the slab's table -> the operand image image_out [n_items][608] bf16 in the layout of gen->wp1t_bf16 (row = item, K
 * zero-padded to 608).  dot: element = bf16 round-to-nearest-even of the fp32 value (decoder / dot == ltg_refresh_shadow bit for bit).
 * cosine: the row's squared norm summed in fp64, inv = (float)(1.0 / sqrt(norm2)), element = bf16 RNE of the single fp32 product
 * x * inv; a row of norm 0 gives a row of zeros (score 0, never NaN).  Queries are items: the same call packs them, and a query image is
 * rows of a table image.  LTG_EINVAL: NULL pointer, unknown space / metric, h_enc > 608.
 * ltg_item_neighbors: per query row r of q_image [n_q][608] the k best items of this rank's slab (table_image [n_items][608], global id =
 * cfg->item_lo + row).  Score of (r, j) = the fp32 accumulator of the bf16 MFMA product of the two image rows over the 19 K blocks in
 * ascending order; it does not depend on where j sits in the slab, so an item-sharded run produces the unsharded scores bit for bit.
 * Item j is eligible for row r iff j != q_gid[r] (GLOBAL id; -1 excludes nothing) and, when item_group != NULL ([n_items_global] uint8,
 * one label per GLOBAL id), bit min(label, 8) of group_mask is set -- ltg_topk_groups' rule.  score_out / id_out [n_q][k] exactly as
 * ltg_topk writes them: scores descending, equal scores lower GLOBAL id first, padding id -1 / score -inf, bit-identical from run to
 * run, NaN outside the contract -- per-slab lists go straight into ltg_topk_merge.  1 <= k <= LTG_NBR_MAX_K; the slab is streamed, so
 * ltg_topk's 360 448 items per slab do not apply (the image of a slab must stay below 2^32 bytes: 3 532 110 items).
 * The workspace (ltg_item_neighbors_ws_bytes; 0 for arguments the call refuses) holds one list per (item segment, query row) -- segments x
 * n_q x k (score, id) pairs, at most 64 segments -- never a block of the score matrix.
 * Before any HIP call: LTG_EINVAL for a NULL pointer (item_group may be NULL), n_q < 0, k out of range, group_mask 0 or > 0x1FF when
 * item_group is given, item_lo < 0 or item_lo + n_items > n_items_global, h_enc > 608; LTG_EWORKSPACE for ws_bytes too small; n_q = 0
 * returns LTG_OK and touches nothing. */
#define LTG_SPACE_DECODER 0
#define LTG_SPACE_ENCODER 1
#define LTG_METRIC_COSINE 0
#define LTG_METRIC_DOT 1
#define LTG_NBR_MAX_K 256
int ltg_item_pack(const ltg_config* cfg, const ltg_gen_state* gen, int32_t space, int32_t metric, uint16_t* image_out, ltg_stream stream);
size_t ltg_item_neighbors_ws_bytes(const ltg_config* cfg, int32_t n_q, int32_t k);
int ltg_item_neighbors(const ltg_config* cfg, const uint16_t* table_image, const uint16_t* q_image, const int32_t* q_gid, int32_t n_q,
                       const uint8_t* item_group, uint32_t group_mask, int32_t k, float* score_out, int32_t* id_out, void* workspace,
                       size_t ws_bytes, ltg_stream stream);

/* Diversified top-K lists: greedy maximal marginal relevance over a row's candidate list (additive in ABI v14).
 * image [image_rows][608] bf16 as ltg_item_pack writes it, row r = GLOBAL id image_lo + r (16-byte aligned); score_in / id_in
 * [n_rows][c_in] sorted and padded as ltg_topk writes them; 1 <= k <= c_in <= LTG_DIV_MAX_C.  An entry whose id lies outside
 * [image_lo, image_lo + image_rows) is padding, and so is everything behind it: the image is never indexed with an unchecked id.  A
 * non-padding entry with a non-finite score is outside the contract.
 * Per row, n = the candidates in front of the padding, s their scores, S[i][j] = the fp32 accumulator of the 19-step
 * v_mfma_f32_16x16x32_bf16 chain over the image rows of candidates i and j (a score of ltg_item_neighbors, never rounded):
 *   rel_i = (s_i - s_{n-1}) / (s_0 - s_{n-1}) in fp32 (one subtraction pair, one IEEE division); all 0 when s_0 == s_{n-1};
 *   the first pick is position 0; after a pick p, m_i = S[i][p] (first pick) or max(m_i, S[i][p]);
 *   the next pick is the position not yet picked with the largest obj_i = lambda * rel_i - (1 - lambda) * m_i -- two fp32 products and
 *   one subtraction, no contraction, 1 - lambda computed once in fp32 -- equal objectives to the lowest position.
 * score_out / id_out [n_rows][k] = the picks in pick order, min(k, n) of them, each with its ORIGINAL score bit for bit (so the list is
 * generally not descending in score), then padding id -1 / score -inf.  lambda = 1 gives the first k candidates bit for bit.
 * stat_out (may be NULL) [n_rows][2] = the mean of S over the unordered pairs among the first min(k, n) candidates, and over the
 * pairs of the output list; 0 with fewer than two entries; fp32 sums.
 * One launch, one workgroup per row, S stays in LDS; no workspace, no atomics outside LDS, bit-identical from run to run.
 * LTG_EINVAL before any HIP call: image / score_in / id_in / score_out / id_out NULL, c_in outside [1, 256], k outside [1, c_in],
 * lambda outside [0, 1] or NaN, image_rows < 1, image_lo < 0, n_rows < 0, image not 16-byte aligned; n_rows = 0 returns LTG_OK. */
#define LTG_DIV_MAX_C 256
int ltg_topk_diversify(const uint16_t* image, int32_t image_lo, int32_t image_rows, int32_t n_rows, int32_t c_in,
                       const float* score_in, const int32_t* id_in, float lambda, int32_t k, float* score_out, int32_t* id_out,
                       float* stat_out /* may be NULL */, ltg_stream stream);

/* Item audiences: the k likeliest users of an item, selected down the columns of the row-major logits (additive in ABI v14).
 * ltg_item_audience: per query column q_col[q] (LOCAL column of logits [n_rows][cfg->n_items]; q_col is DEVICE memory, need not be sorted
 * or distinct -- duplicates give identical lists; the caller validates its values) the k best eligible rows of THIS chunk.  Score of
 * (row, column) = logits[row][column] - lse[row], one fp32 subtraction (the log-probability the row's softmax gives the item); lse NULL:
 * the raw logit.  Row r is eligible iff the column is not in r's fold-in list of tr (LOCAL ids, ascending per row, as ltg_topk takes
 * them; tr NULL: every row is eligible); -inf scores are eligible, NaN is outside the contract.  score_out / id_out [n_q][k] exactly as
 * ltg_topk writes a list with id = row_lo + row: score descending, equal scores lower row first, -0.0 == +0.0, padding id -1 / score
 * -inf (n_rows < k pads), bit-identical from run to run.  The call is pure per chunk; chunks over disjoint row ranges accumulate with
 * ltg_topk_merge (n_parts = 2: the running lists and this chunk's; n_rows = n_q; k_in = k).
 * The logits are read once, every request a run along a row, and are not modified; the [n_rows][n_q] scores are never written anywhere.
 * The workspace (ltg_item_audience_ws_bytes; 0 for arguments the call refuses, and 0 when the chunk is walked as one row segment: ws may
 * then be NULL) holds one list per (row segment, query) -- segments x n_q x k (score, id) pairs, at most 32 segments.
 * 1 <= k <= LTG_AUD_MAX_K.  LTG_EINVAL before any HIP call: cfg / logits / q_col / score_out / id_out NULL, k out of range, n_rows, n_q
 * or row_lo negative, row_lo + n_rows > INT32_MAX, a tr whose n_rows differs from the call's or that lacks indptr / indices, a workspace
 * that is NULL or too small when one is needed.  n_rows = 0 or n_q = 0 launches nothing and returns LTG_OK. */
#define LTG_AUD_MAX_K 256
size_t ltg_item_audience_ws_bytes(const ltg_config* cfg, int32_t n_rows, int32_t n_q, int32_t k);
int ltg_item_audience(const ltg_config* cfg, const float* logits, const float* lse /* [n_rows] or NULL */, const ltg_batch* tr /* or NULL */,
                      int32_t n_rows, int32_t row_lo, const int32_t* q_col, int32_t n_q, int32_t k, float* score_out, int32_t* id_out,
                      void* ws, size_t ws_bytes, ltg_stream stream);

/* Why a user got a list entry: per (user row, entry) the r history items of that user nearest to the entry (additive in ABI v14;
 * DESIGN 5.14).  image [image_rows][608] bf16 as ltg_item_pack writes it, row i = GLOBAL id image_lo + i (16-byte aligned).  id_in
 * [n_rows][k_in]: lists as ltg_topk / ltg_topk_merge / ltg_topk_quota / ltg_topk_diversify write them; the first `top` entries of every
 * row are explained, 1 <= top <= min(k_in, LTG_WHY_MAX_TOP).  tr: the fold-in rows of the same users (tr->n_rows == n_rows, indptr absolute
 * offsets, ids ascending per row, values ignored); the GLOBAL id of a history item is hist_lo + indices[...] -- on an item-sharded rank
 * hist_lo = cfg->item_lo and tr holds the slab's part of the history.
 * Per (row u, entry e < top) with g = id_in[u][e]: the candidates are the history items h of row u whose global id lies inside
 * [image_lo, image_lo + image_rows) and differs from g; the score of h = the fp32 accumulator of the 19-step v_mfma_f32_16x16x32_bf16
 * chain over the image rows of g and h, K blocks ascending (a score of ltg_item_neighbors, never rounded; it depends neither on where
 * a row is staged nor on the slab the history item came from).  score_out / id_out [n_rows][top][r]: entry (u, e) holds the r best
 * candidates exactly as ltg_item_neighbors writes a list -- score descending, equal scores lower GLOBAL id first, -0.0 == +0.0, padding
 * id -1 / score -inf.  A g outside the image (padding -1 included) gets r paddings and, unlike ltg_topk_diversify, does not end the row.
 * No id, of the list or of the history, indexes the image unchecked.  Viewed as [n_rows * top][r] the outputs are ltg_topk-format lists:
 * per-slab outputs go straight into ltg_topk_merge (n_rows = n_rows * top, k_in = k = r).
 * One launch, one workgroup per row, the top x history scores stay in LDS; no workspace, no atomics, bit-identical from run to run.
 * LTG_EINVAL before any HIP call: image / tr / tr->indptr / tr->indices / id_in / score_out / id_out NULL, tr->n_rows != n_rows,
 * n_rows < 0, k_in outside [1, 1024], top outside [1, min(k_in, 256)], r outside [1, 8], image_rows < 1, image_lo < 0, hist_lo < 0, image
 * not 16-byte aligned; n_rows = 0 returns LTG_OK and launches nothing. */
#define LTG_WHY_MAX_TOP 256
#define LTG_WHY_MAX_R 8
int ltg_topk_explain(const uint16_t* image, int32_t image_lo, int32_t image_rows, const ltg_batch* tr, int32_t hist_lo, int32_t n_rows,
                     int32_t k_in, const int32_t* id_in, int32_t top, int32_t r, float* score_out, int32_t* id_out, ltg_stream stream);

/* Calibrated top-K lists: every user's list follows the class mix of that user's fold-in history (additive in ABI v14).
 * Classes: C = n_groups + 1, the class of an item = min(label, n_groups), the last class is "in no group"; 1 <= n_groups <= 8.
 *
 * ltg_hist_groups: count_out[u][c] (int32 [n_rows][C], WRITTEN, not added to) = the history items of row u whose GLOBAL id hist_lo +
 * indices[..] lies in [0, n_items_global) and whose class is c (item_group: uint8 per GLOBAL id); an id outside that range counts nowhere
 * and indexes nothing.  tr: the fold-in rows as ltg_topk_explain takes them (tr->n_rows == n_rows, indptr absolute, values ignored); on an
 * item-sharded rank hist_lo = cfg->item_lo, tr holds the slab's part of the histories and the host adds the counts (one int32 all-reduce).
 * One wave per row, no atomics, no workspace.  LTG_EINVAL before any HIP call: tr / indptr / indices / item_group / count_out NULL,
 * tr->n_rows != n_rows, n_rows < 0, hist_lo < 0, n_items_global < 1, n_groups outside [1, 8].
 *
 * ltg_topk_calibrate: score_grp / id_grp [n_lists][n_rows][m_in] = one ltg_topk_groups list per class that has one (the layout of
 * ltg_topk_quota's reserved lists; padding id < 0 ends a list; a non-padding entry with a non-finite score is outside the contract;
 * lists of different classes hold disjoint ids); list_class (HOST, read before the call returns) = their classes, strictly ascending in
 * [0, n_groups]; hist [n_rows][C] as ltg_hist_groups writes it (a class without a list has no candidates, its history still counts).
 * Per row, with h = the row of hist, H = sum h, n = the non-padding entries over all lists, kk = min(k, n):
 *   plain list = the first kk entries of the merge of the lists in ltg_topk's order; s_hi / s_lo its first / last score;
 *     rel(s) = (s - s_lo) / (s_hi - s_lo), two fp32 subtractions and one IEEE fp32 division; 0 for every s when s_hi == s_lo;
 *   tv of a list of m entries with class counts n_c = (float)((double)D / (double)(2 H m)), D = sum_c |h_c m - n_c H| (int64); 0 if H == 0;
 *   round t = 0 .. kk - 1 picks, among the heads of the lists not used up, the one with the largest
 *     obj = a * rel(s) - lambda * tv(list so far plus one entry of the head's class, m = t + 1),  a = 1 - lambda in fp32, two fp32 products
 *     and one subtraction, never contracted; equal objectives: the head that comes first in ltg_topk's order.
 * score_out / id_out [n_rows][k]: the picks in pick order, every one with its original score bit for bit (generally not descending), padded
 * with id -1 / score -inf.  stat_out ([n_rows][2], may be NULL) = {tv of the plain list, tv of the output}; both 0 when H == 0 or kk == 0.
 * lambda = 0 is the plain list.  One launch, no workspace, no atomics, bit-identical from run to run; ids never index anything; the outputs
 * must not alias the inputs.  LTG_EINVAL before any HIP call: a NULL pointer (stat_out and stream excepted), n_groups outside [1, 8],
 * n_lists outside [1, n_groups + 1], m_in outside [1, 1024], k outside [1, m_in], lambda outside [0, 1] or NaN, list_class not strictly
 * ascending or out of range, n_rows < 0.  For both: n_rows = 0 returns LTG_OK and launches nothing (the arguments are still checked). */
#define LTG_CAL_MAX_CLASSES 9
int ltg_hist_groups(const ltg_batch* tr, int32_t hist_lo, int32_t n_rows, const uint8_t* item_group, int32_t n_items_global,
                    int32_t n_groups, int32_t* count_out /* [n_rows][n_groups+1] */, ltg_stream stream);
int ltg_topk_calibrate(int32_t n_rows, int32_t n_lists, int32_t m_in, const float* score_grp, const int32_t* id_grp,
                       const int32_t* list_class /* HOST [n_lists] */, int32_t n_groups, const int32_t* hist /* device [n_rows][n_groups+1] */,
                       float lambda, int32_t k, float* score_out, int32_t* id_out, float* stat_out /* [n_rows][2], may be NULL */,
                       ltg_stream stream);

/* Exposure-capped top-K lists: no item appears in more than cap[item] of the served lists (additive in ABI v14).
 * cand_score / cand_id [n_rows][c_in]: every row's c_in best items as ltg_topk / ltg_topk_merge write them (logits descending, ties lower
 * id first, ids distinct within a row; the first id < 0 ends the row; an id >= n_items_global is skipped and never used as an index).
 * cap [n_items_global] int32 >= 0 per GLOBAL item id.  lse [n_rows] or NULL.  1 <= k <= c_in <= 1024, n_rows * c_in < 2^31.
 * Entry (u, j) carries the word  w = (key(s) << 32) | ((0x7FFFFFFF - u) << 1) | (s is -0.0),  s = fp32 (cand_score - lse[u]), the logit when
 * lse is NULL, key = ltg_topk's order-preserving key: ltg_item_audience's order -- score descending, equal scores lower row first, -0.0 ==
 * +0.0; -inf is eligible, NaN is outside the contract.  The result is the user-optimal stable many-to-many matching of user-proposing
 * deferred acceptance, stated as the least thresholds thr[item] (words, 0 at the start) such that, with active(u) = the first k entries of
 * row u whose cap[id] > 0 and whose word >= thr[id], no item has more than cap[item] active entries.  A round = propose (the active bytes
 * from thr) then accept (an item with more than cap active entries raises thr to its cap-th largest active word).  Thresholds only rise, a
 * round after convergence changes nothing, and the fixed point does not depend on the order or the batching of the rounds: lists are
 * bit-identical from run to run.  No floating-point atomics, no sort.
 *
 * ltg_cap_index   once per candidate table: the per-item index of the entries (global integer atomics for the counts and the cursors only;
 *                 nothing read from it depends on the order they leave), thr <- 0, state <- 0.
 * ltg_cap_rounds  enqueues n_rounds rounds (1 .. LTG_CAP_MAX_ROUNDS) back to back.  The matching has converged when a round raised no
 *                 threshold: state[4] < state[1] after a batch.  k, cap, lse and the candidates must be the same in every call of one matching.
 * ltg_cap_finish  score_out / id_out [n_rows][k] = the active entries of every row in candidate order, each with its original logit bit for
 *                 bit, padded with id -1 / score -inf (a row whose candidates run out gets a short list); fills state[2], state[3].
 * state (device, int32 [LTG_CAP_STATE]): [0] threshold raises so far, [1] rounds run, [2] entries passed over (catalogue entries before a
 * row's k-th active one -- all of them in a short row -- that are not active), [3] rows with a short list, [4] the last round that raised a
 * threshold (0: none), [5..7] 0.  ws: ltg_cap_ws_bytes(n_rows, c_in, n_items_global) bytes, 256-byte aligned, the same buffer through
 * index, rounds and finish.  LTG_EINVAL before any HIP call: a NULL pointer (lse and stream excepted), n_rows < 0, c_in outside [1, 1024],
 * k outside [1, c_in], n_items_global < 1, n_rows * c_in >= 2^31, n_rounds outside [1, LTG_CAP_MAX_ROUNDS], ws_bytes too small
 * (ltg_cap_ws_bytes returns 0 for sizes it refuses).  n_rows = 0 returns LTG_OK and launches nothing (the arguments are still checked). */
#define LTG_CAP_STATE 8
#define LTG_CAP_MAX_ROUNDS 64
size_t ltg_cap_ws_bytes(int32_t n_rows, int32_t c_in, int32_t n_items_global);
int ltg_cap_index(int32_t n_rows, int32_t c_in, const int32_t* cand_id, int32_t n_items_global, int32_t* state /* device [LTG_CAP_STATE] */,
                  void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_cap_rounds(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse /* may be NULL */,
                   const int32_t* cap /* device [n_items_global] */, int32_t n_items_global, int32_t k, int32_t n_rounds, int32_t* state,
                   void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_cap_finish(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, int32_t n_items_global, int32_t k,
                   float* score_out, int32_t* id_out, int32_t* state, void* ws, size_t ws_bytes, ltg_stream stream);

/* Share-targeted top-K lists: the promoted groups get `want` of all served slots, placed where they cost the least relevance (additive in
 * ABI v14).  Per row u a promoted list score_pro / id_pro [n_rows][m_in] and a rest list score_rest / id_rest [n_rows][m_in],
 * both as ltg_topk_groups writes them: sorted in ltg_topk's order, padded with id -1 / score -inf, the first id < 0 ends a list (whatever
 * lies behind it is ignored).  Ids are disjoint between the two lists and are never used as an index; a non-padding entry with a
 * non-finite score is outside the contract.  1 <= k <= m_in <= 1024, n_rows * k < 2^31, want (int64) >= 0.
 * Per row: np, nr = the non-padding entries of the two lists, kk = min(k, np + nr); plain list = the first kk entries of the merge of the two
 * lists in ltg_topk's order (score descending, -0.0 == +0.0, ties lower id first); a = how many of them are promoted, b = kk - a.
 * Steps t = 1 .. min(b, np - a): cost c_t = fp32(rest[b - t] - pro[a + t - 1]) (0-based, one IEEE fp32 subtraction; a result of +-0 is taken as
 * +0.0), word w = ((uint64)bits(c_t) << 32) | (u * k + t - 1).  Costs are >= 0, so the bits order as the floats do, and the words of a row
 * strictly increase with t.
 * Over all rows: A = sum a, N = the number of steps, take = min(max(0, want - A), N), thr = the take-th smallest word, t_u = the steps of
 * row u with w <= thr (a prefix; take = 0: t_u = 0).  Output row u = the first a + t_u entries of the promoted list and the first b - t_u of
 * the rest list, merged in ltg_topk's order, every entry with its original score bit for bit, padded with id -1 / score -inf.
 * Consequences: want <= A returns the plain lists bit for bit; want >= A + N returns every row at its limit; among all allocations that
 * move `take` slots the output has the least total step cost (the step costs of a row never decrease, so the globally cheapest steps
 * are a prefix of every row).
 * state (device, int32 [LTG_SHARE_STATE]): [0] A, [1] N, [2] take, [3] rows with t_u > 0, [4] the bits of the threshold's cost (0 if take = 0)
 * -- the marginal relevance price of a promoted slot -- [5] sum kk, [6..7] 0.
 * One call enqueues everything (a fixed 19 launches, no read-back in between): the steps, a radix select over the n_rows * k words (most
 * significant digit first, 8 bits a pass, 8 passes, LDS histograms added to global bins by integer atomics), the lists.  Integer atomics
 * only, no sort: bit-identical from run to run.  Nothing relies on what ws held.  ws: ltg_share_ws_bytes(n_rows, k) bytes (0 for sizes
 * the call refuses), 256-byte aligned.  LTG_EINVAL before any HIP call: a NULL pointer (stream excepted), n_rows < 0, m_in outside
 * [1, 1024], k outside [1, m_in], n_rows * k >= 2^31, want < 0, ws_bytes too small, an output that overlaps an input.  n_rows = 0 returns
 * LTG_OK, launches nothing and writes no state (the arguments are still checked). */
#define LTG_SHARE_STATE 8
size_t ltg_share_ws_bytes(int32_t n_rows, int32_t k);            /* 0 for sizes the call refuses */
int ltg_topk_share(int32_t n_rows, int32_t m_in, const float* score_pro, const int32_t* id_pro, const float* score_rest,
                   const int32_t* id_rest, int32_t k, int64_t want, float* score_out, int32_t* id_out,
                   int32_t* state /* device [LTG_SHARE_STATE = 8] */, void* ws, size_t ws_bytes, ltg_stream stream);

/* Exposure-floor top-K lists: every item with need[item] > 0 reaches need[item] of the served lists where enough users hold it among their
 * candidates (additive in ABI v14) -- the dual of the cap.  cand_score / cand_id / lse / the word w of an entry: as for
 * ltg_cap_*.  need [n_items_global] int32 per GLOBAL item id, <= 0: no floor.  1 <= k <= c_in <= 1024, 0 <= reserve <= k, n_rows * c_in < 2^31.
 * A FLOOR entry (u, j): j before the row's first padding id, 0 <= id < n_items_global, need[id] > 0.  The zone of a row: the positions
 * j >= k - reserve.  The result is the item-optimal stable matching of item-proposing deferred acceptance -- an item proposes to the users
 * that hold it, best word first, until it holds need acceptances; a user accepts every proposal before its zone and keeps, of those in
 * the zone, the `reserve` with the lowest positions -- stated as the greatest per-user limits lim[u] (c_in - 1 at the start, k - 1 when
 * reserve = 0) such that, with active(item) = its need floor entries with j <= lim[u] of the largest words (all of them if it has no
 * more), no row has more than `reserve` active entries in its zone.  A round = items (sel[item] = the need-th largest admissible word, 0 if
 * there are no more than need) then users (a row with more than `reserve` zone entries whose w >= sel[id] lowers lim[u] to the position
 * of the reserve-th).  Limits only fall, a round after convergence changes nothing, and the fixed point does not depend on the order or
 * the batching of the rounds: lists are bit-identical from run to run.  No floating-point atomics, no sort.
 * The list of row u: t = the smallest value for which the active entries at positions >= k - t are at most t (then exactly t; t <=
 * reserve); the first k - t candidates of the row, then those active entries in candidate order, each with its original logit bit for
 * bit; a row that ends before k - t is padded with id -1 / score -inf.  Rows stay in score order, every active entry is served, an item is
 * in at least min(need, held) lists; need all 0, or reserve = 0, gives the first k candidates bit for bit.
 *
 * ltg_floor_index   once per candidate table: the per-item index of the entries (ltg_cap_index's), lim <- c_in - 1, state <- 0.
 * ltg_floor_rounds  enqueues n_rounds rounds (1 .. LTG_FLOOR_MAX_ROUNDS) back to back, two launches each.  Converged when a round lowered
 *                   no limit: state[4] < state[1] after a batch.  k, reserve, need, lse and the candidates must be the same in every call
 *                   of one matching.
 * ltg_floor_finish  recomputes sel from the limits as they stand and writes score_out / id_out [n_rows][k]; active_out (uint8 [n_rows][c_in],
 *                   may be NULL) = the matching itself, held_out (int32 [n_items_global], may be NULL) = the active entries per item.
 *                   Before convergence a row counts only its first `reserve` active zone entries.
 * state (device, int32 [LTG_FLOOR_STATE]): [0] limit lowerings so far, [1] rounds run, [2] floor items that hold fewer entries than their
 * floor, [3] rows that differ from the plain top-k (t > 0), [4] the last round that lowered a limit (0: none), [5] inserted slots (the sum
 * of t), [6] floor items, [7] 0; [2], [3], [5..7] are filled by ltg_floor_finish.  ws: ltg_floor_ws_bytes(n_rows, c_in, n_items_global)
 * bytes, 256-byte aligned, the same buffer through index, rounds and finish; nothing relies on what it held before the index.
 * LTG_EINVAL before any HIP call: a NULL pointer (lse, active_out, held_out and stream excepted), n_rows < 0, c_in outside [1, 1024], k
 * outside [1, c_in], reserve outside [0, k], n_items_global < 1, n_rows * c_in >= 2^31, n_rounds outside [1, LTG_FLOOR_MAX_ROUNDS], ws_bytes
 * too small (ltg_floor_ws_bytes returns 0 for sizes it refuses).  n_rows = 0 returns LTG_OK and launches nothing (the arguments are still
 * checked). */
#define LTG_FLOOR_STATE 8
#define LTG_FLOOR_MAX_ROUNDS 64
size_t ltg_floor_ws_bytes(int32_t n_rows, int32_t c_in, int32_t n_items_global);
int ltg_floor_index(int32_t n_rows, int32_t c_in, const int32_t* cand_id, int32_t n_items_global, int32_t* state /* device [LTG_FLOOR_STATE] */,
                    void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_floor_rounds(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse /* may be NULL */,
                     const int32_t* need /* device [n_items_global] */, int32_t n_items_global, int32_t k, int32_t reserve, int32_t n_rounds,
                     int32_t* state, void* ws, size_t ws_bytes, ltg_stream stream);
int ltg_floor_finish(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse /* may be NULL */,
                     const int32_t* need, int32_t n_items_global, int32_t k, int32_t reserve, float* score_out, int32_t* id_out,
                     uint8_t* active_out /* may be NULL */, int32_t* held_out /* may be NULL */, int32_t* state, void* ws, size_t ws_bytes,
                     ltg_stream stream);

/* Niche companions: the discriminator's top-K partners of an item (additive in ABI v14).  The score of a (popular a, niche b)
 * pair is the discriminator's logit at keep = 1 (no dropout):
 *   s(a, b) = b4 + sum_{j < h3} w4[j] tanh(U[a][j] + V[b][j]),   U[a] = tanh(emb[a] w1 + b1) w3[0:h1],   V[b] = tanh(emb[b] w2 + b2) w3[h1:h1+h2] + b3
 * and sigmoid(s) is y of ltg_fake_tower_batched / ltg_d_step without dropout.  It does not separate into a product of item vectors, but
 * tanh(u + v) = 1 - 2 / (1 + exp(2u) exp(2v)) does: a SIDE IMAGE stores E = exp(2 x) per item and column, and the pair loop holds no
 * exponential.
 * ltg_pair_ld: floats per image row, >= d_h3 (d_h3 rounded up to a multiple of 4); 0 for a cfg the calls refuse (NULL, a layer width < 1,
 * d_feat < 1, d_h3 > 352, d_h0 + max(d_h1, d_h2) > 2048).
 * ltg_pair_pack: image_out [n][ld] fp32, row i for ids[i] (DEVICE int32, rows of disc->emb: 0 <= id < d_feat; other ids are outside the
 * contract, the host layer validates them), side LTG_PAIR_POP (branch A: w1, b1, w3[0:h1]) or LTG_PAIR_NICHE (branch B: w2, b2,
 * w3[h1:h1+h2], + b3).  Always computed from the fp32 MASTER weights disc->emb / disc->p[0..5] in fp32 (fmaf chains, tanhf), whatever
 * cfg->d_precision / d_arith the engine trains with: the operand shadows are not read.  Element = expf(2 clamp(x, -40, 40)) with libm's expf
 * (1 ulp), so E lies in [e^-80, e^80] and a product of two is never inf x 0; padding columns [d_h3, ld) are written (1.0) and are never
 * read by ltg_pair_companions.  Every element is one chain in a fixed order: an id's row is bit-identical wherever it sits in ids and
 * whatever n is.  LTG_EINVAL before any HIP call: a NULL pointer (stream excepted), an unknown side, n < 0, a cfg as above; n = 0 returns
 * LTG_OK.
 * ltg_pair_companions: per query row r of q_image [n_q][ld] (an image of one side) its k best candidates of c_image [n_c][ld] (an image of
 * the OTHER side; the kernel does not care which is which -- popular queries over niche candidates is the shelf of a head item, niche
 * queries over popular candidates its anchors).  Score of (r, c) = fma(-2, acc, c0) with c0 = (float)(b4 + sum_j w4[j]) summed in fp64 in
 * ascending j and acc the ONE chain acc <- fma(w4[j], rcp(fma(Eq[j], Ec[j], 1)), acc) from 0 over j = 0 .. d_h3 - 1 ascending (rcp =
 * v_rcp_f32, 1 ulp); it depends on nothing but the two image rows and disc->p[6], p[7], so candidates or queries split across calls
 * reproduce the same bits and item shards merge.  Candidate c is eligible for row r iff c_gid[c] != q_gid[r] (q_gid = -1 excludes
 * nothing); c_gid [n_c] DEVICE, strictly ascending global ids >= 0.  score_out / id_out [n_q][k] exactly as ltg_topk writes a list: scores
 * descending, equal scores lower global id first, -0.0 == +0.0, padding id -1 / score -inf when fewer than k are eligible, bit-identical
 * from run to run, NaN outside the contract -- per-part lists go straight into ltg_topk_merge.  1 <= k <= LTG_PAIR_MAX_K.  The workspace
 * (ltg_pair_companions_ws_bytes; 0 for arguments the call refuses and for n_q = 0) holds one list per (candidate segment, query row) --
 * at most 64 segments -- never a block of scores.  No atomics, no inline assembly.
 * Before any HIP call: LTG_EINVAL for a cfg as above, n_q < 0, n_c < 0, k out of range, a NULL pointer (stream excepted; c_image / c_gid
 * may be NULL when n_c = 0; the pointers are not looked at when n_q = 0); LTG_EWORKSPACE for ws_bytes too small.  n_q = 0 returns LTG_OK and
 * touches nothing; n_c = 0 gives all-padding lists. */
#define LTG_PAIR_POP 0
#define LTG_PAIR_NICHE 1
#define LTG_PAIR_MAX_K 256
int32_t ltg_pair_ld(const ltg_config* cfg);
int ltg_pair_pack(const ltg_config* cfg, const ltg_disc_state* disc, int32_t side, const int32_t* ids /* DEVICE [n], rows of emb */, int32_t n,
                  float* image_out /* [n][ld] */, ltg_stream stream);
size_t ltg_pair_companions_ws_bytes(const ltg_config* cfg, int32_t n_q, int32_t n_c, int32_t k);
int ltg_pair_companions(const ltg_config* cfg, const ltg_disc_state* disc, const float* q_image, const int32_t* q_gid, int32_t n_q,
                        const float* c_image, const int32_t* c_gid /* DEVICE [n_c], strictly ascending global ids */, int32_t n_c, int32_t k,
                        float* score_out, int32_t* id_out, void* ws, size_t ws_bytes, ltg_stream stream);

/* Critic-checked lists: the discriminator scores and gates each user's niche entries (additive in ABI v14).  s(a, b) is the pair
 * logit of ltg_pair_companions -- the same images, chain and c0, hence the same bits for the same two image rows.  For a user row u the
 * ANCHORS A_u are the history items (tr / hist_lo exactly as ltg_topk_explain takes them) whose global id g lies in [0, n_items_global)
 * with 0 <= pop_row[g] < n_pop; entry e < top of the row's list id_in [n_rows][k_in] is a CANDIDATE iff its id g lies in
 * [0, n_items_global) with 0 <= niche_row[g] < n_niche, and it is SCORED iff the user also has at least one anchor.  pop_row / niche_row:
 * DEVICE int32 [n_items_global], item id -> row of pop_image [n_pop][ld] / niche_image [n_niche][ld] (ltg_pair_pack images of the two
 * sides), -1 = not on that side.  No id of a list, a history or a map indexes anything unchecked.
 * Every pair logit becomes q = llrint((double) s * 2^24) (round to nearest even) and the integers are added: the sums do not depend on the
 * wave, workgroup, history block, call or rank that held an anchor.  Contract: |s| < 2^17 and fewer than 2^20 anchors per user.
 * ltg_pair_critic: per (row, entry e < top) sum_out [n_rows][top] int64 = the sum of q over the anchors of THIS call's histories (0 for an
 * entry that is no candidate), cnt_out [n_rows] int32 = those anchors' number, best_s / best_i [n_rows][top] = the anchor with the largest
 * s as a length-1 list in ltg_topk's format (equal scores the lower global id, -0.0 == +0.0; id -1 / score -inf when the entry is no
 * candidate or the call saw no anchor) -- over item shards the sums and counts are added as integers and the best anchors go through
 * ltg_topk_merge (n_rows = n_rows * top, k_in = k = 1).  One launch, one workgroup per row, no workspace, no atomics, bit-identical from
 * run to run.  1 <= top <= min(k_in, LTG_CRITIC_MAX_TOP), 1 <= k_in <= 1024.
 * ltg_critic_finish: crit_out [n_rows][top] = (float)((double) sum / ((double) cnt * 16777216.0)) for a scored entry (cnt = the user's
 * anchors over all parts), 0.0 for every other -- best_i = -1 flags those; scored_out [n_rows] int32 = the row's scored entries.
 * ltg_topk_gate: cand_score / cand_id [n_rows][c_in] lists as ltg_topk / ltg_topk_merge write them, crit [n_rows][c_in] and flag
 * [n_rows][c_in] (int32, >= 0: the entry is scored -- ltg_pair_critic's best_i), k <= c_in <= LTG_GATE_MAX_C.  Walking a row's candidates in
 * order, a non-padding entry passes iff it is unscored or crit >= tau; score_out / id_out [n_rows][k] = the first k passing entries with
 * their scores (a subsequence of the candidates, so in score order), padded with id -1 / score -inf; stat_out [n_rows][3] int32 = the
 * scored candidates, the candidates rejected before the list was full, the list's length.  tau = -inf passes everything: the plain
 * top-k.  One wave per row, ballot and prefix count, no sort.
 * All three: LTG_EINVAL before any HIP call for a NULL pointer (stream excepted), n_rows < 0, tr->n_rows != n_rows, hist_lo < 0, a size out
 * of the ranges above, n_items_global < 1, n_pop < 0, n_niche < 0, a NaN tau, and for ltg_pair_critic a cfg ltg_pair_ld refuses; n_rows = 0
 * returns LTG_OK and launches nothing. */
#define LTG_CRITIC_MAX_TOP 256
#define LTG_GATE_MAX_C 256
int ltg_pair_critic(const ltg_config* cfg, const ltg_disc_state* disc, const float* pop_image, int32_t n_pop, const float* niche_image,
                    int32_t n_niche, const int32_t* pop_row, const int32_t* niche_row, int32_t n_items_global, const ltg_batch* tr,
                    int32_t hist_lo, int32_t n_rows, int32_t k_in, const int32_t* id_in, int32_t top, int64_t* sum_out, int32_t* cnt_out,
                    float* best_s, int32_t* best_i, ltg_stream stream);
int ltg_critic_finish(int32_t n_rows, int32_t k_in, const int32_t* id_in, int32_t top, const int32_t* niche_row, int32_t n_items_global,
                      int32_t n_niche, const int64_t* sum, const int32_t* cnt, float* crit_out, int32_t* scored_out, ltg_stream stream);
int ltg_topk_gate(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* crit, const int32_t* flag,
                  float tau, int32_t k, float* score_out, int32_t* id_out, int32_t* stat_out, ltg_stream stream);

/* Exploration lists (additive, ABI v14): top-K SAMPLED without replacement under the Plackett-Luce policy at temperature T,
 * with the conditional log-probability of every pick.  Three calls, cut at the two points where item shards exchange; the unsharded path
 * makes the same three calls without the exchanges.  inv_temp = (float)(1 / T), formed by the caller.
 * ltg_topk_sample: the draw is Gumbel-top-k.  Eligible = not a fold-in item of tr and not in excl_id [n_rows][f_in] (a fixed head as
 * ltg_topk / ltg_topk_merge wrote it: GLOBAL ids; ids outside the slab and padding are skipped and index nothing; NULL with f_in = 0).
 * key = s * inv_temp + g, one fp32 multiply and one fp32 add, never contracted; g = -logf(-logf(u)), u = the counter RNG's uniform at
 * (cfg->seed, stream 8, draw, (row_lo + row) * n_items_global + global id) -- a pure function of the seed, the draw, the GLOBAL row and the
 * GLOBAL id (n_items_global = cfg->n_items_global, or cfg->n_items where that is 0).  u == 0 gives key -inf: eligible, last.  g_noise
 * (optional) [n_rows][cfg->n_items]: injected Gumbel values aligned with the slab's columns; the RNG is then not called.  key_out / id_out
 * [n_rows][k]: this slab's k largest keys in ltg_topk's list format with the key in the score's place (key descending, equal keys lower
 * GLOBAL id first, -0.0 == +0.0, padding id -1 / key -inf), so per-slab outputs go straight into ltg_topk_merge, and the merge of the slabs
 * of a row equals the call on the whole row bit for bit.  One workgroup per row; the noise is recomputed in every pass, and no [n_rows][n_items]
 * array is written.  ltg_topk's limits: 1 <= k <= 1024, n_items per slab <= 360 448.  NaN keys are outside the contract.
 * ltg_topk_sample_mass: id_in [n_rows][k] = the FINAL picks (GLOBAL ids, after the merge).  Over this slab: score_out [n_rows][k] = the raw
 * logit of every pick the slab owns, -inf elsewhere; max_out [n_rows] = the largest eligible logit (picks included; -inf if there is none);
 * rest_out [n_rows] = the sum over the eligible items that were NOT picked of exp((s - max_out) * inv_temp), -inf logits adding nothing.  Fixed
 * per-thread stride and a fixed reduction tree: bit-identical from run to run.  Across slabs the caller forms M = max of max_out, rest = sum of
 * rest_out * exp((max_out - M) * inv_temp), score = max of score_out.
 * ltg_topk_sample_finish: logp_out [n_rows][k], logp_j = x_j - log(rest + sum_{m >= j} exp(x_m)) with x_m = (score_m - M) * inv_temp: the log of
 * the conditional probability of pick j given the earlier ones, from positive terms only.  An entry with score -inf (padding) gets 0.0.  One wave
 * per row.  Outside the contract: logp where x_j < -80 for a pick, or where every eligible logit is -inf.
 * No floating-point atomics anywhere.  LTG_EINVAL before any HIP call: a NULL output or input (tr, excl_id with f_in = 0, g_noise and stream
 * excepted), k outside [1, 1024], f_in < 0, f_in > 0 with excl_id NULL, inv_temp not finite or <= 0, row_lo < 0, item_lo < 0, and whatever
 * ltg_topk refuses; n_rows = 0 returns LTG_OK and launches nothing. */
int ltg_topk_sample(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t row_lo, int32_t k, float inv_temp,
                    uint64_t draw, const int32_t* excl_id, int32_t f_in, const float* g_noise, float* key_out, int32_t* id_out,
                    ltg_stream stream);
int ltg_topk_sample_mass(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, float inv_temp,
                         const int32_t* excl_id, int32_t f_in, const int32_t* id_in, float* score_out, float* max_out, float* rest_out,
                         ltg_stream stream);
int ltg_topk_sample_finish(int32_t n_rows, int32_t k, const float* score, const float* M, const float* rest, float inv_temp, float* logp_out,
                           ltg_stream stream);

/* Replay of an exploration log (additive, ABI v14): off-policy estimates for OTHER Plackett-Luce policies from lists that were
 * served and logged with their propensities.  A target policy is (T_p, F'): up to LTG_REPLAY_MAX_POLICIES temperatures per call, which share
 * the fixed head F'.  inv_temp is a HOST array [n_pol] of (float)(1 / T_p); it is read during the call and travels as a kernel argument.
 * ltg_list_mass: id_in [n_rows][k] = the LOGGED lists (GLOBAL ids, -1 = padding; the ids of a row are distinct and in [0, n_items_global):
 * the caller's contract, not checked here).  Not eligible under the target = a fold-in item of tr, or in excl_id [n_rows][f_in] (the
 * target's plain top-F' as ltg_topk / ltg_topk_merge wrote it; NULL with f_in = 0).  Over this slab, for every slot j >= f_in whose id the slab
 * owns: state_out [n_rows][k] (int32) = 1 if the item is eligible, 2 if not; score_out [n_rows][k] = its raw logit if the state is 1, -inf
 * otherwise.  Slots j < f_in, padding and ids the slab does not own get state 0 and score -inf.  max_out [n_rows] = the largest eligible
 * logit, as in ltg_topk_sample_mass.  rest_out [n_pol][n_rows] = the sum over the eligible items that are not a state-1 entry of
 * exp((s - max_out) * inv_temp[p]), -inf logits adding nothing: an entry without support takes no mass out.  All n_pol sums come from one
 * walk over the row (two passes: maximum, then sums; fp32 accumulation with ltg_topk_sample_mass's term, stride and tree), so n_pol = 8 in
 * one call equals eight calls at n_pol = 1 bit for bit, and every call is bit-identical from run to run.  No [n_rows][n_items] array is
 * written.  Across slabs the caller forms M = max of max_out, rest_p = sum of rest_out[p] * exp((max_out - M) * inv_temp[p]), score = max
 * of score_out, state = max of state_out.
 * ltg_replay_rows: takes the merged values of the whole catalogue (score, state [n_rows][k], M [n_rows], rest [n_pol][n_rows]), the target's
 * head head_id [n_rows][f_in] (NULL with f_in = 0), the log (id_in, logp0 <= 0, reward, each [n_rows][k]) and the group labels item_group
 * (uint8 per GLOBAL item id, a label >= n_groups is in no group; 1 <= n_groups <= 8 as ltg_topk_metrics takes them).  Everything below in
 * fp64.  A real slot j < f_in is supported iff id_in[j] == head_id[j], with logp1 = 0; a real slot j >= f_in is supported iff its state is 1,
 * with logp1_j = x_j - log(rest_p + sum over the supported m >= j, m >= f_in of exp(x_m)), x_m = (score_m - M) * inv_temp[p].  d_j = logp1_j -
 * logp0_j, c_j = the sum of d_m over the real slots m <= j, w_j = exp(min(c_j, log(clip))) before the first unsupported slot and 0 from it on;
 * padding is skipped.  row_out [n_rows][n_pol][n_groups + 1][2] = (A, B) = (sum_j w_j reward_j, sum_j w_j) over the slots whose item is
 * in group g, slot n_groups = all items; w_out [n_rows][n_pol] = w at the last real slot (0 if any slot is unsupported; exp(min(0,
 * log(clip))) for a row of padding); first_bad_out [n_rows][n_pol] = the first unsupported slot, k if none; logp1_out (optional)
 * [n_pol][n_rows][k] = logp1 as float, 0.0 for padding and a supported head slot, -inf for an unsupported slot.  One wave per row, no
 * workspace, no atomics: bit-identical from run to run.  logp1 where x_j < -80 is outside the contract, as for ltg_topk_sample_finish.
 * Both calls return LTG_EINVAL before any HIP call for: a NULL required pointer (tr, excl_id / head_id with f_in = 0, logp1_out and stream
 * excepted), k outside [1, 1024], n_pol outside [1, 8], f_in < 0, f_in >= k, f_in > 0 without the head, an inv_temp that is not finite or
 * <= 0, clip not finite or <= 0, n_groups outside [1, 8], n_items_global <= 0, and whatever ltg_topk refuses; n_rows = 0 returns LTG_OK and
 * launches nothing. */
#define LTG_REPLAY_MAX_POLICIES 8
int ltg_list_mass(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, const int32_t* id_in, int32_t f_in,
                  const int32_t* excl_id, int32_t n_pol, const float* inv_temp, float* score_out, int32_t* state_out, float* max_out,
                  float* rest_out, ltg_stream stream);
int ltg_replay_rows(int32_t n_rows, int32_t k, int32_t n_pol, const float* inv_temp, int32_t f_in, const int32_t* head_id, const int32_t* id_in,
                    const float* logp0, const float* reward, const float* score, const int32_t* state, const float* M, const float* rest,
                    const uint8_t* item_group, int32_t n_groups, int32_t n_items_global, double clip, double* row_out, double* w_out,
                    int32_t* first_bad_out, float* logp1_out, ltg_stream stream);

/* Posterior-aware scores (additive, ABI v14): lists ranked by the VAE's own uncertainty.  S = n_samples in {1, 4, 8, 16, 32}
 * samples of z are drawn from the encoder's posterior of every user row, pushed through the decoder, and reduced per (user, item) to
 * mean, std (population, two-pass) and score = fmaf(beta, std, mean): beta = 0 the posterior mean, beta > 0 UCB, beta < 0 LCB, S = 1 one
 * Thompson draw (std = 0, score = the sample's logit; beta must be 0).  The [n_rows * S][n_items] logits are never written anywhere.
 * ltg_posterior_ld: bf16 elements per image row = h_enc rounded up to 32 (608 at 600); 0 for a cfg the calls refuse.
 * ltg_posterior_image_bytes: the size of the image of n_rows rows; 0 for what the calls refuse.
 * ltg_posterior_h2: sample s of row r: z = mu + expf(0.5f * logvar) * e from mulv [n_rows][2Z] (mu | logvar, as ltg_gen_acts.mulv holds
 * them); e = eps[r][s][j] if eps is given, else the counter RNG's normal at (cfg->seed, stream 9, draw, ((row_lo + r) * S + s) * Z + j) -- a
 * pure function of the seed, the draw, the GLOBAL row, the sample and the column, whatever chunk, row block or rank holds the row.  Then
 * h2 = tanhf(z . W_p0 + b_p0) in fp32 (gen->p[2], gen->p[6]; one fmaf chain over Z in ascending order), rounded to nearest even into bf16
 * at image row r * S + s; columns [h_enc, ld) are written as zeros.  z_out (optional) [n_rows * S][Z] receives z.  One kernel.
 * ltg_posterior_scores: l[r][s][i] = image[r * S + s] . bf16(W_p1t[i]) + b_p1[i] on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  The
 * operands are bf16 WHATEVER cfg->precision is.  W_p1t comes from gen->wp1t_bf16 when present (and h_enc <= 608), otherwise gen->p[3] is
 * rounded on the fly: the same operand values, the same result bit for bit.  score_out [n_rows][cfg->n_items] = fmaf(beta, std, mean);
 * spread_out (optional, same shape) = std.  An element's bits depend on no tile, workgroup, segment or slab: one MFMA chain over K in
 * ascending order and one balanced tree over the sample index, no atomics; the slab [lo, hi) of a catalogue gives the whole call's columns
 * bit for bit, and every call is bit-identical from run to run.  image must be 16-byte aligned.
 * ltg_posterior_entries: mean_out / std_out [n_rows][k] = the same mean and std for the entries id_in [n_rows][k] (GLOBAL ids) gathered from
 * the same image, one wave per entry (another K order: equal to ltg_posterior_scores up to fp32 rounding).  An id outside the slab
 * [cfg->item_lo, cfg->item_lo + cfg->n_items) and padding (-1) get 0.0f in both, so item shards add up under a sum all-reduce.
 * ltg_row_lse: lse_out [n_rows] = the log-sum-exp of every row of logits [n_rows][cfg->n_items], the kernel ltg_vae_forward runs.
 * All return LTG_EINVAL before any HIP call for: a NULL required pointer (eps, z_out, spread_out and stream excepted), n_samples outside the
 * set, beta not finite, n_samples == 1 with beta != 0, row_lo < 0, n_rows < 0, n_rows * n_samples >= 2^31, k outside [1, 1024], an image
 * that is not 16-byte aligned, n_samples * z_dim * 4 > 64 KiB, a bad cfg.  n_rows == 0 returns LTG_OK and launches nothing. */
#define LTG_POST_MAX_SAMPLES 32
int32_t ltg_posterior_ld(const ltg_config* cfg);
size_t ltg_posterior_image_bytes(const ltg_config* cfg, int32_t n_rows, int32_t n_samples);
int ltg_posterior_h2(const ltg_config* cfg, const ltg_gen_state* gen, const float* mulv, int32_t n_rows, int32_t row_lo, int32_t n_samples,
                     uint64_t draw, const float* eps, uint16_t* image_out, float* z_out, ltg_stream stream);
int ltg_posterior_scores(const ltg_config* cfg, const ltg_gen_state* gen, const uint16_t* image, int32_t n_rows, int32_t n_samples, float beta,
                         float* score_out, float* spread_out, ltg_stream stream);
int ltg_posterior_entries(const ltg_config* cfg, const ltg_gen_state* gen, const uint16_t* image, int32_t n_rows, int32_t n_samples,
                          const int32_t* id_in, int32_t k, float* mean_out, float* std_out, ltg_stream stream);
int ltg_row_lse(const ltg_config* cfg, const float* logits, int32_t n_rows, float* lse_out, ltg_stream stream);

/* Verification helper of the LTG_PREC_FP8 mode: out[i] = the value the fp8 GEMM operands carry for in[i]
 * (clamp to +-448, round to nearest-even OCP e4m3) -- lets a test pin its CPU model of the rounding to the hardware. */
int ltg_fp8_roundtrip(const float* in, float* out, int32_t n, ltg_stream stream);
/* verification helper (ABI v14): the three bf16 terms (hi, mid, lo as fp32 values) into which the d_arith = BF16X6 loaders split every fp32 operand:
 * out[3 i + t] for in[i], n % 4 == 0.  The claim the tests pin: hi + mid + lo == in exactly, each term the round-to-nearest bf16 of its residual. */
int ltg_debug_split(const float* in, float* out, int32_t n, ltg_stream stream);
/* Verification helper: C[M][N] = A[M][K] . B[K][N] (row-major fp32) through the MFMA block template every GEMM-shaped
 * kernel is an instance of; mode 0 = fp32 operands, 1 = bf16, 2 = e4m3 with scale 2^4 on both operands. */
int ltg_debug_gemm(int32_t mode, int32_t M, int32_t N, int32_t K, const float* A, const float* B, float* C, ltg_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* LTG_H */
