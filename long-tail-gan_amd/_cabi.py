"""ctypes binding of the C ABI declared in include/ltg.h (libltg_hip.so).

There is deliberately NO fallback: if the HIP library is missing or a symbol is absent the import
of the product path fails loudly (the oracle under oracle/ is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LTG_HIP_LIB") or os.path.join(_HERE, "libltg_hip.so")   # LTG_HIP_LIB: another build of the SAME library (A/B timing)

LTG_PREC_BF16 = 0
LTG_PREC_FP32 = 1
LTG_PREC_FP8 = 2
LTG_DARITH_FP32, LTG_DARITH_BF16X6, LTG_DARITH_BF16X4 = 0, 1, 2    # ltg_config.d_arith
LTG_ABI_VERSION = 14
LTG_PLAN_AHEAD, LTG_PLAN_SHADOW = 1, 2
LTG_Q0_HIST = 1024
LTG_SPACE = {"decoder": 0, "encoder": 1}     # ltg_item_pack
LTG_METRIC = {"cosine": 0, "dot": 1}
LTG_NBR_MAX_K = 256
LTG_PAIR_SIDE = {"popular": 0, "niche": 1}   # ltg_pair_pack
LTG_PAIR_MAX_K = 256                         # ltg_pair_companions: the longest companion list
LTG_CRITIC_MAX_TOP, LTG_GATE_MAX_C = 256, 256   # ltg_pair_critic: the entries scored per row; ltg_topk_gate: the longest candidate list
LTG_AUD_MAX_K = 256                       # ltg_item_audience: the longest audience list
LTG_DIV_MAX_C = 256                          # ltg_topk_diversify: the longest candidate list
LTG_WHY_MAX_TOP, LTG_WHY_MAX_R = 256, 8      # ltg_topk_explain: the entries explained per row, the history items per entry
LTG_CAL_MAX_CLASSES = 9                      # ltg_hist_groups / ltg_topk_calibrate: n_groups + 1 classes at the most
LTG_CAP_STATE, LTG_CAP_MAX_ROUNDS = 8, 64    # ltg_cap_*: the int32 words of the state block, the rounds one call enqueues at the most
LTG_SHARE_STATE = 8                          # ltg_topk_share: the int32 words of its state block
LTG_FLOOR_STATE, LTG_FLOOR_MAX_ROUNDS = 8, 64  # ltg_floor_*: the int32 words of the state block, the rounds one call enqueues at the most

ERRORS = {0: "LTG_OK", -1: "LTG_EINVAL", -2: "LTG_EWORKSPACE", -3: "LTG_ELAUNCH"}

vp = C.c_void_p


class ltg_config(C.Structure):
    _fields_ = [("n_items", C.c_int32), ("h_enc", C.c_int32), ("z_dim", C.c_int32), ("d_feat", C.c_int32),
                ("d_h0", C.c_int32), ("d_h1", C.c_int32), ("d_h2", C.c_int32), ("d_h3", C.c_int32),
                ("precision", C.c_int32), ("tuning", C.c_int32), ("item_lo", C.c_int32), ("n_items_global", C.c_int32),
                ("d_precision", C.c_int32), ("d_arith", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float),
                ("seed", C.c_uint64)]


class ltg_gen_state(C.Structure):
    _fields_ = [("p", vp * 8), ("m", vp * 8), ("v", vp * 8), ("wp1t_bf16", vp),
                ("q0_last", vp), ("q0_lr_hist", vp), ("q0_ord", C.c_int32), ("q0_period", C.c_int32)]   # optional lazy Adam clock of W_q0


class ltg_disc_state(C.Structure):
    _fields_ = [("emb", vp), ("p", vp * 8), ("m", vp * 8), ("v", vp * 8),
                ("emb_fp8", vp), ("w1t_fp8", vp), ("w2t_fp8", vp), ("w3t_fp8", vp), ("w3_fp8", vp)]      # optional e4m3 operand shadows


class ltg_batch(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_unique", C.c_int32), ("indptr", vp), ("indices", vp), ("values", vp),
                ("slot", vp), ("uptr", vp), ("rowidx", vp), ("csr_pos", vp), ("row_norm2", vp), ("uitem", vp)]


class ltg_gen_acts(C.Structure):
    _fields_ = [("h1", vp), ("mulv", vp), ("z", vp), ("h2", vp), ("logits", vp), ("lse", vp), ("kl_rows", vp),
                ("row_scale", vp)]


class ltg_probe(C.Structure):
    _fields_ = [("kernel_id", C.c_int32), ("reserved0", C.c_int32), ("ev_start", vp), ("ev_stop", vp)]


KERNEL_IDS = {"enc0_fwd": 1, "enc1": 2, "dec0": 3, "dec1_fwd": 4, "d_l1": 5, "d_l2": 6, "d_bwd1": 7, "d_bwd2": 8, "d_adam": 9,
              "dh2": 10, "dec1_bwd_adam": 11, "enc0_bwd_adam": 12, "dz": 13, "dh1": 14, "wgrad_p0": 15, "wgrad_q1": 16,
              "row_dlogits": 17, "enc0_grad": 18, "g_tail": 19, "exch_h1": 20, "exch_rowpart": 21, "exch_dh2": 22}


class ltg_fwd_opts(C.Structure):
    _fields_ = [("keep_prob", C.c_float), ("is_training", C.c_float), ("rng_step", C.c_uint64), ("drop_keep", vp),
                ("eps", vp), ("probe", C.POINTER(ltg_probe)), ("rows_per_step", C.c_int32), ("reserved0", C.c_int32)]


class ltg_pairs(C.Structure):
    _fields_ = [("n", C.c_int32), ("reserved0", C.c_int32), ("pop", vp), ("niche", vp), ("row", vp)]


class ltg_d_opts(C.Structure):
    _fields_ = [("keep_prob", C.c_float), ("adam_t", C.c_int32), ("rng_step", C.c_uint64), ("drop_real", vp * 3),
                ("drop_fake", vp * 3), ("probe", C.POINTER(ltg_probe)), ("aux_stream", vp), ("sync", vp), ("seq", C.c_uint32), ("reserved0", C.c_int32)]


class ltg_g_opts(C.Structure):
    _fields_ = [("fwd", ltg_fwd_opts), ("anneal", C.c_float), ("gan_lambda", C.c_float), ("d_keep_prob", C.c_float),
                ("adam_t", C.c_int32), ("d_rng_step", C.c_uint64), ("drop_fake", vp * 3), ("cnt", vp), ("probe", C.POINTER(ltg_probe)),
                ("aux_stream", vp), ("ev_fork", vp), ("ev_join", vp), ("dec1_done", C.c_int32), ("fake_done", C.c_int32), ("ev_sweep", vp), ("y_pre", vp)]


class ltg_sample_inputs(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("max_cand", C.c_int32), ("cand_ptr", vp), ("cand_idx", vp), ("pop_ptr", vp),
                ("pop_idx", vp), ("n_sample", vp), ("slot_ptr", vp), ("valid_item", vp), ("rng_step", C.c_uint64),
                ("u_gumbel", vp), ("u_pick", vp), ("cand_logit", vp), ("rows_per_step", C.c_int32), ("reserved0", C.c_int32)]


# the two collective entry points a caller hands to ltg_g_step_sharded: the signatures of ncclAllReduce / ncclAllGather (rccl.h:611, :678)
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, C.c_int, vp, vp)
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, vp, vp)
LTG_NCCL_FLOAT32, LTG_NCCL_SUM = 7, 0
LTG_PIPE_NO_DEC1_FORK, LTG_PIPE_NO_SLICE_FORK, LTG_PIPE_WIDE_GRAD, LTG_PIPE_EVENTS, LTG_PIPE_SLICE_IN_TOUCH, LTG_PIPE_TAIL_OWN = 1, 2, 8, 16, 32, 128


class ltg_comm(C.Structure):
    _fields_ = [("comm", vp), ("n_ranks", C.c_int32), ("rank", C.c_int32), ("all_reduce", vp), ("all_gather", vp)]


class ltg_pipe(C.Structure):
    _fields_ = [("side_stream", vp), ("ev_fork", vp), ("ev_dec1", vp), ("ev_tail", vp),
                ("h1pre", vp), ("rowpart_all", vp), ("dh2", vp), ("flags", C.c_int32), ("seq", C.c_uint32), ("sync", vp), ("tail_stream", vp),
                ("q0_mark", vp), ("next_uitem", vp), ("next_nu", C.c_int32), ("caught_up", C.c_int32), ("shadow_out", vp)]


# kernel routes (include/ltg.h: ltg_g_route / ltg_d_route); the enumerators in the header's order
LTG_ENC0_GENERIC, LTG_ENC0_FAST = 0, 1
LTG_MID_DENSE, LTG_MID_FAST = 0, 1
LTG_DEC_TILE, LTG_DEC_SMALL, LTG_DEC_STREAM1, LTG_DEC_STREAM2 = 0, 1, 2, 3
LTG_STATS_ROW, LTG_STATS_SEGMENT, LTG_STATS_EPILOGUE = 0, 1, 2
LTG_LOSS_GENERIC, LTG_LOSS_COMBINE, LTG_LOSS_ROW = 0, 1, 2
LTG_DH2_PARTIAL, LTG_DH2_SMALL, LTG_DH2_STREAM = 0, 1, 2
LTG_DW_TILE, LTG_DW_TAIL_JOB, LTG_DW_STREAM = 0, 1, 2
LTG_Q0_DENSE, LTG_Q0_SWEEP, LTG_Q0_LAZY = 0, 1, 2
LTG_D_GENERIC, LTG_D_TOWER, LTG_D_STAGED_FWD, LTG_D_FAST, LTG_D_FP8_OPFMT, LTG_D_FP8_STAGED, LTG_D_FP8_REG = 0, 1, 2, 3, 4, 5, 6
LTG_D_ADAM_TENSORS, LTG_D_ADAM_FLAT, LTG_D_ADAM_FP8 = 0, 1, 2


class ltg_g_route_info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("enc0", "small", "mid", "mid_vec", "dec", "dec_tile", "stats", "seg_pass", "loss", "dlog_bf16", "dh2", "dh2_tile",
                                         "dh2_chunk", "dh2_nsplit", "dw", "dw_tile", "dw_ragged", "q0", "q0_own_launch", "grad_rows", "sharded_ok")]


class ltg_d_route_info(C.Structure):
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("tile", C.c_int32 * 4), ("spl", C.c_int32 * 4), ("adam", C.c_int32), ("fork", C.c_int32)]


# the pipe's schedule (include/ltg.h: ltg_g_pipe_plan) and the device words of ltg_pipe.sync / ltg_d_opts.sync (enum ltg_word)
LTG_HAND_ORDER, LTG_HAND_EVENTS, LTG_HAND_WORDS = 0, 1, 2
LTG_SLICE_OWN_END, LTG_SLICE_IN_TOUCH, LTG_SLICE_SIDE = 0, 1, 2
(LTG_WORD_DH2_DONE, LTG_WORD_H2_READ, LTG_WORD_POISON, LTG_WORD_PROBE, LTG_WORD_CATCHUP, LTG_WORD_SLICE_DONE, LTG_WORD_UPDATE_END, LTG_WORD_H2_COUNT,
 LTG_WORD_DH1_DONE, LTG_WORD_TAIL_END) = 0, 1, 2, 3, 5, 6, 7, 8, 9, 10
LTG_WORD_D_FWD_DONE, LTG_WORD_D_JOBS_DONE = 0, 1


class ltg_pipe_plan_info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("handover", "slice", "ahead", "shadow", "tail_own", "h2_early", "grad_rows", "poisonable")]


LTG_ONESHOT_MAX_RANKS = 16


class ltg_oneshot(C.Structure):
    _fields_ = [("n_ranks", C.c_int32), ("rank", C.c_int32), ("seq", C.c_uint32), ("limit_ms", C.c_uint32), ("max_floats", C.c_size_t),
                ("stage", vp * LTG_ONESHOT_MAX_RANKS)]


# every symbol include/ltg.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ltg_oneshot_stage_bytes": (C.c_size_t, [C.c_int32, C.c_size_t]),
    "ltg_oneshot_expired_offset": (C.c_size_t, [C.c_int32]),
    "ltg_oneshot_all_reduce": (C.c_int, [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, vp]),
    "ltg_oneshot_all_gather": (C.c_int, [vp, vp, C.c_size_t, C.c_int, vp, vp]),
    "ltg_g_step_sharded_ok": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.c_int32]),
    "ltg_g_step_sharded_plan": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_batch), C.POINTER(ltg_pipe)]),
    "ltg_g_pipe_plan": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_batch), C.POINTER(ltg_pipe), C.POINTER(ltg_pipe_plan_info)]),
    "ltg_g_route": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.c_int32, C.POINTER(ltg_g_route_info)]),
    "ltg_d_route": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), C.c_int32, C.c_int32, C.c_int32, C.POINTER(ltg_d_route_info)]),
    "ltg_g_step_sharded": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_disc_state), C.POINTER(ltg_batch),
                                     C.POINTER(ltg_pairs), C.POINTER(ltg_g_opts), C.POINTER(ltg_gen_acts), C.POINTER(ltg_comm),
                                     C.POINTER(ltg_pipe), vp, vp, C.c_size_t, vp]),
    "ltg_g_pipe_join": (C.c_int, [C.POINTER(ltg_pipe), vp]),
    "ltg_g_pipe_probe": (C.c_int, [C.POINTER(ltg_pipe), vp]),
    "ltg_abi_version": (C.c_int32, []),
    "ltg_workspace_bytes": (C.c_size_t, [C.POINTER(ltg_config), C.c_int32, C.c_int32]),
    "ltg_vae_forward": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_batch),
                                  C.POINTER(ltg_fwd_opts), C.POINTER(ltg_gen_acts), vp, vp, C.c_size_t, vp]),
    "ltg_sample_pairs": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_sample_inputs), vp, vp, vp, vp, vp, vp]),
    "ltg_d_step": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), C.POINTER(ltg_pairs),
                             C.POINTER(ltg_pairs), C.POINTER(ltg_d_opts), vp, vp, C.c_size_t, vp]),
    "ltg_d_grad_floats": (C.c_size_t, [C.POINTER(ltg_config)]),
    "ltg_d_grad": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), C.POINTER(ltg_pairs), C.POINTER(ltg_pairs), C.c_int32,
                             C.c_int32, C.POINTER(ltg_d_opts), vp, vp, C.c_size_t, vp]),
    "ltg_d_apply": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), vp, C.c_int32, vp, vp]),
    "ltg_g_bwd_dec1": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_batch), C.POINTER(ltg_pairs),
                                 C.POINTER(ltg_g_opts), C.POINTER(ltg_gen_acts), vp, C.c_size_t, vp]),
    "ltg_g_step": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_disc_state),
                             C.POINTER(ltg_batch), C.POINTER(ltg_pairs), C.POINTER(ltg_g_opts),
                             C.POINTER(ltg_gen_acts), vp, vp, C.c_size_t, vp]),
    "ltg_g_fwd_enc": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_batch), C.POINTER(ltg_fwd_opts),
                                C.POINTER(ltg_gen_acts), vp]),
    "ltg_g_fwd_rest": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_batch), C.POINTER(ltg_pairs),
                                 C.POINTER(ltg_fwd_opts), C.POINTER(ltg_gen_acts), vp, vp, C.c_size_t, vp]),
    "ltg_rowstats_combine": (C.c_int, [C.POINTER(ltg_config), vp, C.c_int32, C.c_int32, vp, vp, C.c_size_t, vp]),
    "ltg_g_bwd_dec": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_disc_state), C.POINTER(ltg_batch),
                                C.POINTER(ltg_pairs), C.POINTER(ltg_g_opts), C.POINTER(ltg_gen_acts), vp, C.c_int32, vp, vp, vp,
                                C.c_size_t, vp]),
    "ltg_g_bwd_rest": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.POINTER(ltg_batch), C.POINTER(ltg_pairs),
                                 C.POINTER(ltg_g_opts), C.POINTER(ltg_gen_acts), vp, vp, C.c_size_t, vp]),
    "ltg_gather_cand_logits": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_sample_inputs), vp, vp, vp]),
    "ltg_refresh_shadow": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), vp]),
    "ltg_forward_scratch_bytes": (C.c_size_t, [C.POINTER(ltg_config), C.c_int32]),
    "ltg_g_fake_tower": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), C.POINTER(ltg_pairs), C.POINTER(ltg_g_opts), C.c_int32, vp, C.c_size_t, vp]),
    "ltg_fake_tower_batched": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), C.POINTER(ltg_pairs), vp, vp, vp, C.c_float, vp, vp,
                                        C.c_size_t, vp]),
    "ltg_g_flush": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), vp]),
    "ltg_refresh_d_shadow": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), vp]),
    "ltg_rank_metrics": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.POINTER(ltg_batch), C.c_int32,
                                   C.c_int32, C.c_int32, vp, vp]),
    "ltg_rank_scores": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.POINTER(ltg_batch), vp, vp]),
    "ltg_rank_counts": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.POINTER(ltg_batch), vp, vp, vp]),
    "ltg_rank_finish": (C.c_int, [C.POINTER(ltg_batch), vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
    "ltg_topk": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.c_int32, C.c_int32, vp, vp, vp]),
    "ltg_topk_merge": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, vp, vp]),
    "ltg_topk_groups": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.c_int32, C.c_int32, vp, C.c_int32, C.c_uint32, vp, vp, vp]),
    "ltg_topk_quota": (C.c_int, [C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, C.POINTER(C.c_int32), C.c_int32, vp, vp, vp]),
    "ltg_topk_metrics": (C.c_int, [vp, C.c_int32, C.c_int32, C.POINTER(ltg_batch), vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, vp, vp, vp]),
    "ltg_item_pack": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), C.c_int32, C.c_int32, vp, vp]),
    "ltg_item_neighbors_ws_bytes": (C.c_size_t, [C.POINTER(ltg_config), C.c_int32, C.c_int32]),
    "ltg_item_neighbors": (C.c_int, [C.POINTER(ltg_config), vp, vp, vp, C.c_int32, vp, C.c_uint32, C.c_int32, vp, vp, vp, C.c_size_t, vp]),
    "ltg_pair_ld": (C.c_int32, [C.POINTER(ltg_config)]),
    "ltg_pair_pack": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), C.c_int32, vp, C.c_int32, vp, vp]),
    "ltg_pair_companions_ws_bytes": (C.c_size_t, [C.POINTER(ltg_config), C.c_int32, C.c_int32, C.c_int32]),
    "ltg_pair_companions": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp,
                                      vp, C.c_size_t, vp]),
    "ltg_pair_critic": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_disc_state), vp, C.c_int32, vp, C.c_int32, vp, vp, C.c_int32,
                                  C.POINTER(ltg_batch), C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp]),
    "ltg_critic_finish": (C.c_int, [C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]),
    "ltg_topk_gate": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_int32, vp, vp, vp, vp]),
    "ltg_topk_sample": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64, vp,
                                  C.c_int32, vp, vp, vp, vp]),
    "ltg_topk_sample_mass": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.c_int32, C.c_int32, C.c_float, vp, C.c_int32, vp, vp,
                                       vp, vp, vp]),
    "ltg_topk_sample_finish": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, C.c_float, vp, vp]),
    "ltg_list_mass": (C.c_int, [C.POINTER(ltg_config), vp, C.POINTER(ltg_batch), C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_int32,
                                C.POINTER(C.c_float), vp, vp, vp, vp, vp]),
    "ltg_replay_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                  C.c_int32, C.c_int32, C.c_double, vp, vp, vp, vp, vp]),
    "ltg_posterior_ld": (C.c_int32, [C.POINTER(ltg_config)]),
    "ltg_posterior_image_bytes": (C.c_size_t, [C.POINTER(ltg_config), C.c_int32, C.c_int32]),
    "ltg_posterior_h2": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp,
                                   vp]),
    "ltg_posterior_scores": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), vp, C.c_int32, C.c_int32, C.c_float, vp, vp, vp]),
    "ltg_posterior_entries": (C.c_int, [C.POINTER(ltg_config), C.POINTER(ltg_gen_state), vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, vp]),
    "ltg_row_lse": (C.c_int, [C.POINTER(ltg_config), vp, C.c_int32, vp, vp]),
    "ltg_topk_diversify": (C.c_int, [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_float, C.c_int32, vp, vp, vp, vp]),
    "ltg_topk_explain": (C.c_int, [vp, C.c_int32, C.c_int32, C.POINTER(ltg_batch), C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp,
                                   vp, vp]),
    "ltg_hist_groups": (C.c_int, [C.POINTER(ltg_batch), C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp]),
    "ltg_topk_calibrate": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, C.POINTER(C.c_int32), C.c_int32, vp, C.c_float, C.c_int32, vp, vp,
                                     vp, vp]),
    "ltg_cap_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "ltg_cap_index": (C.c_int, [C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, C.c_size_t, vp]),
    "ltg_cap_rounds": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_size_t, vp]),
    "ltg_cap_finish": (C.c_int, [C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_size_t, vp]),
    "ltg_floor_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "ltg_floor_index": (C.c_int, [C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, C.c_size_t, vp]),
    "ltg_floor_rounds": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_size_t, vp]),
    "ltg_floor_finish": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_size_t,
                                   vp]),
    "ltg_share_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "ltg_topk_share": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, C.c_int64, vp, vp, vp, vp, C.c_size_t, vp]),
    "ltg_item_audience_ws_bytes": (C.c_size_t, [C.POINTER(ltg_config), C.c_int32, C.c_int32, C.c_int32]),
    "ltg_item_audience": (C.c_int, [C.POINTER(ltg_config), vp, vp, C.POINTER(ltg_batch), C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp,
                                    vp, C.c_size_t, vp]),
    "ltg_fp8_roundtrip": (C.c_int, [vp, vp, C.c_int32, vp]),
    "ltg_debug_split": (C.c_int, [vp, vp, C.c_int32, vp]),
    "ltg_debug_gemm": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]),
}

_lib = None


class LtgError(RuntimeError):
    pass


def load():
    """dlopen libltg_hip.so and bind every declared symbol.  Raises (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LtgError(
            "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or make -C long-tail-gan_amd/csrc).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    # LTG_HIP_LIB alone points at another build of THIS library: same strict checks.  LTG_AB_COMPAT=1 (scripts/ab_libs.sh, A/B timing
    # against an OLDER build): entry points it lacks stay unbound (Engine.sharded_step_ok is then False) and ABI 9 / 10 are accepted --
    # struct layouts only ever grew.
    ab = bool(os.environ.get("LTG_HIP_LIB")) and os.environ.get("LTG_AB_COMPAT", "0") == "1"
    for name, (res, args) in SYMBOLS.items():
        if ab and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    got = lib.ltg_abi_version()
    if got != LTG_ABI_VERSION and not (ab and 9 <= got < LTG_ABI_VERSION):
        raise LtgError("ABI version mismatch: library %d, binding %d" % (got, LTG_ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise LtgError("%s failed: %s (%d)" % (what, ERRORS.get(rc, "?"), rc))
