"""Host-side engine: owns every device buffer (torch is only the allocator / stream provider) and
drives the HIP kernels through the C ABI of include/ltg.h.

One Engine == the state the reference keeps inside its TF session (Codes/train.py:125-174):
generator variables (MultiVAE.py:188-230), discriminator variables (discriminator.py:14-41), ONE
AdamOptimizer whose step counter is shared by the D and the G updates (train.py:160-164, Q5).
"""
from __future__ import annotations

import ctypes as C
import os
import math

import numpy as np
import torch

from . import _cabi as cabi

G_NAMES = ["weight_q_0to1", "weight_q_1to2", "weight_p_0to1", "weight_p_1to2",
           "bias_q_1", "bias_q_2", "bias_p_1", "bias_p_2"]          # MultiVAE.py:196-197,216-217
D_NAMES = ["d_w1_1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3", "d_w4", "d_b4"]  # discriminator.py:23-41


def _ptr(t, off=0):
    if t is None:
        return None
    return t.data_ptr() + off * t.element_size()


def _pp(probe):
    return C.pointer(probe) if probe is not None else None


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise cabi.LtgError("no HIP device visible: the Long-Tail-GAN path has no CPU fallback")
    return torch.device(device)


def init_generator_host(I, H, Z, seed):
    """Default initialisers of MultiVAE._construct_weights (MultiVAE.py:188-230) in engine layout
    [W_q0 [I,H], W_q1 [H,2Z], W_p0 [Z,H], W_p1t [I,H], b_q0 [H], b_q1 [2Z], b_p0 [H], b_p1 [I]]: weights
    tf.contrib.layers.xavier_initializer = uniform(+-sqrt(6 / (fan_in + fan_out))) (:199-202, :219-221), biases
    tf.truncated_normal_initializer(stddev=0.001) = N(0, 0.001) re-drawn beyond 2 sigma (:204-207, :223-225).  The
    random STREAM is torch's (TF's cannot be reproduced without TF); the distributions are the reference's."""
    g = torch.Generator().manual_seed(seed)

    def xavier(fi, fo, shape):
        lim = math.sqrt(6.0 / (fi + fo))
        return (torch.rand(shape, generator=g) * 2 - 1) * lim

    def tn(shape, std):
        t = torch.empty(shape)
        torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std, generator=g)
        return t

    host = [xavier(I, H, (I, H)), xavier(H, 2 * Z, (H, 2 * Z)), xavier(Z, H, (Z, H)),
            xavier(H, I, (I, H)),                                # W_p1 [H, I] stored item-major [I][H]
            tn((H,), 1e-3), tn((2 * Z,), 1e-3), tn((H,), 1e-3), tn((I,), 1e-3)]
    return [t.numpy() for t in host]


def init_discriminator_host(feature_len, h_sizes, seed):
    """Default initialisers of discriminator.py:14-41: every matrix tf.truncated_normal(stddev=0.1) (the frozen embedding
    :14, w1 :23, w2 :28, w3 :36, w4 :40), every bias tf.zeros (:24, :29, :37, :41).
    -> (emb [F,h0], [w1 [h0,h1], b1, w2 [h0,h2], b2, w3 [h1+h2,h3], b3, w4 [h3], b4 [1]])."""
    g = torch.Generator().manual_seed(seed)

    def tn(shape):
        t = torch.empty(shape)
        torch.nn.init.trunc_normal_(t, 0.0, 0.1, -0.2, 0.2, generator=g)
        return t

    h0, h1, h2, h3 = h_sizes
    emb = tn((feature_len, h0))
    host = [tn((h0, h1)), torch.zeros(h1), tn((h0, h2)), torch.zeros(h2), tn((h1 + h2, h3)), torch.zeros(h3), tn((h3,)), torch.zeros(1)]
    return emb.numpy(), [t.numpy() for t in host]


class Acts:
    """Caller-owned activations of one generator forward (ltg_gen_acts)."""

    def __init__(self, rows, n_items, H, Z, device):
        f = dict(dtype=torch.float32, device=device)
        self.rows = rows
        self.h1 = torch.empty(rows, H, **f)
        self.mulv = torch.empty(rows, 2 * Z, **f)
        self.z = torch.empty(rows, Z, **f)
        self.h2 = torch.empty(rows, H, **f)
        self.logits = torch.empty(rows, n_items, **f)
        self.lse = torch.empty(rows, **f)
        self.kl_rows = torch.empty(rows, **f)
        self.row_scale = torch.empty(rows, **f)
        self.c = cabi.ltg_gen_acts(_ptr(self.h1), _ptr(self.mulv), _ptr(self.z), _ptr(self.h2), _ptr(self.logits),
                                   _ptr(self.lse), _ptr(self.kl_rows), _ptr(self.row_scale))


class CsrRows:
    """A range of user rows of a device-resident CSR matrix (ltg_batch), optionally with the transposed
    view (entries grouped by item) that the G step needs."""

    def __init__(self, indptr, indices, row_lo, row_hi, values=None, slot=None, uptr=None, rowidx=None, csr_pos=None,
                 n_unique=0, slot_off=0, uptr_off=0, ent_off=0, row_norm2=None, uitem=None, uitem_off=None):
        self.keep = (indptr, indices, values, slot, uptr, rowidx, csr_pos, row_norm2, uitem)
        self.n_rows = int(row_hi - row_lo)
        self.c = cabi.ltg_batch(self.n_rows, int(n_unique), _ptr(indptr, row_lo), _ptr(indices), _ptr(values),
                                _ptr(slot, slot_off), _ptr(uptr, uptr_off), _ptr(rowidx, ent_off), _ptr(csr_pos, ent_off),
                                _ptr(row_norm2, row_lo), _ptr(uitem, uptr_off if uitem_off is None else uitem_off))


class Pairs:
    def __init__(self, pop, niche, row=None, n=None, off=0):
        self.keep = (pop, niche, row)
        self.n = int(pop.numel() - off if n is None else n)
        self.c = cabi.ltg_pairs(self.n, 0, _ptr(pop, off), _ptr(niche, off), _ptr(row, off))


def _probe_streams(lib, probe_c, st, tries, another):
    """ltg_g_pipe_probe on the pair (st, the streams of probe_c): True when they run concurrently.  Otherwise another() swaps in a fresh
    stream (it gets the try's index) and the pair is tested again, `tries` times in all (HIP maps streams onto a few hardware queues)."""
    if not hasattr(lib, "ltg_g_pipe_probe"):      # (an older build under LTG_AB_COMPAT)
        return False
    for k in range(tries):
        rc = lib.ltg_g_pipe_probe(C.byref(probe_c()), st)
        if rc < 0:
            cabi.check(rc, "ltg_g_pipe_probe")
        if rc == 1:
            return True
        another(k)
    return False


class Pipe:
    """Caller-owned side stream, events and exchange buffers of ltg_g_step_sharded (include/ltg.h: ltg_pipe) for batches of up to
    `rows` rows exchanged between `n_ranks` ranks."""

    def __init__(self, engine, rows, n_ranks=1, flags=0):
        from ._hip import EventPair
        dev = engine.device
        self.side_stream = torch.cuda.Stream(dev)
        # the Adam tail's own stream: only with LTG_PIPE_TAIL_OWN (device-word hand-over; the default keeps the tail on the caller's stream)
        self.tail_stream = torch.cuda.Stream(dev) if (int(flags) & cabi.LTG_PIPE_TAIL_OWN) else None
        self._ev = (EventPair(timing=False), EventPair(timing=False))     # (fork, dec1), (tail, -)
        f = dict(dtype=torch.float32, device=dev)
        self.h1pre = torch.zeros(rows, engine.H, **f)
        self.rowpart_all = torch.zeros(n_ranks * rows * 5, **f)
        self.dh2 = torch.zeros(rows, engine.H, **f)
        self.sync = torch.zeros(16, dtype=torch.int32, device=dev)        # words of the device-side hand-overs (cabi.LTG_WORD_*); LTG_WORD_POISON = waits that gave up
        # catch-up ahead (include/ltg.h, ABI v13): "the current batch holds this row" marks; LTGAN_Q0_AHEAD=0: every call launches its own catch-up
        self.q0_mark = torch.zeros(engine.I, dtype=torch.int32, device=dev) if os.environ.get("LTGAN_Q0_AHEAD", "1") != "0" else None
        self.c = cabi.ltg_pipe(self.side_stream.cuda_stream, self._ev[0].start, self._ev[0].stop, self._ev[1].start, _ptr(self.h1pre),
                               _ptr(self.rowpart_all), _ptr(self.dh2), int(flags), 0, _ptr(self.sync),
                               self.tail_stream.cuda_stream if self.tail_stream is not None else None,
                               _ptr(self.q0_mark) if self.q0_mark is not None else None, None, 0, 0)
        # second shadow buffer of W_p1t (include/ltg.h: ltg_pipe.shadow_out): the weight update of a call writes it and the two are exchanged
        # after the call, so the update starts beside the dh2 product instead of behind it.  LTGAN_SHADOW_PINGPONG=0: in place.
        self.shadow = (torch.zeros_like(engine.g_shadow) if engine.g_shadow is not None and os.environ.get("LTGAN_SHADOW_PINGPONG", "1") != "0"
                       else None)
        self.c.shadow_out = _ptr(self.shadow) if self.shadow is not None else None
        self.ahead = None           # (uitem address, n_unique, q0_ord, seq) of the call whose rows the last call brought up to date
        self.ahead_calls = 0        # calls that launched no catch-up of their own
        self.probed_for = None      # the caller's stream the side stream was last tested against (Engine._pipe_ready)
        self.handover = None        # "device-words" | "events"
        engine._pipes.add(self)     # Engine.check_pipes(): nothing reads the model out behind a wait that gave up

    def new_side_stream(self):
        self.side_stream = torch.cuda.Stream(self.sync.device)
        self.c.side_stream = self.side_stream.cuda_stream

    def new_tail_stream(self, drop=False):
        self.tail_stream = None if drop else torch.cuda.Stream(self.sync.device)
        self.c.tail_stream = self.tail_stream.cuda_stream if self.tail_stream is not None else None

    def buffers(self):
        return [self.h1pre, self.rowpart_all, self.dh2]

    def expired_waits(self):
        """device-side waits of the hand-overs that gave up (must be 0; synchronises).  Non-zero = the pipe is POISONED: every kernel of the
        one-call step that writes h2 or the model returns at once (csrc: ltg_poisoned), so the model stays what it was when the wait expired."""
        return int(self.sync[cabi.LTG_WORD_POISON].item())

    def reset(self):
        """after a failed call: nothing in flight, every word zero, ordinals restart (a call that stopped between its gate launches would
        otherwise leave the next one waiting for words nobody sets)"""
        torch.cuda.synchronize(self.sync.device)
        self.sync.zero_()
        if self.q0_mark is not None:
            self.q0_mark.zero_()
        self.c.seq = 0
        self.ahead = None
        self.c.next_uitem, self.c.next_nu, self.c.caught_up = None, 0, 0
        torch.cuda.synchronize(self.sync.device)


class DFork:
    """Caller-owned aux stream and device words of ltg_d_step's fork (include/ltg.h: ltg_d_opts.aux_stream / sync / seq): jobs B / C of the
    discriminator's backward run beside the critical chain of the step.  The two streams must be concurrent (tested once per caller
    stream with ltg_g_pipe_probe; otherwise the step stays on one stream)."""

    def __init__(self, engine):
        self.stream = torch.cuda.Stream(engine.device)
        self.sync = torch.zeros(16, dtype=torch.int32, device=engine.device)
        self.seq = 0
        self.probed_for = None
        self.ok = False

    def ready(self, engine, st):
        if self.probed_for != st:
            def another(_):
                self.stream = torch.cuda.Stream(engine.device)
            self.ok = _probe_streams(engine.lib, lambda: cabi.ltg_pipe(self.stream.cuda_stream, None, None, None, None, None, None, 0, 0, _ptr(self.sync), None),
                                     st, 4, another)
            self.sync.zero_()
            self.seq = 0
            self.probed_for = st
        return self.ok

    def expired_waits(self):
        return int(self.sync[cabi.LTG_WORD_POISON].item())


# arithmetic of the fp32 discriminator's GEMMs (ltg_config.d_arith): the six-term bf16 split is fp32-accurate (every fp32-path parity test passes at
# its fp32 bound with it: tests/test_gpu_parity.py::test_d_step_parity) and 3.9 ms per epoch faster on Askubuntu_Sample (profiles/r6_ab_d_arith.txt);
# "fp32" = v_mfma_f32_16x16x4_f32, the exact fma chain, stays selectable
D_ARITH_DEFAULT = "bf16x6"


def _check_d_sizes(h_sizes):
    """the library refuses (LTG_EINVAL, before any launch) a discriminator with a layer of width < 1: say so at construction"""
    if len(h_sizes) != 4 or min(int(x) for x in h_sizes) < 1:
        raise ValueError("discriminator layer sizes must be four widths of at least 1, got %r" % (tuple(h_sizes),))


class Engine:
    def __init__(self, n_items, h_sizes=(100, 150, 250, 300), lr=1e-4, p_dims=None, feature_len=None,
                 precision="bf16", seed=98765, d_seed=0, device="cuda:0", beta1=0.9, beta2=0.999, eps=1e-8,
                 item_lo=0, item_hi=None, d_precision="fp32", lazy_q0=None, q0_period=32, d_arith=None):
        """n_items = GLOBAL item count; [item_lo, item_hi) = the slab this rank owns (default: everything).
        precision: operands of the three decoder GEMMs; d_precision: operands of the discriminator GEMMs
        ("fp32" = the reference's arithmetic, "bf16", "fp8" = BASELINE config 5).
        d_arith (d_precision "fp32", config.ini-sized layers): how the fp32 products are formed -- "fp32" = exact fp32 MFMA, "bf16x6" = the
        fp32-accurate six-term bf16 split on the bf16 matrix pipe, "bf16x4" = the four-term split (2^-17 per product, opt-in); None = D_ARITH_DEFAULT
        (environment LTGAN_D_ARITH overrides; include/ltg.h: ltg_config.d_arith).
        lazy_q0: lazy Adam clock of W_q0 (include/ltg.h, ltg_gen_state.q0_last; same results as the dense sweep).  None = on
        for item slabs of 8192 items or more.  Rows are brought up to date by every forward that reads them; `g_flush()`
        does it for all rows and runs after every G step unless a trainer holds `q0_defer` for the length of its phase."""
        _check_d_sizes(h_sizes)
        self.lib = cabi.load()
        import weakref
        self._pipes = weakref.WeakSet()                              # the Pipe objects created for this engine (check_pipes)
        self.check_on_flush = True                                   # False: a probe that times the host's issue rate (scripts/host_bound_probe.py)
        self.d_fork = os.environ.get("LTGAN_D_FORK", "1") != "0"     # ltg_d_step: jobs B / C of the backward on an aux stream (measurement switch)
        self._dfork = None
        self._pinned = None                                          # pin_stream()
        self.device = _require_gpu(device)
        torch.cuda.set_device(self.device)
        p_dims = p_dims or [200, 600, n_items]                       # generator.py:13
        assert p_dims[-1] == n_items
        self.I_global = n_items
        self.item_lo = int(item_lo)
        self.item_hi = int(n_items if item_hi is None else item_hi)
        self.sharded = (self.item_lo, self.item_hi) != (0, n_items)
        self.I, self.H, self.Z = self.item_hi - self.item_lo, p_dims[1], p_dims[0]   # self.I = LOCAL item count
        self.h0, self.h1, self.h2, self.h3 = h_sizes
        self.feature_len = feature_len or n_items
        self.precision = {"bf16": cabi.LTG_PREC_BF16, "fp32": cabi.LTG_PREC_FP32}[precision]
        self.d_precision = {"fp32": cabi.LTG_PREC_FP32, "bf16": cabi.LTG_PREC_BF16, "fp8": cabi.LTG_PREC_FP8}[d_precision]
        if d_arith is None:
            d_arith = os.environ.get("LTGAN_D_ARITH", D_ARITH_DEFAULT)
        self.d_arith = d_arith
        d_arith_code = {"fp32": cabi.LTG_DARITH_FP32, "bf16x6": cabi.LTG_DARITH_BF16X6, "bf16x4": cabi.LTG_DARITH_BF16X4}[d_arith]
        d_arith_code |= (int(os.environ.get("LTGAN_D_ARITH_SET", "0"), 0) & 15) << 4     # measurement switch: which of the four GEMM kernels
        self.cfg = cabi.ltg_config(self.I, self.H, self.Z, self.feature_len, self.h0, self.h1, self.h2, self.h3,
                                   self.precision, 0, self.item_lo, n_items if self.sharded else 0, self.d_precision, d_arith_code,
                                   lr, beta1, beta2, eps, seed)
        self.cfg.tuning = int(os.environ.get("LTGAN_TUNING", "0"), 0)     # measurement switch: ltg_config.tuning (include/ltg.h)
        self.lr, self.beta1, self.beta2 = lr, beta1, beta2
        self.adam_t = 0                                              # shared by D and G (Q5)
        if lazy_q0 is None:
            lazy_q0 = os.environ.get("LTGAN_LAZY_Q0", "1") != "0"   # measurement switch: 0 = dense sweep every step
        self.lazy_q0 = bool(lazy_q0) and self.I >= 8192
        self.q0_period = int(q0_period)
        if self.lazy_q0 and not 1 <= self.q0_period <= cabi.LTG_Q0_HIST // 2:
            raise ValueError("q0_period must be in [1, %d] (the clock's ring keeps the last %d step sizes)" % (cabi.LTG_Q0_HIST // 2, cabi.LTG_Q0_HIST))
        self.q0_defer = False                                        # True: the caller flushes (end of its G phase)
        self.q0_sweep_overlap = os.environ.get("LTGAN_Q0_OVERLAP", "1") != "0"   # measurement switch
        self._q0_dirty = False
        self._init_generator(seed)
        self._init_discriminator(d_seed)
        self._ws = None
        self._ws_key = (0, 0)
        self.loss_buf = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.overlap = True                                          # fake-tower forward on a second stream (ltg_g_opts.aux_stream)
        self._aux = None

    # ------------------------------------------------------------------ parameters
    def _init_generator(self, seed):
        self.set_generator(init_generator_host(self.I_global, self.H, self.Z, seed))     # global tables: set_generator keeps this rank's slab

    def set_generator(self, arrays, m=None, v=None):
        """arrays in engine layout: [W_q0 [I,H], W_q1 [H,2Z], W_p0 [Z,H], W_p1t [I,H], b_q0, b_q1, b_p0, b_p1] with
        I = the GLOBAL item count; an item-sharded engine keeps rows [item_lo, item_hi) of the item tables."""
        dev = self.device
        lo, hi = self.item_lo, self.item_hi

        def cut(seq):
            seq = list(seq)
            if seq[0].shape[0] == self.I_global and self.sharded:
                for i in (0, 3, 7):
                    seq[i] = seq[i][lo:hi]
            return seq
        arrays = cut(arrays)
        m = cut(m) if m is not None else None
        v = cut(v) if v is not None else None
        self.g_p = [torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev).contiguous() for a in arrays]
        self.g_m = [torch.zeros_like(t) if m is None else torch.as_tensor(np.ascontiguousarray(m[i]), dtype=torch.float32).to(dev)
                    for i, t in enumerate(self.g_p)]
        self.g_v = [torch.zeros_like(t) if v is None else torch.as_tensor(np.ascontiguousarray(v[i]), dtype=torch.float32).to(dev)
                    for i, t in enumerate(self.g_p)]
        if self.I >= 8192 and os.environ.get("LTGAN_ONE_BLOCK", "1") != "0":
            # theta / m / v of W_p1t in ONE allocation (each table on a 2-MiB boundary): the weight update streams the three in lock step, and
            # a sweep over three separate allocations measured 2-6 % below the same sweep over one block (scripts/micro/stagger.hip: 5.56-5.79
            # against 5.90 TB/s at 200 000 items; which of the two a process got showed as the two modes of profiles/r4_c4_two_modes.txt)
            n = self.g_p[3].numel()
            per = ((n * 4 + (2 << 20) - 1) // (2 << 20)) * (2 << 20) // 4
            self._p1_block = torch.empty(3 * per, dtype=torch.float32, device=dev)
            for k, lst in enumerate((self.g_p, self.g_m, self.g_v)):
                view = self._p1_block[k * per:k * per + n].view_as(lst[3])
                view.copy_(lst[3])
                lst[3] = view
        arr = lambda ts: (cabi.vp * 8)(*[_ptr(t) for t in ts])
        # bf16 shadow of W_p1t for the streaming decoder kernels (large item slabs only)
        self.g_shadow = None
        if self.precision == cabi.LTG_PREC_BF16 and self.I >= 8192 and self.I % 8 == 0 and self.H <= 608:
            self.g_shadow = torch.zeros(self.I, 608, dtype=torch.int16, device=dev)
        self.q0_last = self.q0_lr_hist = None
        if self.lazy_q0:                                             # all rows current at ordinal 0
            self.q0_last = torch.zeros(self.I, dtype=torch.int32, device=dev)
            self.q0_lr_hist = torch.zeros(cabi.LTG_Q0_HIST, dtype=torch.float32, device=dev)
        self._q0_dirty = False
        self._forget_ahead()                                         # (new weights, ordinal 0: no catch-up announced against the old clock stays valid)
        self.gen_c = cabi.ltg_gen_state(arr(self.g_p), arr(self.g_m), arr(self.g_v), _ptr(self.g_shadow),
                                        _ptr(self.q0_last), _ptr(self.q0_lr_hist), 0, self.q0_period if self.lazy_q0 else 0)
        if self.g_shadow is not None:
            cabi.check(self.lib.ltg_refresh_shadow(C.byref(self.cfg), C.byref(self.gen_c), self.stream()), "ltg_refresh_shadow")

    def _init_discriminator(self, seed):
        emb, host = init_discriminator_host(self.feature_len, (self.h0, self.h1, self.h2, self.h3), seed)
        self.set_discriminator(emb, host)

    def resize_discriminator(self, h_sizes, feature_len=None, d_seed=0):
        """Re-create the discriminator part for other layer sizes (discriminator.py:3: the sizes are arguments of the
        factory, not of the generator): fresh truncated-normal variables, zero Adam moments, new workspace."""
        _check_d_sizes(h_sizes)
        self.h0, self.h1, self.h2, self.h3 = (int(x) for x in h_sizes)
        if feature_len is not None:
            self.feature_len = int(feature_len)
        self.cfg.d_feat, self.cfg.d_h0, self.cfg.d_h1, self.cfg.d_h2, self.cfg.d_h3 = self.feature_len, self.h0, self.h1, self.h2, self.h3
        self._init_discriminator(d_seed)
        self._ws, self._ws_key = None, (0, 0)

    def set_learning_rate(self, lr):
        """tf.train.AdamOptimizer(LEARNING_RATE) (train.py:160): one optimiser, one rate for the D and the G update."""
        self.lr = float(lr)
        self.cfg.lr = self.lr

    def set_discriminator(self, emb, arrays, m=None, v=None):
        dev = self.device
        self.d_emb = torch.as_tensor(np.ascontiguousarray(emb), dtype=torch.float32).to(dev).contiguous()
        host = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        host[6] = host[6].reshape(-1)                                # w4 [h3,1] -> [h3]
        host[7] = host[7].reshape(-1)
        # the eight trainable tensors (and each of their Adam moments) live back to back in ONE buffer, padded to whole float4:
        # the library then runs the optimiser as a single flat 16-byte-per-lane sweep; d_p / d_m / d_v are views into it
        sizes = [a.size for a in host]
        total = (sum(sizes) + 3) // 4 * 4

        def flat(arrs):
            buf = torch.zeros(total, dtype=torch.float32, device=dev)
            views, off = [], 0
            for a, ref in zip(arrs, host):
                n = ref.size
                if a is not None:
                    buf[off:off + n] = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).reshape(-1).to(dev)
                views.append(buf[off:off + n].view(ref.shape))
                off += n
            return buf, views
        self.d_flat_p, self.d_p = flat(host)
        self.d_flat_m, self.d_m = flat([None] * 8 if m is None else list(m))
        self.d_flat_v, self.d_v = flat([None] * 8 if v is None else list(v))
        arr = lambda ts: (cabi.vp * 8)(*[_ptr(t) for t in ts])
        # e4m3 operand-format shadows for the fp8 mode of the wide discriminator (every layer size a multiple of 64): the frozen
        # embedding table and the TRANSPOSED weights, kept in step by the library's Adam sweep
        self.d_fp8 = None
        h0, h1, h2, h3 = self.h0, self.h1, self.h2, self.h3
        if self.d_precision == cabi.LTG_PREC_FP8 and all(x % 64 == 0 for x in (h0, h1, h2, h3)):
            u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
            self.d_fp8 = (u8(self.feature_len * h0), u8(h1 * h0), u8(h2 * h0), u8(h3 * (h1 + h2)), u8((h1 + h2) * h3))
        sh = [_ptr(t) for t in self.d_fp8] if self.d_fp8 else [None] * 5
        self.disc_c = cabi.ltg_disc_state(_ptr(self.d_emb), arr(self.d_p), arr(self.d_m), arr(self.d_v), *sh)
        if self.d_fp8:
            cabi.check(self.lib.ltg_refresh_d_shadow(C.byref(self.cfg), C.byref(self.disc_c), self.stream()), "ltg_refresh_d_shadow")

    # ------------------------------------------------------------------ plumbing
    def stream(self):
        """raw handle of the stream the library launches on: torch's current stream -- or the one a trainer pinned for the length
        of a phase (`pin_stream`: the lookup costs a few microseconds and a sharded G step makes seven of them)"""
        return self._pinned if self._pinned is not None else torch.cuda.current_stream(self.device).cuda_stream

    def pin_stream(self, on=True):
        self._pinned = torch.cuda.current_stream(self.device).cuda_stream if on else None

    def workspace(self, rows, pairs):
        rows, pairs = max(1, int(rows)), max(1, int(pairs))
        if self._ws is None or rows > self._ws_key[0] or pairs > self._ws_key[1]:
            rows = max(rows, self._ws_key[0])
            pairs = max(pairs, self._ws_key[1])
            nbytes = self.lib.ltg_workspace_bytes(C.byref(self.cfg), rows, pairs)
            if nbytes == 0:
                raise cabi.LtgError("ltg_workspace_bytes rejected the configuration")
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws_key = (rows, pairs)
        return self._ws

    def _fwd_scratch(self, rows):
        """row-statistics scratch of the forward (large item slabs only)"""
        if self.I <= 8192:
            return None
        need = int(self.lib.ltg_forward_scratch_bytes(C.byref(self.cfg), rows))
        if getattr(self, "_fs", None) is None or self._fs.numel() < need:
            self._fs = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._fs

    def new_acts(self, rows):
        return Acts(rows, self.I, self.H, self.Z, self.device)

    def _fork_handles(self):
        if not self.overlap:
            return None, None, None
        if self._aux is None:
            from ._hip import EventPair
            self._aux = (torch.cuda.Stream(self.device), EventPair(timing=False), EventPair(timing=False))
        st, ev = self._aux[:2]
        return st.cuda_stream, ev.start, ev.stop

    def _sweep_event(self):
        """ltg_g_opts.ev_sweep: the lazy clock's rotating slice runs on the aux stream beside the decoder kernels"""
        if not (self.overlap and self.lazy_q0 and self.q0_sweep_overlap):
            return None
        self._fork_handles()
        return self._aux[2].start

    def next_adam_t(self):
        self.adam_t += 1
        return self.adam_t

    # ------------------------------------------------------------------ the five run signatures
    def forward(self, batch, acts, keep_prob=0.75, is_training=0.0, rng_step=0, probs_out=None, drop_keep=None, eps=None,
                probe=None, rows_per_step=0):
        """sess.run(generator_out, {input_ph: X})  -- train.py:200, :339; test.py:146.
        rows_per_step > 0: `batch` spans several batches of that many rows; batch k draws its dropout with rng_step + k."""
        assert acts.rows >= batch.n_rows
        o = cabi.ltg_fwd_opts(keep_prob, is_training, rng_step, _ptr(drop_keep), _ptr(eps), _pp(probe), int(rows_per_step), 0)
        ws = self._fwd_scratch(batch.n_rows)
        rc = self.lib.ltg_vae_forward(C.byref(self.cfg), C.byref(self.gen_c), C.byref(batch.c), C.byref(o),
                                      C.byref(acts.c), _ptr(probs_out), _ptr(ws), ws.numel() if ws is not None else 0, self.stream())
        cabi.check(rc, "ltg_vae_forward")

    def sample_pairs(self, samp_c, acts, gen_out, pop_out, cnt_out, out_off=0):
        """the Python loop train.py:212-251 (+ sample.py:40-67) on the device."""
        rc = self.lib.ltg_sample_pairs(C.byref(self.cfg), C.byref(samp_c), _ptr(acts.logits), _ptr(acts.lse),
                                       _ptr(gen_out, out_off), _ptr(pop_out, out_off), _ptr(cnt_out), self.stream())
        cabi.check(rc, "ltg_sample_pairs")

    def d_step(self, real, fake, keep_prob=0.7, rng_step=0, loss_out=None, drop_real=None, drop_fake=None, probe=None):
        """sess.run([d_trainer, d_loss_mean], ...)  -- train.py:300."""
        loss_out = self.loss_buf if loss_out is None else loss_out
        ws = self.workspace(1, real.n + fake.n)
        dr = (cabi.vp * 3)(*[_ptr(t) for t in (drop_real or (None, None, None))])
        df = (cabi.vp * 3)(*[_ptr(t) for t in (drop_fake or (None, None, None))])
        o = cabi.ltg_d_opts(keep_prob, self.next_adam_t(), rng_step, dr, df, _pp(probe))
        if self.d_fork and self.d_precision == cabi.LTG_PREC_FP32:
            if self._dfork is None:
                self._dfork = DFork(self)
            if self._dfork.ready(self, self.stream()):
                self._dfork.seq = (self._dfork.seq + 1) & 0xFFFFFFFF
                o.aux_stream, o.sync, o.seq = self._dfork.stream.cuda_stream, _ptr(self._dfork.sync), self._dfork.seq
        rc = self.lib.ltg_d_step(C.byref(self.cfg), C.byref(self.disc_c), C.byref(real.c), C.byref(fake.c), C.byref(o),
                                 _ptr(loss_out), _ptr(ws), ws.numel(), self.stream())
        cabi.check(rc, "ltg_d_step")
        return loss_out

    # ------------------------------------------------------------------ the D step cut at its exchange point (pair rows split)
    def d_grad_floats(self):
        return int(self.lib.ltg_d_grad_floats(C.byref(self.cfg)))

    def d_grad(self, real, fake, row_lo, row_hi, grad_out, keep_prob=0.7, rng_step=0, drop_real=None, drop_fake=None):
        """forward + backward over pair rows [row_lo, row_hi) of real | fake -> this rank's gradient vector (+ loss share)"""
        ws = self.workspace(1, max(1, row_hi - row_lo))
        dr = (cabi.vp * 3)(*[_ptr(t) for t in (drop_real or (None, None, None))])
        df = (cabi.vp * 3)(*[_ptr(t) for t in (drop_fake or (None, None, None))])
        o = cabi.ltg_d_opts(keep_prob, 0, rng_step, dr, df, None)
        rc = self.lib.ltg_d_grad(C.byref(self.cfg), C.byref(self.disc_c), C.byref(real.c), C.byref(fake.c), int(row_lo), int(row_hi),
                                 C.byref(o), _ptr(grad_out), _ptr(ws), ws.numel(), self.stream())
        cabi.check(rc, "ltg_d_grad")

    def d_apply(self, grad, loss_out=None):
        """the (all-reduced) gradient vector -> one TF-Adam sweep at the next shared step; d_loss -> loss_out[0]"""
        loss_out = self.loss_buf if loss_out is None else loss_out
        rc = self.lib.ltg_d_apply(C.byref(self.cfg), C.byref(self.disc_c), _ptr(grad), self.next_adam_t(), _ptr(loss_out), self.stream())
        cabi.check(rc, "ltg_d_apply")
        return loss_out

    def fake_tower_batched(self, fake, seg_of, seg_row0, seg_step, y_out, d_keep_prob=0.7, seg_off=0, y_off=0):
        """y_generated of MANY pair batches in one pass (the discriminator is fixed during phase G): `fake` = the concatenated
        slots, seg_of (+ seg_off) / seg_row0 / seg_step as in include/ltg.h; the G steps then take their slice through `y_pre`."""
        ws = self.workspace(1, fake.n)
        cabi.check(self.lib.ltg_fake_tower_batched(C.byref(self.cfg), C.byref(self.disc_c), C.byref(fake.c), _ptr(seg_of, seg_off), _ptr(seg_row0),
                                                   _ptr(seg_step), d_keep_prob, _ptr(y_out, y_off), _ptr(ws), ws.numel(), self.stream()),
                   "ltg_fake_tower_batched")

    def g_step(self, batch, fake, acts, cnt, anneal, gan_lambda=1.0, keep_prob=0.75, is_training=1.0, d_keep_prob=0.7,
               rng_step=0, d_rng_step=0, loss_out=None, drop_keep=None, eps=None, drop_fake=None, probe=None, y_pre=None, y_off=0):
        """sess.run([g_trainer, g_loss_mean, g_vae_loss, gan_loss], ...)  -- train.py:326.
        y_pre (+ y_off): y_generated of this batch's fake pairs from fake_tower_batched (same d_rng_step): no tower in the step."""
        loss_out = self.loss_buf if loss_out is None else loss_out
        ws = self.workspace(batch.n_rows, fake.n)
        f = cabi.ltg_fwd_opts(keep_prob, is_training, rng_step, _ptr(drop_keep), _ptr(eps), _pp(probe))
        df = (cabi.vp * 3)(*[_ptr(t) for t in (drop_fake or (None, None, None))])
        o = cabi.ltg_g_opts(f, anneal, gan_lambda, d_keep_prob, self.next_adam_t(), d_rng_step, df, _ptr(cnt), _pp(probe),
                            *self._fork_handles(), 0, 0, self._sweep_event(), _ptr(y_pre, y_off))
        rc = self.lib.ltg_g_step(C.byref(self.cfg), C.byref(self.gen_c), C.byref(self.disc_c), C.byref(batch.c),
                                 C.byref(fake.c), C.byref(o), C.byref(acts.c), _ptr(loss_out), _ptr(ws), ws.numel(),
                                 self.stream())
        cabi.check(rc, "ltg_g_step")
        self._q0_stepped()
        return loss_out

    def _q0_stepped(self):
        """one more G step on the lazy clock of W_q0 (ltg_gen_state.q0_ord is the caller's to advance)"""
        if self.lazy_q0:
            self.gen_c.q0_ord += 1
            self._q0_dirty = True
            if not self.q0_defer:
                self.g_flush()

    def g_flush(self):
        """every deferred zero-gradient Adam step of W_q0, all rows: before W_q0 / its moments are read outside a forward"""
        if self.lazy_q0 and self._q0_dirty:
            if self.check_on_flush:
                self.check_pipes()                                   # (end of a G phase / before the model is read out: one host sync.  BEFORE the
                                                                     # flush: behind a wait that gave up the clock's ordinals are not to be trusted)
            cabi.check(self.lib.ltg_g_flush(C.byref(self.cfg), C.byref(self.gen_c), self.stream()), "ltg_g_flush")
            self._q0_dirty = False
            # every row is current: restart the ordinals (the int32 clock never grows without bound; stream order keeps the
            # memset behind the flush kernel)
            self.q0_last.zero_()
            self.gen_c.q0_ord = 0
            self._forget_ahead()       # (an announcement made against the old ordinals must not match a later call's key)

    def _forget_ahead(self):
        """the clock's ordinals restart (flush, new weights): no pipe's catch-up-ahead announcement is valid any more"""
        for pipe in list(self._pipes):
            pipe.ahead = None
            pipe.c.next_uitem, pipe.c.next_nu, pipe.c.caught_up = None, 0, 0

    def check_pipes(self):
        """raises if a device-side wait of a one-call G step gave up (ltg_pipe.sync[LTG_WORD_POISON]).  The kernels behind such a wait have skipped
        their work, so the model is the one from before that step -- but the run is not the run that was asked for.  ONE device-to-host
        copy and one synchronisation however many pipes the engine has."""
        words = [pipe.sync[cabi.LTG_WORD_POISON:cabi.LTG_WORD_POISON + 1] for pipe in list(self._pipes) + ([self._dfork] if self._dfork is not None else [])]
        if not words:
            return
        n = int((words[0] if len(words) == 1 else torch.cat(words)).sum().item())
        if n:
            torch.cuda.synchronize(self.device)
            self.refresh_shadow()      # (a skipped weight update did not write the shadow buffer the host has switched to since)
            raise cabi.LtgError("%d device-side wait(s) of a step's hand-overs gave up: the steps behind them were skipped, "
                                "the results of that phase are not trustworthy" % n)

    # ------------------------------------------------------------------ the G step cut at its exchange points
    def fwd_opts(self, keep_prob=0.75, is_training=0.0, rng_step=0, drop_keep=None, eps=None, probe=None):
        return cabi.ltg_fwd_opts(keep_prob, is_training, rng_step, _ptr(drop_keep), _ptr(eps), _pp(probe))

    def g_opts(self, cnt, anneal, gan_lambda=1.0, keep_prob=0.75, is_training=1.0, d_keep_prob=0.7, rng_step=0, d_rng_step=0,
               drop_keep=None, eps=None, drop_fake=None, probe=None, y_pre=None, y_off=0):
        f = self.fwd_opts(keep_prob, is_training, rng_step, drop_keep, eps, probe)
        df = (cabi.vp * 3)(*[_ptr(t) for t in (drop_fake or (None, None, None))])
        return cabi.ltg_g_opts(f, anneal, gan_lambda, d_keep_prob, self.next_adam_t(), d_rng_step, df, _ptr(cnt), _pp(probe),
                               *self._fork_handles(), 0, 0, None, _ptr(y_pre, y_off))      # ltg_g_bwd_rest forks / joins inside the call

    # ------------------------------------------------------------------ the item-sharded G step as ONE call
    def sharded_step_ok(self, rows):
        """ltg_g_step_sharded serves this engine's configuration (bf16 + shadow, lazy clock, slab of >= 8192 items, <= 128 rows)"""
        if not hasattr(self.lib, "ltg_g_step_sharded_ok"):      # an older build loaded through LTG_HIP_LIB (A/B timing)
            return False
        return bool(self.lib.ltg_g_step_sharded_ok(C.byref(self.cfg), C.byref(self.gen_c), int(rows)))

    def g_route(self, rows):
        """the kernels a G step (or a forward) over `rows` batch rows runs with this engine's configuration (include/ltg.h: ltg_g_route)"""
        out = cabi.ltg_g_route_info()
        if not self.lib.ltg_g_route(C.byref(self.cfg), C.byref(self.gen_c), int(rows), C.byref(out)):
            raise cabi.LtgError("ltg_g_route refused the configuration")
        return out

    def d_route(self, n, with_bwd=True):
        """the kernels a D step (with_bwd) or a forward-only tower over n pair rows runs (include/ltg.h: ltg_d_route)"""
        out = cabi.ltg_d_route_info()
        has_aux = bool(with_bwd and self.d_fork and self.d_precision == cabi.LTG_PREC_FP32)
        if not self.lib.ltg_d_route(C.byref(self.cfg), C.byref(self.disc_c), int(n), int(bool(with_bwd)), int(has_aux), C.byref(out)):
            raise cabi.LtgError("ltg_d_route refused the configuration")
        return out

    def pipe_plan(self, batch, pipe):
        """where each stage of a one-call G step over `batch` on `pipe` runs and what it waits for (include/ltg.h: ltg_g_pipe_plan); None
        when ltg_g_step_sharded would refuse the call"""
        out = cabi.ltg_pipe_plan_info()
        if not hasattr(self.lib, "ltg_g_pipe_plan"):
            # An older build under LTG_AB_COMPAT (A/B timing against it must find it as fast as it was): the plan from what such a
            # library can answer -- the two bits of ltg_g_step_sharded_plan (before ABI 13: neither), and for the hand-over the rule it
            # applies to flags / sync itself.  The fields the host does not read stay 0.  This path only.
            fl = int(pipe.c.flags)
            if hasattr(self.lib, "ltg_g_step_sharded_plan"):
                bits = self.lib.ltg_g_step_sharded_plan(C.byref(self.cfg), C.byref(self.gen_c), C.byref(batch.c), C.byref(pipe.c))
                out.ahead, out.shadow = int(bool(bits & cabi.LTG_PLAN_AHEAD)), int(bool(bits & cabi.LTG_PLAN_SHADOW))
            out.handover = (cabi.LTG_HAND_ORDER if fl & cabi.LTG_PIPE_NO_DEC1_FORK else
                            cabi.LTG_HAND_WORDS if pipe.c.sync and not fl & cabi.LTG_PIPE_EVENTS else cabi.LTG_HAND_EVENTS)
            out.tail_own = int(out.handover == cabi.LTG_HAND_WORDS and bool(pipe.c.tail_stream) and bool(fl & cabi.LTG_PIPE_TAIL_OWN))
            return out
        ok = self.lib.ltg_g_pipe_plan(C.byref(self.cfg), C.byref(self.gen_c), C.byref(batch.c), C.byref(pipe.c), C.byref(out))
        return out if ok else None

    def g_step_sharded(self, batch, fake, acts, gopts, pipe, comm=None, loss_out=None, next_batch=None):
        """every launch of the step and its exchanges from one call (comm: _rccl.RcclComm / HostComm; None = one rank).
        next_batch: the batch of the NEXT call on this pipe when the caller knows it -- its rows of W_q0 are brought up to the lazy clock
        during this call on the side stream, and the next call launches no catch-up (include/ltg.h: catch-up ahead)"""
        loss_out = self.loss_buf if loss_out is None else loss_out
        ws = self.workspace(batch.n_rows, fake.n)
        self._pipe_ready(pipe, batch)
        if pipe.c.seq >= 0x7FFFFFF0:                                   # (the marks compare ordinals: restart long before they could repeat)
            self.pipe_join(pipe)
            pipe.reset()
        pipe.c.seq = (pipe.c.seq + 1) & 0xFFFFFFFF                     # the call's ordinal on this pipe (what its gates count in)
        key = (batch.c.uitem, int(batch.c.n_unique), int(self.gen_c.q0_ord), int(pipe.c.seq))
        pipe.c.caught_up = 1 if (pipe.ahead is not None and pipe.ahead == key) else 0
        pipe.ahead_calls += pipe.c.caught_up
        pipe.ahead = None
        pipe.c.next_uitem, pipe.c.next_nu = None, 0
        plan = self.pipe_plan(batch, pipe)     # (None: the call below is refused)
        if next_batch is not None and next_batch.c.uitem and self.q0_defer and plan is not None and plan.ahead:
            pipe.c.next_uitem, pipe.c.next_nu = next_batch.c.uitem, int(next_batch.c.n_unique)
            pipe.ahead = (next_batch.c.uitem, int(next_batch.c.n_unique), int(self.gen_c.q0_ord) + 1, (int(pipe.c.seq) + 1) & 0xFFFFFFFF)
        rc = self.lib.ltg_g_step_sharded(C.byref(self.cfg), C.byref(self.gen_c), C.byref(self.disc_c), C.byref(batch.c), C.byref(fake.c),
                                         C.byref(gopts), C.byref(acts.c), C.byref(comm.c) if comm is not None else None, C.byref(pipe.c),
                                         _ptr(loss_out), _ptr(ws), ws.numel(), self.stream())
        if rc != 0:
            pipe.reset()               # (the call may have stopped between its gate launches: words of this ordinal that nobody will set)
            self.refresh_shadow()      # (... or between the update's launch and the exchange below)
        cabi.check(rc, "ltg_g_step_sharded")
        if plan is not None and plan.shadow:    # the update wrote the pipe's buffer: it is the shadow from now on, the old one the next call's target
            self.g_shadow, pipe.shadow = pipe.shadow, self.g_shadow
            self.gen_c.wp1t_bf16, pipe.c.shadow_out = _ptr(self.g_shadow), _ptr(pipe.shadow)
        if not self.q0_defer:
            self.pipe_join(pipe)       # a standalone step: nothing stays in flight behind the call (a trainer joins once per phase)
        self._q0_stepped()             # (standalone: flushes the clock and checks the pipe's poison -- g_flush)
        return loss_out

    def refresh_shadow(self):
        """the bf16 shadow of W_p1t rebuilt from the fp32 rows (after loading weights; after a failed pipelined call)"""
        if self.g_shadow is not None:
            cabi.check(self.lib.ltg_refresh_shadow(C.byref(self.cfg), C.byref(self.gen_c), self.stream()), "ltg_refresh_shadow")

    HANDOVER = {cabi.LTG_HAND_ORDER: "none (everything in program order)", cabi.LTG_HAND_EVENTS: "events", cabi.LTG_HAND_WORDS: "device-words"}

    def _pipe_ready(self, pipe, batch):
        """The device-word hand-over of ltg_g_step_sharded needs two CONCURRENT streams; HIP maps streams onto a few hardware queues, so
        the pair is tested once (ltg_g_pipe_probe; a few other side streams are tried, then the pipe falls back to event pairs).
        pipe.handover then says what the library's plan for this pipe is."""
        st = self.stream()
        if pipe.probed_for == st:
            return
        if pipe.probed_for is not None:
            self.pipe_join(pipe)                     # the mode may change: nothing in flight across the change
            torch.cuda.synchronize(self.device)
        plan = self.pipe_plan(batch, pipe)
        if plan is None:
            return                                   # (the call will be refused; the streams stay untested for the next one)
        if plan.handover == cabi.LTG_HAND_WORDS:
            tail = pipe.c.tail_stream
            pipe.c.tail_stream = None                # the side stream first ...
            if not _probe_streams(self.lib, lambda: pipe.c, st, 6, lambda k: pipe.new_side_stream()):
                pipe.c.flags |= cabi.LTG_PIPE_EVENTS
                pipe.new_tail_stream(drop=True)
            elif tail:                               # ... then the tail's own stream: a third concurrent queue, or the tail stays on the caller's stream
                pipe.c.tail_stream = tail
                # (a process that has created many streams: the next few may share the side stream's queue)
                _probe_streams(self.lib, lambda: pipe.c, st, 10, lambda k: pipe.new_tail_stream(drop=(k == 9)))
            plan = self.pipe_plan(batch, pipe)
        pipe.handover = self.HANDOVER[plan.handover] + (" + tail stream" if plan.tail_own else "")
        pipe.probed_for = st

    def pipe_join(self, pipe):
        cabi.check(self.lib.ltg_g_pipe_join(C.byref(pipe.c), self.stream()), "ltg_g_pipe_join")

    def g_fwd_enc(self, batch, acts, fopts):
        cabi.check(self.lib.ltg_g_fwd_enc(C.byref(self.cfg), C.byref(self.gen_c), C.byref(batch.c), C.byref(fopts), C.byref(acts.c),
                                          self.stream()), "ltg_g_fwd_enc")

    def g_fwd_rest(self, batch, fake, acts, fopts, rowpart_out):
        ws = self.workspace(batch.n_rows, fake.n if fake else 1)
        cabi.check(self.lib.ltg_g_fwd_rest(C.byref(self.cfg), C.byref(self.gen_c), C.byref(batch.c), C.byref(fake.c) if fake else None,
                                           C.byref(fopts), C.byref(acts.c), _ptr(rowpart_out), _ptr(ws), ws.numel(), self.stream()),
                   "ltg_g_fwd_rest")

    def rowstats_combine(self, rowpart_all, n_ranks, n_rows, lse_out):
        ws = self.workspace(n_rows, 1)
        cabi.check(self.lib.ltg_rowstats_combine(C.byref(self.cfg), _ptr(rowpart_all), n_ranks, n_rows, _ptr(lse_out), _ptr(ws), ws.numel(),
                                                 self.stream()), "ltg_rowstats_combine")

    def g_bwd_dec(self, batch, fake, acts, gopts, rowpart_all, n_ranks, loss_out, dh2_out):
        ws = self.workspace(batch.n_rows, fake.n)
        cabi.check(self.lib.ltg_g_bwd_dec(C.byref(self.cfg), C.byref(self.gen_c), C.byref(self.disc_c), C.byref(batch.c), C.byref(fake.c),
                                          C.byref(gopts), C.byref(acts.c), _ptr(rowpart_all), n_ranks, _ptr(loss_out), _ptr(dh2_out),
                                          _ptr(ws), ws.numel(), self.stream()), "ltg_g_bwd_dec")

    def g_fake_tower(self, batch, fake, gopts, stream=None):
        """the fake tower's forward of the step, on `stream` (a torch stream; default: the current one); sets gopts.fake_done"""
        ws = self.workspace(batch.n_rows, fake.n)
        st = self.stream() if stream is None else stream.cuda_stream
        cabi.check(self.lib.ltg_g_fake_tower(C.byref(self.cfg), C.byref(self.disc_c), C.byref(fake.c), C.byref(gopts), batch.n_rows, _ptr(ws),
                                             ws.numel(), st), "ltg_g_fake_tower")
        gopts.fake_done = 1

    def g_bwd_dec1(self, batch, fake, acts, gopts, stream=None):
        """Adam on the local W_p1t / b_p1 rows: needs nothing of the dh2 exchange, so it is issued while that all-reduce flies
        (`stream`: a torch side stream -- the caller orders it behind ltg_g_bwd_dec and joins it before the next forward)"""
        ws = self.workspace(batch.n_rows, fake.n)
        st = self.stream() if stream is None else stream.cuda_stream
        cabi.check(self.lib.ltg_g_bwd_dec1(C.byref(self.cfg), C.byref(self.gen_c), C.byref(batch.c), C.byref(fake.c), C.byref(gopts),
                                           C.byref(acts.c), _ptr(ws), ws.numel(), st), "ltg_g_bwd_dec1")
        gopts.dec1_done = 1

    def g_bwd_rest(self, batch, fake, acts, gopts, dh2):
        ws = self.workspace(batch.n_rows, fake.n)
        cabi.check(self.lib.ltg_g_bwd_rest(C.byref(self.cfg), C.byref(self.gen_c), C.byref(batch.c), C.byref(fake.c), C.byref(gopts),
                                           C.byref(acts.c), _ptr(dh2), _ptr(ws), ws.numel(), self.stream()), "ltg_g_bwd_rest")
        self._q0_stepped()

    def gather_cand_logits(self, samp_c, acts, out):
        cabi.check(self.lib.ltg_gather_cand_logits(C.byref(self.cfg), C.byref(samp_c), _ptr(acts.logits), _ptr(out), self.stream()),
                   "ltg_gather_cand_logits")

    def rank_metrics(self, acts, tr, te, out, k_ndcg=100, k_r1=20, k_r2=50):
        """pred[X.nonzero()] = -inf + NDCG@100 / Recall@20 / Recall@50  -- train.py:341-346."""
        rc = self.lib.ltg_rank_metrics(C.byref(self.cfg), _ptr(acts.logits), C.byref(tr.c), C.byref(te.c), k_ndcg, k_r1,
                                       k_r2, _ptr(out), self.stream())
        cabi.check(rc, "ltg_rank_metrics")

    # ------------------------------------------------------------------ ranking metrics cut at their exchange points
    def rank_scores(self, acts, tr, te, score_out):
        cabi.check(self.lib.ltg_rank_scores(C.byref(self.cfg), _ptr(acts.logits), C.byref(tr.c), C.byref(te.c), _ptr(score_out),
                                            self.stream()), "ltg_rank_scores")

    def rank_counts(self, acts, tr, te, score, count_out):
        cabi.check(self.lib.ltg_rank_counts(C.byref(self.cfg), _ptr(acts.logits), C.byref(tr.c), C.byref(te.c), _ptr(score),
                                            _ptr(count_out), self.stream()), "ltg_rank_counts")

    def rank_finish(self, te, counts, out, k_ndcg=100, k_r1=20, k_r2=50):
        cabi.check(self.lib.ltg_rank_finish(C.byref(te.c), _ptr(counts), k_ndcg, k_r1, k_r2, _ptr(out), self.stream()), "ltg_rank_finish")

    # ------------------------------------------------------------------ top-K recommendations
    def topk(self, logits_or_acts, tr, k, score_out, id_out):
        """the k best items of each of the score_out.shape[0] rows of this slab's logits (an Acts or a [rows, I] float32 tensor),
        fold-in items of `tr` (a CsrRows with LOCAL ids, or None) excluded: score_out [rows, k] float32, id_out [rows, k] int32 GLOBAL
        ids (ltg_topk: score descending, ties lower id first, padding id -1 / score -inf)."""
        logits = logits_or_acts.logits if isinstance(logits_or_acts, Acts) else logits_or_acts
        n = int(score_out.shape[0])
        assert logits.dtype == torch.float32 and logits.numel() >= n * self.I and tuple(id_out.shape) == tuple(score_out.shape) == (n, k)
        assert score_out.is_contiguous() and id_out.is_contiguous() and id_out.dtype == torch.int32
        cabi.check(self.lib.ltg_topk(C.byref(self.cfg), _ptr(logits), C.byref(tr.c) if tr is not None else None, n, int(k),
                                     _ptr(score_out), _ptr(id_out), self.stream()), "ltg_topk")

    def topk_merge(self, score_in, id_in, k, score_out, id_out):
        """top-k of the union of the per-slab lists score_in / id_in [parts, rows, k_in] (each as topk writes it) -> [rows, k]"""
        parts, n, k_in = (int(x) for x in score_in.shape)
        assert tuple(id_in.shape) == (parts, n, k_in) and tuple(score_out.shape) == tuple(id_out.shape) == (n, k)
        assert score_in.is_contiguous() and id_in.is_contiguous() and score_out.is_contiguous() and id_out.is_contiguous()
        cabi.check(self.lib.ltg_topk_merge(parts, n, k_in, _ptr(score_in), _ptr(id_in), int(k), _ptr(score_out), _ptr(id_out),
                                           self.stream()), "ltg_topk_merge")

    def topk_groups(self, logits_or_acts, tr, k, labels, group_mask, score_out, id_out):
        """topk over the items whose label is admitted: labels uint8 per GLOBAL item id, bit g of group_mask admits label g (g < 8),
        bit 8 every label >= 8 (ltg_topk_groups); everything else as topk"""
        logits = logits_or_acts.logits if isinstance(logits_or_acts, Acts) else logits_or_acts
        n = int(score_out.shape[0])
        assert logits.dtype == torch.float32 and logits.numel() >= n * self.I and tuple(id_out.shape) == tuple(score_out.shape) == (n, k)
        assert score_out.is_contiguous() and id_out.is_contiguous() and id_out.dtype == torch.int32
        assert labels.dtype == torch.uint8 and labels.is_contiguous()
        cabi.check(self.lib.ltg_topk_groups(C.byref(self.cfg), _ptr(logits), C.byref(tr.c) if tr is not None else None, n, int(k),
                                            _ptr(labels), int(labels.numel()), int(group_mask), _ptr(score_out), _ptr(id_out),
                                            self.stream()), "ltg_topk_groups")

    def topk_sample(self, logits_or_acts, tr, row_lo, k, inv_temp, draw, excl, key_out, id_out, g_noise=None):
        """the k largest Gumbel keys of each of the key_out.shape[0] rows of this slab's logits: the sampled part of an exploration list
        (ltg_topk_sample).  row_lo: the GLOBAL row of the first row; inv_temp: float32(1 / T); draw: the counter of the draw; excl: the
        fixed head [rows, f] int32 GLOBAL ids (as topk / topk_merge wrote it), or None; g_noise: injected Gumbel values [rows, I] (tests).
        -> key_out [rows, k] float32, id_out [rows, k] int32 GLOBAL ids, ordered and padded as topk writes a list"""
        logits = logits_or_acts.logits if isinstance(logits_or_acts, Acts) else logits_or_acts
        n = int(key_out.shape[0])
        assert logits.dtype == torch.float32 and logits.numel() >= n * self.I and tuple(id_out.shape) == tuple(key_out.shape) == (n, k)
        assert key_out.is_contiguous() and id_out.is_contiguous() and id_out.dtype == torch.int32
        f = 0 if excl is None else int(excl.shape[1])
        assert excl is None or (excl.dtype == torch.int32 and excl.is_contiguous() and int(excl.shape[0]) == n)
        assert g_noise is None or (g_noise.dtype == torch.float32 and g_noise.is_contiguous() and g_noise.numel() >= n * self.I)
        cabi.check(self.lib.ltg_topk_sample(C.byref(self.cfg), _ptr(logits), C.byref(tr.c) if tr is not None else None, n, int(row_lo), int(k),
                                            float(inv_temp), int(draw), _ptr(excl) if f else None, f, _ptr(g_noise), _ptr(key_out),
                                            _ptr(id_out), self.stream()), "ltg_topk_sample")

    def topk_sample_mass(self, logits_or_acts, tr, inv_temp, excl, ids, score_out, max_out, rest_out):
        """this slab's part of the mass behind the FINAL picks ids [rows, k] int32 (ltg_topk_sample_mass): score_out [rows, k] the raw logit
        of every pick the slab owns (-inf elsewhere), max_out [rows] the largest eligible logit, rest_out [rows] the sum over the eligible
        items that were not picked of exp((s - max_out) * inv_temp); excl as topk_sample takes it"""
        logits = logits_or_acts.logits if isinstance(logits_or_acts, Acts) else logits_or_acts
        n, k = (int(x) for x in ids.shape)
        assert logits.dtype == torch.float32 and logits.numel() >= n * self.I and tuple(score_out.shape) == (n, k)
        assert ids.is_contiguous() and ids.dtype == torch.int32 and score_out.is_contiguous() and max_out.numel() >= n and rest_out.numel() >= n
        assert max_out.is_contiguous() and rest_out.is_contiguous() and max_out.dtype == rest_out.dtype == score_out.dtype == torch.float32
        f = 0 if excl is None else int(excl.shape[1])
        assert excl is None or (excl.dtype == torch.int32 and excl.is_contiguous() and int(excl.shape[0]) == n)
        cabi.check(self.lib.ltg_topk_sample_mass(C.byref(self.cfg), _ptr(logits), C.byref(tr.c) if tr is not None else None, n, k,
                                                 float(inv_temp), _ptr(excl) if f else None, f, _ptr(ids), _ptr(score_out), _ptr(max_out),
                                                 _ptr(rest_out), self.stream()), "ltg_topk_sample_mass")

    def topk_sample_finish(self, score, M, rest, inv_temp, logp_out):
        """logp_out [rows, k] <- the conditional log-probability of every pick, from the picks' logits score [rows, k], the largest
        eligible logit M [rows] and the mass of the unpicked items rest [rows], all over the WHOLE catalogue (ltg_topk_sample_finish)"""
        n, k = (int(x) for x in score.shape)
        assert tuple(logp_out.shape) == (n, k) and M.numel() >= n and rest.numel() >= n
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (score, M, rest, logp_out))
        cabi.check(self.lib.ltg_topk_sample_finish(n, k, _ptr(score), _ptr(M), _ptr(rest), float(inv_temp), _ptr(logp_out), self.stream()),
                   "ltg_topk_sample_finish")

    def posterior_ld(self):
        """bf16 elements per row of a posterior image (ltg_posterior_ld): H rounded up to 32"""
        return int(self.lib.ltg_posterior_ld(C.byref(self.cfg)))

    def posterior_image(self, rows, samples):
        """-> an image buffer [rows * samples, posterior_ld()] int16 (bf16 bits) on the engine's device"""
        nbytes = int(self.lib.ltg_posterior_image_bytes(C.byref(self.cfg), int(rows), int(samples)))
        if nbytes == 0 and rows > 0:
            raise ValueError("no posterior image for %r rows of %r samples (samples in {1, 4, 8, 16, 32})" % (rows, samples))
        return torch.empty(int(rows) * int(samples), self.posterior_ld(), dtype=torch.int16, device=self.device)

    def posterior_h2(self, mulv, n, row_lo, samples, draw, image_out, eps=None, z_out=None):
        """image_out [n * samples, ld] <- bf16(tanh(dec-0)) of `samples` draws of z from the posterior of each of the first n rows of mulv
        [rows, 2Z] (ltg_posterior_h2).  row_lo: the GLOBAL row of the first row; draw: the counter of the draw; eps: injected noise
        [n, samples, Z] (tests), the counter RNG otherwise; z_out: [n * samples, Z] receives z"""
        n, S = int(n), int(samples)
        assert mulv.dtype == torch.float32 and mulv.is_contiguous() and mulv.numel() >= n * 2 * self.Z
        assert image_out.dtype == torch.int16 and image_out.is_contiguous() and image_out.numel() >= n * S * self.posterior_ld()
        assert eps is None or (eps.dtype == torch.float32 and eps.is_contiguous() and eps.numel() >= n * S * self.Z)
        assert z_out is None or (z_out.dtype == torch.float32 and z_out.is_contiguous() and z_out.numel() >= n * S * self.Z)
        cabi.check(self.lib.ltg_posterior_h2(C.byref(self.cfg), C.byref(self.gen_c), _ptr(mulv), n, int(row_lo), S, int(draw), _ptr(eps),
                                             _ptr(image_out), _ptr(z_out), self.stream()), "ltg_posterior_h2")

    def posterior_scores(self, image, n, samples, beta, score_out, spread_out=None):
        """score_out [n, I] <- mean + beta * std over the samples of this slab's logits, from the image posterior_h2 wrote
        (ltg_posterior_scores; bf16 operands whatever the engine's precision); spread_out [n, I] receives std"""
        n, S = int(n), int(samples)
        assert image.dtype == torch.int16 and image.is_contiguous() and image.numel() >= n * S * self.posterior_ld()
        assert score_out.dtype == torch.float32 and score_out.is_contiguous() and score_out.numel() >= n * self.I
        assert spread_out is None or (spread_out.dtype == torch.float32 and spread_out.is_contiguous() and spread_out.numel() >= n * self.I)
        cabi.check(self.lib.ltg_posterior_scores(C.byref(self.cfg), C.byref(self.gen_c), _ptr(image), n, S, float(beta), _ptr(score_out),
                                                 _ptr(spread_out), self.stream()), "ltg_posterior_scores")

    def posterior_entries(self, image, samples, ids, mean_out, std_out):
        """mean_out / std_out [n, k] <- the posterior mean and std of the entries ids [n, k] int32 (GLOBAL ids), from the same image
        (ltg_posterior_entries); an id outside this slab and padding give 0.0 in both"""
        n, k = (int(x) for x in ids.shape)
        assert image.dtype == torch.int16 and image.is_contiguous() and image.numel() >= n * int(samples) * self.posterior_ld()
        assert ids.dtype == torch.int32 and ids.is_contiguous() and tuple(mean_out.shape) == tuple(std_out.shape) == (n, k)
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (mean_out, std_out))
        cabi.check(self.lib.ltg_posterior_entries(C.byref(self.cfg), C.byref(self.gen_c), _ptr(image), n, int(samples), _ptr(ids), k,
                                                  _ptr(mean_out), _ptr(std_out), self.stream()), "ltg_posterior_entries")

    def row_lse(self, logits, n, lse_out):
        """lse_out [n] <- the log-sum-exp of each of the first n rows of logits [rows, I] (ltg_row_lse)"""
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= int(n) * self.I
        assert lse_out.dtype == torch.float32 and lse_out.is_contiguous() and lse_out.numel() >= int(n)
        cabi.check(self.lib.ltg_row_lse(C.byref(self.cfg), _ptr(logits), int(n), _ptr(lse_out), self.stream()), "ltg_row_lse")

    def list_mass(self, logits_or_acts, tr, ids, excl, inv_temps, score_out, state_out, max_out, rest_out):
        """this slab's part of the mass behind the LOGGED lists ids [rows, k] int32 under the target policies inv_temps (a host sequence of
        up to 8 float32(1 / T)) that share the head excl [rows, f] (or None) (ltg_list_mass): state_out [rows, k] int32 1 = eligible / 2 =
        not / 0 = head slot, padding or another slab's id; score_out [rows, k] the raw logit where the state is 1, -inf elsewhere; max_out
        [rows] the largest eligible logit; rest_out [n_pol, rows] the sum over the eligible items that are not a state-1 entry of
        exp((s - max_out) * inv_temp)"""
        logits = logits_or_acts.logits if isinstance(logits_or_acts, Acts) else logits_or_acts
        n, k = (int(x) for x in ids.shape)
        n_pol = len(inv_temps)
        assert logits.dtype == torch.float32 and logits.numel() >= n * self.I and tuple(score_out.shape) == tuple(state_out.shape) == (n, k)
        assert ids.is_contiguous() and ids.dtype == torch.int32 and score_out.is_contiguous() and state_out.is_contiguous()
        assert state_out.dtype == torch.int32 and max_out.numel() >= n and tuple(rest_out.shape) == (n_pol, n)
        assert max_out.is_contiguous() and rest_out.is_contiguous() and max_out.dtype == rest_out.dtype == score_out.dtype == torch.float32
        f = 0 if excl is None else int(excl.shape[1])
        assert excl is None or (excl.dtype == torch.int32 and excl.is_contiguous() and int(excl.shape[0]) == n)
        it = (C.c_float * max(1, n_pol))(*[float(x) for x in inv_temps])
        cabi.check(self.lib.ltg_list_mass(C.byref(self.cfg), _ptr(logits), C.byref(tr.c) if tr is not None else None, n, k, _ptr(ids), f,
                                          _ptr(excl) if f else None, n_pol, it, _ptr(score_out), _ptr(state_out), _ptr(max_out),
                                          _ptr(rest_out), self.stream()), "ltg_list_mass")

    def replay_rows(self, inv_temps, head, ids, logp0, reward, score, state, M, rest, labels, n_groups, clip, row_out, w_out, first_bad_out,
                    logp1_out=None):
        """the prefix importance weights of the logged rows ids / logp0 / reward [rows, k] under the target policies, from the merged score /
        state [rows, k], M [rows] and rest [n_pol, rows] of the whole catalogue and the target's head [rows, f] (or None) (ltg_replay_rows):
        row_out [rows, n_pol, n_groups + 1, 2] float64 (A, B), w_out [rows, n_pol] float64, first_bad_out [rows, n_pol] int32, logp1_out
        (optional) [n_pol, rows, k] float32; labels uint8 per GLOBAL item id"""
        n, k = (int(x) for x in ids.shape)
        n_pol, g = len(inv_temps), int(n_groups)
        for t in (ids, state):
            assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (n, k)
        for t in (logp0, reward, score):
            assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, k)
        assert M.dtype == rest.dtype == torch.float32 and M.is_contiguous() and rest.is_contiguous() and M.numel() >= n
        assert tuple(rest.shape) == (n_pol, n) and labels.dtype == torch.uint8 and labels.is_contiguous()
        assert row_out.dtype == w_out.dtype == torch.float64 and row_out.is_contiguous() and w_out.is_contiguous()
        assert tuple(row_out.shape) == (n, n_pol, g + 1, 2) and tuple(w_out.shape) == tuple(first_bad_out.shape) == (n, n_pol)
        assert first_bad_out.dtype == torch.int32 and first_bad_out.is_contiguous()
        assert logp1_out is None or (logp1_out.dtype == torch.float32 and logp1_out.is_contiguous() and tuple(logp1_out.shape) == (n_pol, n, k))
        f = 0 if head is None else int(head.shape[1])
        assert head is None or (head.dtype == torch.int32 and head.is_contiguous() and int(head.shape[0]) == n)
        it = (C.c_float * max(1, n_pol))(*[float(x) for x in inv_temps])
        cabi.check(self.lib.ltg_replay_rows(n, k, n_pol, it, f, _ptr(head) if f else None, _ptr(ids), _ptr(logp0), _ptr(reward), _ptr(score),
                                            _ptr(state), _ptr(M), _ptr(rest), _ptr(labels), g, int(labels.numel()), float(clip),
                                            _ptr(row_out), _ptr(w_out), _ptr(first_bad_out), _ptr(logp1_out), self.stream()),
                   "ltg_replay_rows")

    def topk_quota(self, score_all, id_all, score_grp, id_grp, quota, score_out, id_out):
        """the lists with at least quota[j] entries of reserved list j: score_all / id_all [rows, k_in] plain lists, score_grp / id_grp
        [lists, rows, m_in] reserved lists (topk_groups with one bit each), quota a host sequence of `lists` counts -> [rows, k]
        (ltg_topk_quota; the outputs must not alias an input)"""
        n, k_in = (int(x) for x in score_all.shape)
        lists, n_g, m_in = (int(x) for x in score_grp.shape)
        k = int(score_out.shape[1])
        assert n_g == n and tuple(id_all.shape) == (n, k_in) and tuple(id_grp.shape) == (lists, n, m_in) and len(quota) == lists
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, k)
        for t in (score_all, score_grp, score_out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        for t in (id_all, id_grp, id_out):
            assert t.dtype == torch.int32 and t.is_contiguous()
        q = (C.c_int32 * lists)(*[int(x) for x in quota])
        cabi.check(self.lib.ltg_topk_quota(n, k_in, _ptr(score_all), _ptr(id_all), lists, m_in, _ptr(score_grp), _ptr(id_grp), q, k,
                                           _ptr(score_out), _ptr(id_out), self.stream()), "ltg_topk_quota")

    def topk_diversify(self, image, image_lo, score_in, id_in, lam, k, score_out, id_out, stat_out=None):
        """greedy MMR over candidate lists: image [rows, 608] int16 (item_pack; row r = GLOBAL id image_lo + r), score_in / id_in
        [n, c_in] as topk / topk_merge write them, lam in [0, 1] the weight of relevance -> score_out / id_out [n, k] = the picks in
        pick order with their original scores, padded with id -1 / score -inf; stat_out (None, or [n, 2] float32) = the mean pair
        similarity of the first k candidates and of the picks (ltg_topk_diversify; the outputs must not alias an input)"""
        n, c_in = (int(x) for x in score_in.shape)
        assert image.dtype == torch.int16 and image.is_contiguous() and image.dim() == 2 and int(image.shape[1]) == 608
        assert tuple(id_in.shape) == (n, c_in) and tuple(score_out.shape) == tuple(id_out.shape) == (n, int(k))
        for t in (score_in, score_out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        for t in (id_in, id_out):
            assert t.dtype == torch.int32 and t.is_contiguous()
        assert stat_out is None or (stat_out.dtype == torch.float32 and stat_out.is_contiguous() and tuple(stat_out.shape) == (n, 2))
        cabi.check(self.lib.ltg_topk_diversify(_ptr(image), int(image_lo), int(image.shape[0]), n, c_in, _ptr(score_in), _ptr(id_in),
                                               float(lam), int(k), _ptr(score_out), _ptr(id_out), _ptr(stat_out), self.stream()),
                   "ltg_topk_diversify")

    def topk_explain(self, image, image_lo, tr, id_in, top, r, score_out, id_out):
        """why the lists hold their entries: image [rows, 608] int16 (item_pack; row i = GLOBAL id image_lo + i), tr the fold-in rows of
        the same users (a CsrRows with this slab's LOCAL ids), id_in [n, k_in] int32 lists as topk / topk_merge / topk_quota /
        topk_diversify write them -> score_out / id_out [n, top, r]: per entry e < top the r history items of its user nearest to it,
        ordered and padded as item_neighbors writes a list (ltg_topk_explain; an entry outside the image gets r paddings)"""
        n, k_in = (int(x) for x in id_in.shape)
        assert image.dtype == torch.int16 and image.is_contiguous() and image.dim() == 2 and int(image.shape[1]) == 608
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, int(top), int(r))
        assert score_out.dtype == torch.float32 and score_out.is_contiguous()
        for t in (id_in, id_out):
            assert t.dtype == torch.int32 and t.is_contiguous()
        cabi.check(self.lib.ltg_topk_explain(_ptr(image), int(image_lo), int(image.shape[0]), C.byref(tr.c), int(self.item_lo), n, k_in,
                                             _ptr(id_in), int(top), int(r), _ptr(score_out), _ptr(id_out), self.stream()),
                   "ltg_topk_explain")

    def hist_groups(self, tr, labels, n_groups, count_out, hist_lo=None):
        """the class histogram of the histories: tr the fold-in rows (a CsrRows with this slab's LOCAL ids; hist_lo, default this slab's
        item_lo, makes them GLOBAL), labels uint8 per GLOBAL item id -> count_out [rows, n_groups + 1] int32, WRITTEN: the history items
        of every row per class min(label, n_groups) (ltg_hist_groups; an id outside the catalogue counts nowhere)"""
        n = int(count_out.shape[0])
        assert labels.dtype == torch.uint8 and labels.is_contiguous()
        assert count_out.dtype == torch.int32 and count_out.is_contiguous() and tuple(count_out.shape) == (n, int(n_groups) + 1)
        cabi.check(self.lib.ltg_hist_groups(C.byref(tr.c), int(self.item_lo if hist_lo is None else hist_lo), n, _ptr(labels),
                                            int(labels.numel()), int(n_groups), _ptr(count_out), self.stream()), "ltg_hist_groups")

    def topk_calibrate(self, score_grp, id_grp, list_class, n_groups, hist, lam, k, score_out, id_out, stat_out=None):
        """the lists whose class mix follows the histories: score_grp / id_grp [lists, rows, m_in] one topk_groups list per class that
        has one, list_class a host sequence of their classes (strictly ascending, in [0, n_groups]), hist [rows, n_groups + 1] int32 as
        hist_groups writes it, lam in [0, 1] the weight of calibration -> score_out / id_out [rows, k] = the picks in pick order with
        their original scores, padded with id -1 / score -inf; stat_out (None, or [rows, 2] float32) = the miscalibration of the plain
        list and of the output (ltg_topk_calibrate; the outputs must not alias an input)"""
        lists, n, m_in = (int(x) for x in score_grp.shape)
        assert tuple(id_grp.shape) == (lists, n, m_in) and len(list_class) == lists
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, int(k))
        assert hist.dtype == torch.int32 and hist.is_contiguous() and tuple(hist.shape) == (n, int(n_groups) + 1)
        for t in (score_grp, score_out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        for t in (id_grp, id_out):
            assert t.dtype == torch.int32 and t.is_contiguous()
        assert stat_out is None or (stat_out.dtype == torch.float32 and stat_out.is_contiguous() and tuple(stat_out.shape) == (n, 2))
        lc = (C.c_int32 * lists)(*[int(x) for x in list_class])
        cabi.check(self.lib.ltg_topk_calibrate(n, lists, m_in, _ptr(score_grp), _ptr(id_grp), lc, int(n_groups), _ptr(hist), float(lam),
                                               int(k), _ptr(score_out), _ptr(id_out), _ptr(stat_out), self.stream()), "ltg_topk_calibrate")

    def topk_metrics(self, ids, te, labels, n_groups, out, item_hits, k_ndcg=100, k_r1=20, k_r2=50, k_exp=100):
        """the long-tail report of ids [rows, k_in] int32 (as topk / topk_merge write them) against the held-out rows `te` (a CsrRows,
        GLOBAL ids): out [rows, n_groups + 1, 4] float32 = {ndcg, recall@k_r1, recall@k_r2, valid} per item group and for all items
        (labels: uint8 per GLOBAL item id, a label >= n_groups is in no group); item_hits (int32 per GLOBAL item id, or None) gets +1
        for every item among a row's first k_exp ids (ltg_topk_metrics)."""
        n, k_in = (int(x) for x in ids.shape)
        assert ids.dtype == torch.int32 and ids.is_contiguous() and labels.dtype == torch.uint8 and labels.is_contiguous()
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n * (int(n_groups) + 1) * 4
        n_glob = int(labels.numel())
        assert item_hits is None or (item_hits.dtype == torch.int32 and item_hits.is_contiguous() and item_hits.numel() == n_glob)
        cabi.check(self.lib.ltg_topk_metrics(_ptr(ids), n, k_in, C.byref(te.c), _ptr(labels), n_glob, int(n_groups), int(k_ndcg),
                                             int(k_r1), int(k_r2), int(k_exp), _ptr(out), _ptr(item_hits), self.stream()),
                   "ltg_topk_metrics")

    # ------------------------------------------------------------------ item-to-item neighbours
    def item_pack(self, space="decoder", metric="cosine", out=None):
        """this slab's item table (`decoder`: the rows of W_p1t, `encoder`: the rows of W_q0) as the bf16 operand image [I, 608] int16 of
        ltg_item_neighbors (`cosine`: unit rows, `dot`: the rows as they are).  A query image is rows of such an image."""
        if out is None:
            out = torch.empty(self.I, 608, dtype=torch.int16, device=self.device)
        assert out.dtype == torch.int16 and out.is_contiguous() and tuple(out.shape) == (self.I, 608)
        if space == "encoder":
            self.g_flush()               # the lazy clock of W_q0: every row at the current step before it is read
        cabi.check(self.lib.ltg_item_pack(C.byref(self.cfg), C.byref(self.gen_c), cabi.LTG_SPACE[space], cabi.LTG_METRIC[metric], _ptr(out),
                                          self.stream()), "ltg_item_pack")
        return out

    def item_neighbors_ws_bytes(self, n_q, k):
        return int(self.lib.ltg_item_neighbors_ws_bytes(C.byref(self.cfg), int(n_q), int(k)))

    def item_neighbors(self, table_image, q_image, q_gid, k, score_out, id_out, labels=None, group_mask=0x1FF, ws=None):
        """the k nearest items of this slab for every row of q_image [n_q, 608] int16: table_image [I, 608] int16 (item_pack), q_gid [n_q]
        int32 = the GLOBAL id each query must not return (-1: none), labels (uint8 per GLOBAL item id, or None) / group_mask as in
        topk_groups -> score_out [n_q, k] float32, id_out [n_q, k] int32 GLOBAL ids, ordered and padded as topk writes them
        (ltg_item_neighbors).  ws: a uint8 tensor of item_neighbors_ws_bytes(n_q, k) bytes (allocated when absent)."""
        n = int(q_image.shape[0])
        assert table_image.dtype == q_image.dtype == torch.int16 and table_image.is_contiguous() and q_image.is_contiguous()
        assert tuple(table_image.shape) == (self.I, 608) and tuple(q_image.shape) == (n, 608)
        assert q_gid.dtype == torch.int32 and q_gid.is_contiguous() and q_gid.numel() == n
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, k) and score_out.is_contiguous() and id_out.is_contiguous()
        assert score_out.dtype == torch.float32 and id_out.dtype == torch.int32
        assert labels is None or (labels.dtype == torch.uint8 and labels.is_contiguous() and labels.numel() == (self.cfg.n_items_global or self.I))
        need = self.item_neighbors_ws_bytes(n, k) if n else 0
        if ws is None:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        cabi.check(self.lib.ltg_item_neighbors(C.byref(self.cfg), _ptr(table_image), _ptr(q_image), _ptr(q_gid), n, _ptr(labels),
                                               int(group_mask), int(k), _ptr(score_out), _ptr(id_out), _ptr(ws), ws.numel(), self.stream()),
                   "ltg_item_neighbors")

    # ------------------------------------------------------------------ niche companions (the discriminator's pair score)
    def pair_ld(self):
        """floats per row of a side image (ltg_pair_ld: h3 rounded up to a multiple of 4)"""
        ld = int(self.lib.ltg_pair_ld(C.byref(self.cfg)))
        if ld <= 0:
            raise cabi.LtgError("ltg_pair_ld refused the discriminator's layer sizes %r" % ((self.h0, self.h1, self.h2, self.h3),))
        return ld

    def pair_pack(self, side, ids, out=None):
        """the side image of the items `ids` (device int32, rows of the embedding table): side `popular` = branch A, `niche` = branch B of
        the discriminator, from the fp32 master weights -> out [n, pair_ld()] float32, E = exp(2 x) of what the side adds to the fc
        layer's pre-activation (ltg_pair_pack).  Ids outside [0, feature_len) are the caller's to refuse (serving.PairCompanions does)."""
        n, ld = int(ids.numel()), self.pair_ld()
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.dim() == 1
        if out is None:
            out = torch.empty(n, ld, dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, ld)
        if n:
            cabi.check(self.lib.ltg_pair_pack(C.byref(self.cfg), C.byref(self.disc_c), cabi.LTG_PAIR_SIDE[side], _ptr(ids), n, _ptr(out),
                                              self.stream()), "ltg_pair_pack")
        return out

    def pair_companions_ws_bytes(self, n_q, n_c, k):
        return int(self.lib.ltg_pair_companions_ws_bytes(C.byref(self.cfg), int(n_q), int(n_c), int(k)))

    def pair_companions(self, q_image, q_gid, c_image, c_gid, k, score_out, id_out, ws=None):
        """the k best candidates of every query under the discriminator's pair score: q_image [n_q, ld] / c_image [n_c, ld] float32 side
        images of OPPOSITE sides (pair_pack), q_gid [n_q] int32 = the global id a query must not return (-1: none), c_gid [n_c] int32 =
        the candidates' global ids, strictly ascending -> score_out [n_q, k] float32 (the logit: sigmoid gives the discriminator's y
        without dropout), id_out [n_q, k] int32, ordered and padded as topk writes them (ltg_pair_companions).  ws: a uint8 tensor of
        pair_companions_ws_bytes(n_q, n_c, k) bytes (allocated when absent)."""
        n, m, ld = int(q_image.shape[0]), int(c_image.shape[0]), self.pair_ld()
        assert q_image.dtype == c_image.dtype == torch.float32 and q_image.is_contiguous() and c_image.is_contiguous()
        assert tuple(q_image.shape) == (n, ld) and tuple(c_image.shape) == (m, ld)
        for g, cnt in ((q_gid, n), (c_gid, m)):
            assert g.dtype == torch.int32 and g.is_contiguous() and g.numel() == cnt
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, k) and score_out.is_contiguous() and id_out.is_contiguous()
        assert score_out.dtype == torch.float32 and id_out.dtype == torch.int32
        if ws is None:
            ws = torch.empty(max(self.pair_companions_ws_bytes(n, m, k), 1), dtype=torch.uint8, device=self.device)
        cabi.check(self.lib.ltg_pair_companions(C.byref(self.cfg), C.byref(self.disc_c), _ptr(q_image), _ptr(q_gid), n, _ptr(c_image),
                                                _ptr(c_gid), m, int(k), _ptr(score_out), _ptr(id_out), _ptr(ws), ws.numel(), self.stream()),
                   "ltg_pair_companions")

    # ------------------------------------------------------------------ critic-checked lists (the discriminator over a user's anchors x entries)
    def pair_critic(self, pop_image, niche_image, pop_row, niche_row, tr, id_in, top, sum_out, cnt_out, best_s, best_i, hist_lo=None):
        """the discriminator's view of the first `top` entries of the lists id_in [n, k_in] int32: pop_image / niche_image the side images
        (pair_pack) of the popular / niche items with features, pop_row / niche_row [I_global] int32 item id -> image row (-1: not on that
        side), tr the fold-in rows of the same users (a CsrRows with this slab's LOCAL ids; hist_lo, default this slab's item_lo, makes
        them GLOBAL) -> sum_out [n, top] int64 the fixed-point sums of the pair logits over the anchors of these histories, cnt_out [n]
        int32 their number, best_s / best_i [n, top] the best anchor as a length-1 topk list (ltg_pair_critic)"""
        n, k_in = (int(x) for x in id_in.shape)
        ld, top = self.pair_ld(), int(top)
        for img in (pop_image, niche_image):
            assert img.dtype == torch.float32 and img.is_contiguous() and img.dim() == 2 and int(img.shape[1]) == ld
        for m in (pop_row, niche_row):
            assert m.dtype == torch.int32 and m.is_contiguous() and m.numel() == self.I_global
        assert sum_out.dtype == torch.int64 and sum_out.is_contiguous() and tuple(sum_out.shape) == (n, top)
        assert cnt_out.dtype == torch.int32 and cnt_out.is_contiguous() and cnt_out.numel() == n
        assert best_s.dtype == torch.float32 and best_s.is_contiguous() and tuple(best_s.shape) == (n, top)
        for t in (id_in, best_i):
            assert t.dtype == torch.int32 and t.is_contiguous()
        assert tuple(best_i.shape) == (n, top)
        cabi.check(self.lib.ltg_pair_critic(C.byref(self.cfg), C.byref(self.disc_c), _ptr(pop_image), int(pop_image.shape[0]), _ptr(niche_image),
                                            int(niche_image.shape[0]), _ptr(pop_row), _ptr(niche_row), int(self.I_global), C.byref(tr.c),
                                            int(self.item_lo if hist_lo is None else hist_lo), n, k_in, _ptr(id_in), top, _ptr(sum_out),
                                            _ptr(cnt_out), _ptr(best_s), _ptr(best_i), self.stream()), "ltg_pair_critic")

    def critic_finish(self, id_in, top, niche_row, n_niche, sum_in, cnt, crit_out, scored_out):
        """sum_in [n, top] int64 / cnt [n] int32 (pair_critic's, added over the slabs) -> crit_out [n, top] float32 the mean anchor logit of
        every scored entry (0.0 elsewhere), scored_out [n] int32 the scored entries per row (ltg_critic_finish)"""
        n, k_in = (int(x) for x in id_in.shape)
        top = int(top)
        assert id_in.dtype == torch.int32 and id_in.is_contiguous() and niche_row.dtype == torch.int32 and niche_row.is_contiguous()
        assert sum_in.dtype == torch.int64 and sum_in.is_contiguous() and tuple(sum_in.shape) == (n, top)
        assert cnt.dtype == torch.int32 and cnt.is_contiguous() and cnt.numel() == n
        assert crit_out.dtype == torch.float32 and crit_out.is_contiguous() and tuple(crit_out.shape) == (n, top)
        assert scored_out.dtype == torch.int32 and scored_out.is_contiguous() and scored_out.numel() == n
        cabi.check(self.lib.ltg_critic_finish(n, k_in, _ptr(id_in), top, _ptr(niche_row), int(niche_row.numel()), int(n_niche), _ptr(sum_in),
                                              _ptr(cnt), _ptr(crit_out), _ptr(scored_out), self.stream()), "ltg_critic_finish")

    def topk_gate(self, cand_score, cand_id, crit, flag, tau, k, score_out, id_out, stat_out):
        """the gated lists: cand_score / cand_id [n, c_in] as topk / topk_merge write them, crit [n, c_in] float32, flag [n, c_in] int32
        (>= 0: the entry is scored) -> score_out / id_out [n, k] = the first k candidates that are unscored or have crit >= tau, padded
        with id -1 / score -inf; stat_out [n, 3] int32 = scored, rejected before the list was full, length (ltg_topk_gate)"""
        n, c_in = (int(x) for x in cand_score.shape)
        for t in (cand_score, crit, score_out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        for t in (cand_id, flag, id_out, stat_out):
            assert t.dtype == torch.int32 and t.is_contiguous()
        assert tuple(cand_id.shape) == tuple(crit.shape) == tuple(flag.shape) == (n, c_in)
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, int(k)) and tuple(stat_out.shape) == (n, 3)
        cabi.check(self.lib.ltg_topk_gate(n, c_in, _ptr(cand_score), _ptr(cand_id), _ptr(crit), _ptr(flag), float(tau), int(k), _ptr(score_out),
                                          _ptr(id_out), _ptr(stat_out), self.stream()), "ltg_topk_gate")

    # ------------------------------------------------------------------ item audiences
    def item_audience_ws_bytes(self, n_rows, n_q, k):
        return int(self.lib.ltg_item_audience_ws_bytes(C.byref(self.cfg), int(n_rows), int(n_q), int(k)))

    def item_audience(self, logits_or_acts, lse, tr, row_lo, q_col, k, score_out, id_out, ws=None, n_rows=None):
        """the k likeliest rows of this chunk for every query column: logits (an Acts or a [rows, I] float32 tensor) of tr.n_rows rows
        (tr: a CsrRows with LOCAL ids whose fold-in items make a row ineligible for that column, or None; the row count is n_rows if
        given, else tr's, lse's or the logits'), lse [rows] float32 or None (None: the raw logit is the score, else logit - lse), q_col [n_q] int32 LOCAL columns on
        the device -> score_out [n_q, k] float32, id_out [n_q, k] int32 = row_lo + row, ordered and padded as topk writes them
        (ltg_item_audience).  ws: a uint8 tensor of item_audience_ws_bytes(rows, n_q, k) bytes (allocated when absent)."""
        logits = logits_or_acts.logits if isinstance(logits_or_acts, Acts) else logits_or_acts
        n_q = int(q_col.numel())
        n = int(n_rows) if n_rows is not None else int(tr.n_rows) if tr is not None else int(lse.numel()) if lse is not None else int(logits.shape[0])
        assert tr is None or int(tr.n_rows) == n
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= n * self.I
        assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= n)
        assert q_col.dtype == torch.int32 and q_col.is_contiguous() and q_col.dim() == 1
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n_q, k) and score_out.is_contiguous() and id_out.is_contiguous()
        assert score_out.dtype == torch.float32 and id_out.dtype == torch.int32
        need = self.item_audience_ws_bytes(n, n_q, k)
        if ws is None:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        assert ws.dtype == torch.uint8 and ws.numel() >= need
        cabi.check(self.lib.ltg_item_audience(C.byref(self.cfg), _ptr(logits), _ptr(lse), C.byref(tr.c) if tr is not None else None, n,
                                              int(row_lo), _ptr(q_col), n_q, int(k), _ptr(score_out), _ptr(id_out), _ptr(ws), ws.numel(),
                                              self.stream()), "ltg_item_audience")

    def cap_ws_bytes(self, n_rows, c_in, n_items=None):
        """the workspace of the exposure-capped matching of n_rows x c_in candidates over n_items (default: the catalogue) global ids"""
        return int(self.lib.ltg_cap_ws_bytes(int(n_rows), int(c_in), int(self.I_global if n_items is None else n_items)))

    def _cap_check(self, cand_s, cand_i, state, ws, n_items):
        n, c = (int(x) for x in cand_i.shape)
        assert cand_i.dtype == torch.int32 and cand_i.is_contiguous()
        assert cand_s is None or (tuple(cand_s.shape) == (n, c) and cand_s.dtype == torch.float32 and cand_s.is_contiguous())
        assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= cabi.LTG_CAP_STATE
        assert ws.dtype == torch.uint8 and ws.numel() >= self.cap_ws_bytes(n, c, n_items)
        return n, c

    def cap_index(self, cand_i, n_items, state, ws):
        """the start of a matching over the candidates cand_i [rows, c] int32 (GLOBAL ids as topk / topk_merge write them): the per-item
        index into ws, thresholds and state [LTG_CAP_STATE] int32 zeroed (ltg_cap_index)"""
        n, c = self._cap_check(None, cand_i, state, ws, n_items)
        cabi.check(self.lib.ltg_cap_index(n, c, _ptr(cand_i), int(n_items), _ptr(state), _ptr(ws), ws.numel(), self.stream()), "ltg_cap_index")

    def cap_rounds(self, cand_s, cand_i, lse, cap, k, n_rounds, state, ws):
        """n_rounds propose / accept rounds of the matching cap_index started: cand_s [rows, c] float32 logits, lse [rows] float32 or None
        (None: items rank users by the logit, else by logit - lse), cap [n_items] int32 per GLOBAL id (ltg_cap_rounds).  Converged when
        state[4] < state[1]: the last round raised no threshold."""
        n, c = self._cap_check(cand_s, cand_i, state, ws, int(cap.numel()))
        assert cap.dtype == torch.int32 and cap.is_contiguous()
        assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= n)
        cabi.check(self.lib.ltg_cap_rounds(n, c, _ptr(cand_s), _ptr(cand_i), _ptr(lse), _ptr(cap), int(cap.numel()), int(k), int(n_rounds),
                                           _ptr(state), _ptr(ws), ws.numel(), self.stream()), "ltg_cap_rounds")

    def cap_finish(self, cand_s, cand_i, n_items, k, score_out, id_out, state, ws):
        """the lists of the matching as it stands: score_out / id_out [rows, k] = every row's active entries in candidate order with
        their original logits, padded with id -1 / score -inf; state[2] / state[3] = entries passed over / short lists (ltg_cap_finish)"""
        n, c = self._cap_check(cand_s, cand_i, state, ws, n_items)
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, int(k)) and score_out.is_contiguous() and id_out.is_contiguous()
        assert score_out.dtype == torch.float32 and id_out.dtype == torch.int32
        cabi.check(self.lib.ltg_cap_finish(n, c, _ptr(cand_s), _ptr(cand_i), int(n_items), int(k), _ptr(score_out), _ptr(id_out), _ptr(state),
                                           _ptr(ws), ws.numel(), self.stream()), "ltg_cap_finish")

    def share_ws_bytes(self, n_rows, k):
        """the workspace of the share-targeted lists of n_rows rows of k entries (0 for sizes ltg_topk_share refuses)"""
        return int(self.lib.ltg_share_ws_bytes(int(n_rows), int(k)))

    def topk_share(self, score_pro, id_pro, score_rest, id_rest, k, want, score_out, id_out, state, ws):
        """the lists in which the promoted lists hold `want` of all slots, placed where they cost the least score: score_pro / id_pro and
        score_rest / id_rest [rows, m_in] as topk_groups writes them with a group mask and with its complement -> score_out / id_out
        [rows, k], every row sorted as topk sorts, every entry with its original score; state [LTG_SHARE_STATE] int32 = {promoted entries
        of the plain lists, steps there are, steps taken, rows changed, bits of the threshold cost, entries served, 0, 0}
        (ltg_topk_share: one call, no read-back; the outputs must not alias an input)"""
        n, m_in = (int(x) for x in score_pro.shape)
        for t in (id_pro, score_rest, id_rest):
            assert tuple(t.shape) == (n, m_in)
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, int(k))
        for t in (score_pro, score_rest, score_out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        for t in (id_pro, id_rest, id_out):
            assert t.dtype == torch.int32 and t.is_contiguous()
        assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= cabi.LTG_SHARE_STATE
        assert ws.dtype == torch.uint8 and ws.numel() >= self.share_ws_bytes(n, k)
        cabi.check(self.lib.ltg_topk_share(n, m_in, _ptr(score_pro), _ptr(id_pro), _ptr(score_rest), _ptr(id_rest), int(k), int(want),
                                           _ptr(score_out), _ptr(id_out), _ptr(state), _ptr(ws), ws.numel(), self.stream()), "ltg_topk_share")

    def floor_ws_bytes(self, n_rows, c_in, n_items=None):
        """the workspace of the exposure-floor matching of n_rows x c_in candidates over n_items (default: the catalogue) global ids"""
        return int(self.lib.ltg_floor_ws_bytes(int(n_rows), int(c_in), int(self.I_global if n_items is None else n_items)))

    def _floor_check(self, cand_s, cand_i, lse, need, state, ws, n_items):
        n, c = (int(x) for x in cand_i.shape)
        assert cand_i.dtype == torch.int32 and cand_i.is_contiguous()
        assert cand_s is None or (tuple(cand_s.shape) == (n, c) and cand_s.dtype == torch.float32 and cand_s.is_contiguous())
        assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= n)
        assert need is None or (need.dtype == torch.int32 and need.is_contiguous())
        assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= cabi.LTG_FLOOR_STATE
        assert ws.dtype == torch.uint8 and ws.numel() >= self.floor_ws_bytes(n, c, n_items)
        return n, c

    def floor_index(self, cand_i, n_items, state, ws):
        """the start of a floor matching over the candidates cand_i [rows, c] int32 (GLOBAL ids as topk / topk_merge write them): the
        per-item index into ws, the limits at c - 1 and state [LTG_FLOOR_STATE] int32 zeroed (ltg_floor_index)"""
        n, c = self._floor_check(None, cand_i, None, None, state, ws, n_items)
        cabi.check(self.lib.ltg_floor_index(n, c, _ptr(cand_i), int(n_items), _ptr(state), _ptr(ws), ws.numel(), self.stream()),
                   "ltg_floor_index")

    def floor_rounds(self, cand_s, cand_i, lse, need, k, reserve, n_rounds, state, ws):
        """n_rounds item / user rounds of the matching floor_index started: cand_s [rows, c] float32 logits, lse [rows] float32 or None
        (None: items rank users by the logit, else by logit - lse), need [n_items] int32 per GLOBAL id (0: no floor), reserve: the slots at
        the end of a list that floor items may take (ltg_floor_rounds).  Converged when state[4] < state[1]: the last round lowered no limit."""
        n, c = self._floor_check(cand_s, cand_i, lse, need, state, ws, int(need.numel()))
        cabi.check(self.lib.ltg_floor_rounds(n, c, _ptr(cand_s), _ptr(cand_i), _ptr(lse), _ptr(need), int(need.numel()), int(k), int(reserve),
                                             int(n_rounds), _ptr(state), _ptr(ws), ws.numel(), self.stream()), "ltg_floor_rounds")

    def floor_finish(self, cand_s, cand_i, lse, need, k, reserve, score_out, id_out, state, ws, active_out=None, held_out=None):
        """the lists of the matching as it stands: score_out / id_out [rows, k] = every row's first k - t candidates, then its t active
        entries behind them, each with its original logit; active_out [rows, c] uint8 or None: the matching itself; held_out [n_items]
        int32 or None: the active entries per item; state[2], [3], [5], [6] = items short of their floor / rows changed / inserted slots /
        floor items (ltg_floor_finish)"""
        n, c = self._floor_check(cand_s, cand_i, lse, need, state, ws, int(need.numel()))
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, int(k)) and score_out.is_contiguous() and id_out.is_contiguous()
        assert score_out.dtype == torch.float32 and id_out.dtype == torch.int32
        assert active_out is None or (tuple(active_out.shape) == (n, c) and active_out.dtype == torch.uint8 and active_out.is_contiguous())
        assert held_out is None or (held_out.numel() >= need.numel() and held_out.dtype == torch.int32 and held_out.is_contiguous())
        cabi.check(self.lib.ltg_floor_finish(n, c, _ptr(cand_s), _ptr(cand_i), _ptr(lse), _ptr(need), int(need.numel()), int(k), int(reserve),
                                             _ptr(score_out), _ptr(id_out), _ptr(active_out), _ptr(held_out), _ptr(state), _ptr(ws),
                                             ws.numel(), self.stream()), "ltg_floor_finish")

    # ------------------------------------------------------------------ views in the reference's shapes
    def generator_params_tf(self):
        """The 8 tensors in the reference's order and TF shapes (MultiVAE.py:129-141); W_p1 is a
        transposed view of the item-major storage."""
        self.g_flush()
        p = self.g_p
        return [p[0], p[1], p[2], p[3].t(), p[4], p[5], p[6], p[7]]

    def discriminator_params_tf(self):
        p = self.d_p
        return [p[0], p[1], p[2], p[3], p[4], p[5], p[6].reshape(-1, 1), p[7]]
