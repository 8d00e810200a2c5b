"""Shared builders for the parity tests: seeded problem instances in the oracle's (TF) layout and
the engine's layout, CSR/CSC construction, RNG-derived random tensors."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle import ltg_oracle as O


def random_history(rng, n_rows, n_items, mean_nnz=18, min_nnz=1):
    rows, cols = [], []
    for b in range(n_rows):
        k = int(min(n_items, max(min_nnz, rng.poisson(mean_nnz))))
        it = rng.choice(n_items, size=k, replace=False)
        rows += [b] * k
        cols += sorted(it.tolist())
    X = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_rows, n_items))
    X.sort_indices()
    return X


# Rows the long-tail builder always holds (when they fit in n_items): either side of the kernels' row thresholds -- NT = 256 entries (the
# strided row loops' second pass), ENC_NT = 1 024 (fk_enc0_fwd's second chunk) -- and one of ~2 500 entries (three chunks)
LONG_TAIL_ROWS = (1, 255, 256, 257, 1023, 1024, 1025, 2500)


def skewed_history(rng, n_rows, n_items, values=False):
    """A sorted CSR batch shaped like the data the model is for: item popularity Zipf(s = 1) (item 0 the most popular, and in EVERY row),
    row lengths max(1, round(LogNormal(2.2, 0.9))) clipped to n_items, plus rows of exactly LONG_TAIL_ROWS entries where they fit (a
    longer one is dropped), at random positions.  The items of a row are drawn by popularity without replacement (Gumbel top-k).
    values=True: entries from {0.5, 1, 2, 3, 5} instead of 1 (the product uploads `values` for any non-binary history)."""
    L = np.minimum(np.maximum(1, np.rint(rng.lognormal(2.2, 0.9, n_rows))).astype(np.int64), n_items)
    forced = [k for k in LONG_TAIL_ROWS if k <= n_items][:n_rows]
    L[rng.permutation(n_rows)[:len(forced)]] = forced
    logw = -np.log(np.arange(2, n_items + 1, dtype=np.float64))      # items 1 .. n_items - 1
    indptr, cols = [0], []
    for k in L.tolist():
        it = np.zeros(0, np.int64)
        if k > 1:
            g = logw - np.log(-np.log(rng.random(n_items - 1)))
            it = (np.arange(n_items - 1) if k - 1 == n_items - 1 else np.argpartition(-g, k - 1)[:k - 1]) + 1
        cols.append(np.sort(np.concatenate([[0], it])))
        indptr.append(indptr[-1] + k)
    cols = np.concatenate(cols).astype(np.int32)
    data = (rng.choice(np.array([0.5, 1.0, 2.0, 3.0, 5.0], np.float32), size=len(cols)) if values else np.ones(len(cols), np.float32))
    X = sp.csr_matrix((data, cols, np.array(indptr, np.int64)), shape=(n_rows, n_items))
    assert X.has_sorted_indices
    return X


def skewed_fake_pairs(rng, X, n_items):
    """(row, gen, pop) triples sorted by row whose per-user count follows the history: a user of n entries gets n .. n + n/4 + 1 pairs
    (capped at n_items), users of fewer than 256 entries none with probability 0.1; gen distinct within a row, ~5 % holes (-1)."""
    rows, gen, pop = [], [], []
    for b, n in enumerate(np.diff(X.indptr).tolist()):
        if n < 256 and rng.random() < 0.1:
            continue
        k = min(n_items, n + int(rng.integers(0, n // 4 + 2)))
        g = np.sort(rng.choice(n_items, size=k, replace=False))
        p = rng.integers(0, n_items, k)
        hole = rng.random(k) < 0.05
        rows.append(np.full(k, b))
        gen.append(np.where(hole, -1, g))
        pop.append(np.where(hole, -1, p))
    cat = lambda a: np.concatenate(a).astype(np.int32) if a else np.zeros(0, np.int32)
    return cat(rows), cat(gen), cat(pop)


def long_tail_batch(n_items, B, values=False):
    """Batch 1 of a two-batch skewed history, seeded by the shape, as the parity tests feed it: (X_all [2 B, n_items], X = rows [B, 2 B)
    -- the batch --, fake pairs of the batch with LOCAL rows).  Batch 0 is skewed too, so that batch 1's rows, entries and distinct items
    start at non-zero offsets of every device array."""
    rng = np.random.default_rng(13 * n_items + B + (1 if values else 0))
    X_all = sp.vstack([skewed_history(rng, B, n_items, values), skewed_history(rng, B, n_items, values)]).tocsr()
    X_all.sort_indices()
    X = X_all[B:2 * B].tocsr()
    return X_all, X, skewed_fake_pairs(rng, X, n_items)


def device_batch(X_all, B, device, b=1):
    """view(b)["batch"] of DeviceData over an IndexData of X_all (no sampler lists): the batch exactly as training hands it to the kernels --
    uitem, row_norm2, values when not binary, non-zero row / entry / uptr offsets.  Returns (DeviceData, CsrRows); keep the first alive."""
    from ltgan.dataset import DeviceData, IndexData
    idx = IndexData(X_all.shape[1], X_all, 0, {}, {}, {}, {}, {}, range(X_all.shape[1]))
    dd = DeviceData(idx, B, device)
    return dd, dd.view(b)["batch"]


def csc_view(X):
    """(slot, uptr, rowidx, csr_pos, n_unique) of a CSR matrix: the transposed view ltg_g_step needs."""
    from ltgan.dataset import batch_csc
    X = X.tocsr()
    slot, uptr, rowidx, pos = batch_csc(X, 0, X.shape[0], X.shape[1])
    return slot, uptr, rowidx, pos, len(uptr) - 1


def dropout_mask_dense(seed, step, n_rows, n_items, keep):
    idx = (np.arange(n_rows, dtype=np.uint64)[:, None] * np.uint64(n_items) + np.arange(n_items, dtype=np.uint64)[None, :])
    return (O.rng_uniform(seed, O.STREAM_VAE_DROPOUT, step, idx).astype(np.float32) < np.float32(keep)).astype(np.float64)


def eps_dense(seed, step, n_rows, Z):
    idx = np.arange(n_rows * Z, dtype=np.uint64).reshape(n_rows, Z)
    return O.rng_normal(seed, O.STREAM_VAE_EPS, step, idx)


def d_masks(seed, step, n, widths, keep):
    out = []
    for stream, w in zip((O.STREAM_D_DROP_A, O.STREAM_D_DROP_B, O.STREAM_D_DROP_C), widths):
        idx = np.arange(n * w, dtype=np.uint64).reshape(n, w)
        out.append((O.rng_uniform(seed, stream, step, idx).astype(np.float32) < np.float32(keep)).astype(np.float64))
    return out


def gen_to_engine(P):
    """oracle dict (TF shapes) -> engine layout list."""
    return [P["Wq0"], P["Wq1"], P["Wp0"], np.ascontiguousarray(P["Wp1"].T), P["bq0"], P["bq1"], P["bp0"], P["bp1"]]


def engine_to_gen(arrs):
    a = [np.asarray(x) for x in arrs]
    return {"Wq0": a[0], "Wq1": a[1], "Wp0": a[2], "Wp1": np.ascontiguousarray(a[3].T), "bq0": a[4], "bq1": a[5],
            "bp0": a[6], "bp1": a[7]}


def disc_to_engine(D):
    return D["emb"], [D[k] for k in O.D_KEYS]


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- hot parameter sets: the dynamic range of a trained model (tests/test_hot_params_cpu.py pins what they give; tests/test_gpu_hot_range.py
# holds the kernels to the oracle on them).  Xavier logits span +-2 of a row and no tanh passes 0.99: exp(m_old - m_new) is ~1 at every merge.
HOT_SEED = 1234                       # the engine seed of the GPU tests (dropout / epsilon counters)
HOT_PROFILES = ("spike-last", "ramp-up", "ramp-down", "dead-tile")
# W_p1 factor per profile, times sqrt((600 + I) / 1600) (Xavier's limit is sqrt(6 / (600 + I)): the factor keeps the per-row spread of the
# logits the same at every I).  One factor for all four profiles cannot meet the conditions of test_hot_params_cpu: with sigma the
# per-row standard deviation of h2 . W_p1 (0.71 per unit of the factor), "spike-last" needs 0.1 % of a row 87 below its maximum from
# sigma alone (sigma >= 14, and 0.1 % only from 14.5 at 1 000 items), the ramps add 60 to that spread (10 % pass 87 from sigma = 9), and
# "dead-tile" (170 of range from the bias) must stay inside 250 (sigma <= 13)
HOT_WP1 = {"spike-last": 21.0, "ramp-up": 10.0, "ramp-down": 10.0, "dead-tile": 17.5}
DEAD_TILE = (64, 96)                  # bp1[64:96] -= 120: one whole 32-item tile of the streaming kernels


def hot_bias(I, profile):
    """what the profile adds to bp1 (fp64 [I])"""
    assert profile in HOT_PROFILES and I >= 128
    i = np.arange(I, dtype=np.float64)
    b = np.zeros(I)
    if profile in ("spike-last", "dead-tile"):
        b[I - 3] += 20.0              # the row maximum in the ragged last tile (I % 32 = 8 at 1 000 / 8 200 / 25 032 / 65 544 items)
    if profile == "ramp-up":
        b += 60.0 * i / I             # every tile raises the running maximum
    if profile == "ramp-down":
        b += 60.0 * (I - 1 - i) / I   # the first tile fixes the maximum, later tiles underflow against it
    if profile == "dead-tile":
        b[DEAD_TILE[0]:DEAD_TILE[1]] -= 120.0     # exp(x - m) = 0 in fp32 for the whole tile
        b[5] -= 150.0
    return b


def hot_generator(P, profile):
    """A copy of an O.init_generator set at a trained model's range: W_q0 x 12 r, W_q1 x 2, W_p0 x 2 (r = sqrt(I / 1000)), W_p1 x
    HOT_WP1[profile] sqrt((600 + I) / 1600), bp1 += hot_bias.  The oracle is finite everywhere with it."""
    I = P["Wp1"].shape[1]
    r = np.sqrt(I / 1000.0)
    Q = {k: np.array(v, dtype=np.float32, copy=True) for k, v in P.items()}
    Q["Wq0"] *= np.float32(12.0 * r)
    Q["Wq1"] *= np.float32(2.0)
    Q["Wp0"] *= np.float32(2.0)
    Q["Wp1"] *= np.float32(HOT_WP1[profile] * np.sqrt((600.0 + I) / 1600.0))
    Q["bp1"] = (Q["bp1"].astype(np.float64) + hot_bias(I, profile)).astype(np.float32)
    return Q


def hot_discriminator(D):
    """A copy of an O.init_discriminator set with emb, w1 .. w4 x 2 (biases stay 0): scores to +-8, a few per cent of the fc layer's tanh
    above 0.99.  Not x 3: there fp32's own 1 - y costs 8e-2 on a row's -log(1 - y), oracle against oracle."""
    Q = {k: np.array(v, dtype=np.float32, copy=True) for k, v in D.items()}
    for k in ("emb", "w1", "w2", "w3", "w4"):
        Q[k] *= np.float32(2.0)
    return Q


def hot_problem(I, B, profile, seed):
    """(rng, X, P) as the parity tests' _problem(I, B, seed) builds them, P made hot"""
    rng = np.random.default_rng(seed)
    X = random_history(rng, B, I)
    return rng, X, hot_generator(O.init_generator(I, seed=seed + 1), profile)


def hot_fake_pairs(rng, X, I, per_user=5):
    """(row, gen, pop) sorted by row, gen ascending and distinct within a row, ~5 % holes -- and in every fourth user's list a pair on item I - 3
    (the spike: a probability near 1), on an item of DEAD_TILE and on item 5 (probabilities that are 0 in fp32 under "dead-tile")"""
    rows, gen, pop = [], [], []
    for b in range(X.shape[0]):
        if b % 4 and rng.random() < 0.1:
            continue
        g = set(rng.choice(I, size=int(rng.integers(1, per_user + 1)), replace=False).tolist())
        if b % 4 == 0:
            g |= {I - 3, DEAD_TILE[0] + (7 * b) % (DEAD_TILE[1] - DEAD_TILE[0]), 5}
        for gi in sorted(g):
            hole = gi not in (I - 3, 5) and rng.random() < 0.05
            rows.append(b)
            gen.append(-1 if hole else int(gi))
            pop.append(-1 if hole else int(rng.integers(0, I)))
    return np.array(rows, np.int32), np.array(gen, np.int32), np.array(pop, np.int32)


# ---- the stage comparators of tests/test_gpu_hot_range.py (each stage is fed what the DEVICE produced in the stage before it: with hot
# parameters the fp32 oracle itself is 1e-3 off the fp64 oracle on probabilities end to end, so an end-to-end bound says nothing)
ACC_K = 600                           # products per logit (h_enc)


def logits_ratio(got, h2, Wp1, bp1):
    """stage (b): the worst |got - want| / bound, element-wise, want = the fp64 product of the operands as given plus the bias, bound =
    (ACC_K + 1) 2^-23 (sum_k |a_k b_k| + |bias|) -- what ACC_K fp32 accumulations of exact products and the bias add can lose (the form of
    neighbors_ref.score_bound).  Returns (ratio, where)."""
    a, w = np.asarray(h2, np.float64), np.asarray(Wp1, np.float64)
    b = np.asarray(bp1, np.float64)
    want = a @ w + b
    bound = (ACC_K + 1) * 2.0 ** -23 * (np.abs(a) @ np.abs(w) + np.abs(b))
    ratio = np.abs(np.asarray(got, np.float64) - want) / bound
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), at


def check_logits(got, h2, Wp1, bp1):
    ratio, at = logits_ratio(got, h2, Wp1, bp1)
    assert ratio <= 1.0, ("logits", at, ratio)
    return ratio


def lse64(logits):
    x = np.asarray(logits, np.float64)
    m = x.max(1)
    return m + np.log(np.exp(x - m[:, None]).sum(1))


def lse_bound(logits):
    """stage (c)'s bound per row, from the reference alone: 8 x the worst gap between the oracle's log-sum-exp at float32 and at float64 on
    THESE logits (the device sums in another order than numpy's pairwise one), never below 2 ulp of the lse.  Returns (lse64, bound, gap)."""
    want = lse64(logits)
    x = np.asarray(logits, np.float32)
    m = x.max(1, keepdims=True)
    with np.errstate(under="ignore"):
        l32 = (m + np.log(np.exp(x - m).sum(1, keepdims=True)))[:, 0]
    assert l32.dtype == np.float32
    gap = float(np.abs(l32.astype(np.float64) - want).max())
    return want, np.maximum(8.0 * gap, 2.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)), gap


def lse_ratio(got, logits, extra=0.0):
    """stage (c): the worst |got - lse64(logits)| / (lse_bound + extra).  Returns (ratio, row, error, bound, the fp32 gap)."""
    want, bound, gap = lse_bound(logits)
    g = np.asarray(got, np.float64)
    err = np.where(np.isfinite(g), np.abs(g - want), np.inf)
    r = int(np.argmax(err / (bound + extra)))
    return float(err[r] / (bound[r] + extra)), r, float(err[r]), float(bound[r] + extra), gap


def check_lse(got, logits, extra=0.0):
    ratio, r, err, bound, gap = lse_ratio(got, logits, extra)
    assert ratio <= 1.0, ("lse row", r, err, bound)
    return err, bound, gap


def probs_ratio(got, logits, lse):
    """stage (d): p against exp(logit - lse) in fp64.  Where that is >= 2^-100: relative error <= (|logit - lse| + 8) 2^-23 -- the subtraction
    and the x log2(e) product round once each (|x| 2^-24 relative after the exponential, each), a few ulp for the exponential itself.  Below:
    0 <= p <= 2^-99.  Returns (the worst error / bound of the first kind, where, whether all of the second kind are in range)."""
    x = np.asarray(logits, np.float64) - np.asarray(lse, np.float64)[:, None]
    want = np.exp(x)
    p = np.asarray(got, np.float64)
    big = want >= 2.0 ** -100
    small_ok = bool(np.all(p[~big] >= 0.0) and np.all(p[~big] <= 2.0 ** -99))
    ratio = np.where(big, np.abs(p - want) / np.where(big, want, 1.0) / ((np.abs(x) + 8.0) * 2.0 ** -23), 0.0)
    ratio = np.where(np.isfinite(p), ratio, np.inf)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), at, small_ok


def check_probs(got, logits, lse):
    ratio, at, small_ok = probs_ratio(got, logits, lse)
    assert small_ok, "a probability below 2^-100 is negative or above 2^-99"
    assert ratio <= 1.0, ("probs", at, ratio)
    return ratio


# ---- the cases of tests/test_gpu_hot_range.py, shared with tests/test_hot_params_cpu.py (which pins the oracle's range on every one of them).
# Forward: (I, B, precision, tuning knob, profiles) -- the smallest item counts that reach each kernel
_TWO = ("ramp-up", "dead-tile")
HOT_FWD = [(1000, 100, "fp32", 0, HOT_PROFILES), (1000, 100, "bf16", 0, HOT_PROFILES),      # small slab
           (1000, 100, "bf16", 1 << 18, HOT_PROFILES),                                        # the generic kernels
           (4096, 37, "bf16", 0, _TWO),                                                       # the largest small slab
           (6000, 64, "bf16", 0, _TWO),                                                       # middle-layer fast path without streaming
           (8200, 100, "fp32", 0, HOT_PROFILES), (8200, 100, "bf16", 0, HOT_PROFILES),        # first streaming form, ragged tail
           (8200, 150, "bf16", 0, HOT_PROFILES),                                              # more than 112 rows
           (25032, 128, "bf16", 0, _TWO),                                                     # ragged slab, 7 segments of 4 096
           (8200, 100, "bf16", 1 << 17, HOT_PROFILES), (25032, 16, "bf16", 1 << 17, _TWO),    # the second streaming form, forced
           (65544, 16, "bf16", 0, _TWO)]                                                      # ... chosen by the library itself
HOT_FWD_STEP, HOT_KEEP = 7, 0.75
HOT_SPAN = (8200, (100, 100, 50), "dead-tile", 21)          # rows_per_step: I, rows of the batches, profile, rng_step
# G step: (precision, I, B, path, warm); both _TWO profiles each
HOT_G = [("fp32", 1000, 100, "step", False), ("bf16", 1000, 100, "step", False), ("bf16", 1000, 100, "step-generic", False),
         ("bf16", 6000, 100, "step", False), ("fp32", 8200, 100, "step", False), ("bf16", 8200, 100, "step", False),
         ("bf16", 25032, 100, "one-call", False), ("bf16", 8200, 100, "step", True), ("bf16", 25032, 100, "one-call", True)]
HOT_G_STEP = 3


def hot_forward_inputs(I, B, profile, step=HOT_FWD_STEP, is_training=1.0, seed=None):
    """(X, P, dropout mask, eps) of a forward case: _problem's seed I + B unless given"""
    _, X, P = hot_problem(I, B, profile, I + B if seed is None else seed)
    eps = eps_dense(HOT_SEED, step, B, O.Z_DIM) if is_training else np.zeros((B, O.Z_DIM))
    return X, P, dropout_mask_dense(HOT_SEED, step, B, I, HOT_KEEP), eps


# ---- item slabs in one process (tests/test_gpu_item_slabs.py): every rank of an item-sharded run as an engine of its own on one device, the
# exchanges done by hand in rank order.  Cut-point G step: (precision, I, B, R, history, warm) -- the smallest shapes that reach each route
# (tests/test_routes_cpu.py has every slab's)
SLAB_G = [(p, 1000, 100, 2, "skewed", False) for p in ("fp32", "bf16")] + \
    [(p, 8200, 100, 2, "uniform", False) for p in ("fp32", "bf16")] + \
    [("fp32", 1101, 37, 9, "uniform", False),
     ("bf16", 16520, 100, 2, "uniform", False), ("bf16", 16520, 100, 2, "uniform", True), ("bf16", 25032, 128, 3, "skewed", False)]


def slab_cuts(I, R):
    """[(item_lo, item_hi)] of the R ranks, as ShardedTrainer's callers cut them"""
    from ltgan.sharded import item_slab
    return [item_slab(I, r, R) for r in range(R)]


def slab_edges(cuts):
    """the items either side of every rank boundary, and the first and the last item"""
    I = cuts[-1][1]
    return sorted({0, I - 1} | {c + d for c, _ in cuts[1:] for d in (-1, 0)})


def with_edge_history(X, row, cols, bare=None):
    """X (binary CSR) with entries at `cols` of `row` as well; bare = (row, lo, hi): and that row without its entries in columns [lo, hi)"""
    X = X.tolil()
    for c in cols:
        X[row, c] = 1.0
    if bare is not None:
        X[bare[0], bare[1]:bare[2]] = 0.0
    X = X.tocsr()
    X.eliminate_zeros()
    X.sort_indices()
    assert X.getnnz(axis=1).min() > 0
    return X


def with_edge_pairs(rows, gen, pop, edges, B, I):
    """the (row, gen, pop) triples plus a pair on every item of `edges`, the k-th in row (7 k + 1) % B unless that row generates the item
    already; rows stay sorted, gen distinct and ascending within a row (a row's holes first)"""
    add = [((7 * k + 1) % B, g) for k, g in enumerate(edges)]
    add = [(r, g) for r, g in add if not np.any((rows == r) & (gen == g))]
    rows = np.concatenate([rows, [r for r, _ in add]]).astype(np.int32)
    gen = np.concatenate([gen, [g for _, g in add]]).astype(np.int32)
    pop = np.concatenate([pop, [(31 * g + 5) % I for _, g in add]]).astype(np.int32)
    order = np.lexsort((gen, rows))
    return rows[order], gen[order], pop[order]


def sum_in_rank_order(parts):
    """((0 + x_0) + x_1) + ... in fp32 on the device: the all-reduce of _rccl.HostComm(ordered=True)"""
    import torch
    acc = torch.zeros_like(parts[0])
    for x in parts:
        acc += x
    return acc


SLAB_TENSORS = (0, 3, 7)              # W_q0, W_p1t, b_p1: a rank owns its slab's rows; every other tensor is replicated


class SlabRig:
    """The R ranks of an item-sharded run over batch b of X_all as R engines in ONE process: Engine(I, item_lo, item_hi) and DeviceData(idx, B,
    item_lo, item_hi) per rank over the same IndexData (the batch carries the full row's row_norm2, uitem, the CSC view, non-zero offsets --
    what training hands over), the same parameters, moments, seed and Adam counter everywhere.  No torch.distributed: the three exchanges
    are sums / concatenations in rank order on the device."""

    def __init__(self, X_all, B, b, R, engine, P, D=None, m=None, v=None, adam_t=0):
        """engine(item_lo, item_hi) -> Engine; P / m / v: generator arrays in engine layout over ALL items (set_generator cuts them); D = (emb,
        arrays) of set_discriminator; b = (b0, b1): the span of batches [b0, b1) as phase C feeds it (forward only)"""
        from ltgan.dataset import IndexData
        I = X_all.shape[1]
        self.I, self.B, self.R, self.cuts = I, B, R, slab_cuts(I, R)
        self.idx = IndexData(I, X_all, 0, {}, {}, {}, {}, {}, range(I))
        self.b = b
        self._start = (engine, P, D, m, v, adam_t)
        self.ranks = [self.rank(r) for r in range(R)]
        self.record = None

    def rank(self, r):
        """(Engine, DeviceData, batch, Acts) of rank r in the start state; a fresh set every call"""
        from ltgan.dataset import DeviceData
        engine, P, D, m, v, adam_t = self._start
        lo, hi = self.cuts[r]
        eng = engine(lo, hi)
        eng.set_generator(P, m=m, v=v)
        if D is not None:
            eng.set_discriminator(*D)
        eng.adam_t = adam_t
        dd = DeviceData(self.idx, self.B, eng.device, item_lo=lo, item_hi=hi)
        batch = (dd.span(*self.b) if isinstance(self.b, tuple) else dd.view(self.b))["batch"]
        return eng, dd, batch, eng.new_acts(batch.n_rows)

    def forward(self, fopts, fake=None):
        """g_fwd_enc on every rank, h1 summed in rank order into every rank's acts, g_fwd_rest: the [R B 5] row partials in rank order"""
        import torch
        n = self.ranks[0][2].n_rows
        for eng, _, batch, acts in self.ranks:
            eng.g_fwd_enc(batch, acts, fopts(eng))
        h1 = [acts.h1[:n].clone() for _, _, _, acts in self.ranks]
        h1_all = sum_in_rank_order(h1)
        parts = []
        for eng, _, batch, acts in self.ranks:
            acts.h1[:n].copy_(h1_all)
            rp = torch.zeros(n * 5, dtype=torch.float32, device=eng.device)
            eng.g_fwd_rest(batch, fake, acts, fopts(eng), rp)
            parts.append(rp)
        return h1, h1_all, parts, torch.cat(parts)

    def g_step(self, fake, cnt, anneal, lam, keep, dkeep, step, dstep):
        """ShardedTrainer._g_one's cut-point sequence with the overlaps off, all ranks in lock step.  Leaves self.record = the ranks'
        contributions to the three exchanges and the three totals; returns every rank's loss_out."""
        import torch
        B, R = self.B, self.R
        gos = {id(eng): eng.g_opts(cnt, anneal, lam, keep, 1.0, dkeep, step, dstep) for eng, _, _, _ in self.ranks}
        h1, h1_all, parts, rp_all = self.forward(lambda eng: gos[id(eng)].fwd, fake)
        losses, dh2 = [], []
        for eng, _, batch, acts in self.ranks:
            loss = torch.zeros(8, dtype=torch.float32, device=eng.device)
            d = torch.zeros(B, eng.H, dtype=torch.float32, device=eng.device)
            eng.g_bwd_dec(batch, fake, acts, gos[id(eng)], rp_all, R, loss, d)
            losses.append(loss)
            dh2.append(d)
        dh2_all = sum_in_rank_order(dh2)
        for eng, _, batch, acts in self.ranks:
            eng.g_bwd_dec1(batch, fake, acts, gos[id(eng)])
            eng.g_bwd_rest(batch, fake, acts, gos[id(eng)], dh2_all)
        for eng, _, _, _ in self.ranks:
            eng.g_flush()
        torch.cuda.synchronize()
        self.record = dict(h1=h1, rowpart=parts, dh2=dh2, h1_all=h1_all, rowpart_all=rp_all, dh2_all=dh2_all)
        return losses

    @staticmethod
    def assemble(engines, losses):
        """(p, m, v as lists of eight numpy arrays over ALL items, loss) of the model the ranks hold together.  The replica invariant first:
        every rank's copy of a replicated tensor, of its moments and of loss_out[0:6] equals rank 0's bit for bit."""
        import torch
        e0 = engines[0]
        for r, e in enumerate(engines[1:], 1):
            for i in range(8):
                if i not in SLAB_TENSORS:
                    for what, a, b in (("p", e0.g_p[i], e.g_p[i]), ("m", e0.g_m[i], e.g_m[i]), ("v", e0.g_v[i], e.g_v[i])):
                        assert torch.equal(a, b), ("replica", what, i, "rank", r, float((a - b).abs().max()))
            assert torch.equal(losses[0][:6], losses[r][:6]), ("replica loss, rank", r, losses[0][:6].tolist(), losses[r][:6].tolist())
        out = []
        for ts in ([e.g_p for e in engines], [e.g_m for e in engines], [e.g_v for e in engines]):
            out.append([(torch.cat([t[i] for t in ts]) if i in SLAB_TENSORS else ts[0][i]).cpu().numpy() for i in range(8)])
        return out[0], out[1], out[2], losses[0].cpu().numpy()
