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
