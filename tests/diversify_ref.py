"""numpy reference of the diversified top-K lists (ltg_topk_diversify; include/ltg.h): greedy maximal marginal relevance over sorted
candidate lists, stated literally, plus the inputs the exact-parity tests share.  Similarities come from neighbors_ref.scores64 /
score_bound on image rows."""
import numpy as np

import neighbors_ref as NR


def valid_counts(ids, image_lo, image_rows):
    """per row: the number of entries in front of the first id outside [image_lo, image_lo + image_rows)"""
    ids = np.asarray(ids, np.int64)
    bad = (ids < image_lo) | (ids >= image_lo + image_rows)
    return np.where(bad.any(1), bad.argmax(1), ids.shape[1]).astype(np.int64)


def relevance(s, dtype):
    """rel_i = (s_i - s_last) / (s_0 - s_last) in `dtype`; all 0 when s_0 == s_last"""
    s = np.asarray(s, np.float32).astype(dtype)
    if s.size == 0 or s[0] == s[-1]:
        return np.zeros(s.size, dtype)
    return ((s - s[-1]) / (s[0] - s[-1])).astype(dtype)


def objective(rel, m, lam, dtype):
    """lam * rel - (1 - lam) * m: two products and one subtraction in `dtype`, lam the float32 the entry point receives"""
    lam = dtype(np.float32(lam))
    oml = dtype(dtype(1) - lam)
    return (lam * rel).astype(dtype) - (oml * m).astype(dtype)


def mmr_row(s, S, k, lam, dtype, count_ties=False):
    """the pick positions of one row: s [n] float32 sorted scores of the n candidates, S [n, n] similarities"""
    n = len(s)
    kk = min(k, n)
    if kk == 0:
        return (np.zeros(0, np.int64), 0) if count_ties else np.zeros(0, np.int64)
    S = np.asarray(S).astype(dtype)
    rel = relevance(s, dtype)
    picks = [0]
    taken = np.zeros(n, bool)
    taken[0] = True
    m = S[:, 0].copy()
    ties = 0
    for _ in range(1, kk):
        obj = objective(rel, m, lam, dtype)
        obj = np.where(taken, -np.inf, obj)
        p = int(np.argmax(obj))                       # the first maximum: the lowest position
        ties += int((obj == obj[p]).sum() > 1)
        picks.append(p)
        taken[p] = True
        m = np.maximum(m, S[:, p])
    picks = np.asarray(picks, np.int64)
    return (picks, ties) if count_ties else picks


def mmr_lists(scores, ids, S, k, lam, dtype, n=None):
    """scores / ids [rows, c] as ltg_topk writes them, S a sequence of per-row [>= n_r, >= n_r] similarity matrices over candidate
    positions, n the per-row candidate counts (default: the ids >= 0 in front) -> (score_out [rows, k] float32, id_out [rows, k] int32,
    picks: a list of position arrays)"""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.int32)
    R = scores.shape[0]
    if n is None:
        n = valid_counts(ids, 0, 2 ** 31)
    so = np.full((R, k), -np.inf, np.float32)
    io = np.full((R, k), -1, np.int32)
    picks = []
    for r in range(R):
        nr = int(n[r])
        p = mmr_row(scores[r, :nr], np.asarray(S[r])[:nr, :nr], k, lam, dtype)
        picks.append(p)
        so[r, :len(p)] = scores[r, p]
        io[r, :len(p)] = ids[r, p]
    return so, io, picks


def brute_force_row(s, S, k, lam):
    """the same picks by plain Python loops in float64 (tests the vectorised form above)"""
    n = len(s)
    if n == 0:
        return []
    s = [float(np.float32(x)) for x in s]
    lam = float(np.float32(lam))
    span = s[0] - s[-1]
    rel = [(x - s[-1]) / span if span != 0 else 0.0 for x in s]
    picks = [0]
    while len(picks) < min(k, n):
        best, arg = None, -1
        for i in range(n):
            if i in picks:
                continue
            o = lam * rel[i] - (1.0 - lam) * max(float(S[i][p]) for p in picks)
            if best is None or o > best:              # strictly larger: ties stay with the lowest position
                best, arg = o, i
        picks.append(arg)
    return picks


def pair_sum(S, positions):
    """(the sum of S over the unordered pairs of `positions` in float64, the number of pairs)"""
    p = np.asarray(positions, np.int64)
    if p.size < 2:
        return 0.0, 0
    sub = np.asarray(S, np.float64)[np.ix_(p, p)]
    return float(np.triu(sub, 1).sum()), int(p.size * (p.size - 1) // 2)


def ils(S, positions):
    """the mean of S over the unordered pairs of `positions`, in float64; 0 with fewer than two"""
    t, pairs = pair_sum(S, positions)
    return t / pairs if pairs else 0.0


def pick_shortfall(s, S64, picks, lam):
    """for every step t >= 1 of a pick sequence: (max over the positions outside the first t picks of obj64) - obj64[p_t], everything in
    float64 given the prefix -> an array of len(picks) - 1 shortfalls (<= 0 where the pick is the fp64 optimum)"""
    rel = relevance(s, np.float64)
    S64 = np.asarray(S64, np.float64)
    n = len(s)
    out = []
    taken = np.zeros(n, bool)
    taken[picks[0]] = True
    m = S64[:, picks[0]].copy()
    for t in range(1, len(picks)):
        obj = objective(rel, m, lam, np.float64)
        out.append(float(np.where(taken, -np.inf, obj).max() - obj[picks[t]]))
        taken[picks[t]] = True
        m = np.maximum(m, S64[:, picks[t]])
    return np.asarray(out, np.float64)


# ---------------------------------------------------------------------------------------------------------------- exact inputs
EXACT_CASES = [(1, 1), (2, 2), (17, 5), (64, 20), (64, 64), (200, 100), (256, 256), (256, 1)]
EXACT_LAMBDAS = [0.0, 0.5, 0.75, 1.0]
EXACT_ROWS = 37


def exact_image(rows=700, seed=5):
    """a `dot` image whose row products are exact in any order: 8 non-zeros from {+-0.5, +-1} per row within the first 32 columns, so
    every partial sum is a multiple of 0.25 (|S| <= 8)"""
    rng = np.random.default_rng(seed)
    W = np.zeros((rows, 32), np.float32)
    for r in range(rows):
        W[r, rng.choice(32, 8, replace=False)] = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0], np.float32), 8)
    return NR.pack_image(W, "dot")


def exact_lists(c_in, k, image_rows, image_lo=0, rows=EXACT_ROWS, seed=11):
    """-> (scores [rows, c_in] float32, ids [rows, c_in] int32): multiples of 1/64 with s_0 = 1 and s_last = 0 (rel == s exactly), distinct
    random ids of the image, sorted as ltg_topk sorts.  Row 0: all padding; row 1: every score equal; row 2: fewer than k entries; row 3:
    an id outside the image in the middle (it and everything behind it is dropped); row 4: one entry; the others full or randomly short."""
    rng = np.random.default_rng(seed + 1000 * c_in + k)
    sc = np.full((rows, c_in), -np.inf, np.float32)
    ids = np.full((rows, c_in), -1, np.int32)
    for r in range(rows):
        n = c_in if r % 3 else int(rng.integers(1, c_in + 1))
        if r == 0:
            n = 0
        elif r == 2:
            n = max(1, k - 1 - int(rng.integers(0, max(1, k // 2))))
        elif r == 4:
            n = 1
        s = rng.integers(0, 65, n).astype(np.float32) / np.float32(64)
        if r == 1:
            s[:] = np.float32(0.5)
        g = (image_lo + rng.choice(image_rows, n, replace=False)).astype(np.int32)
        order = np.lexsort((g, -s))
        s, g = s[order], g[order]
        if n >= 2 and r != 1:
            s[0], s[-1] = 1.0, 0.0                  # (still sorted: every score lies in [0, 1])
        sc[r, :n], ids[r, :n] = s, g
        if r == 3 and n >= 3:
            ids[r, n // 2] = image_lo + image_rows if n % 2 else image_lo - 1
    return sc, ids


def exact_similarities(img, ids, image_lo, n):
    """per row the float64 similarity matrix of its first n[r] candidates (exact for exact_image)"""
    out = []
    for r in range(ids.shape[0]):
        rows = img[np.asarray(ids[r, :n[r]], np.int64) - image_lo]
        out.append(NR.scores64(rows, rows))
    return out
