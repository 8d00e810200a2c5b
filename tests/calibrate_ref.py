"""The reference of the calibrated lists (ltg_hist_groups, ltg_topk_calibrate), stated twice: calibrate_row in numpy with
fp32 / int64 / fp64 exactly where the definition has them, and loop_row, a plain loop over Python numbers that rounds to fp32 by hand
(a sum, product or quotient of two fp32 values computed in fp64 and then rounded to fp32 is the correctly rounded fp32 result).  Plus the
builders of the inputs the CPU and the GPU tests share."""
import struct

import numpy as np

NEG_INF = np.float32(-np.inf)


# ------------------------------------------------------------------------------------------------ the definition, in numpy
def topk_order(scores, ids):
    """the permutation that puts entries into ltg_topk's order: score descending, -0.0 == +0.0, equal scores lower id first"""
    return np.lexsort((np.asarray(ids), -(np.asarray(scores, np.float32) + np.float32(0.0))))


def valid_len(ids):
    """the entries in front of the first padding (id < 0)"""
    bad = np.nonzero(np.asarray(ids) < 0)[0]
    return int(bad[0]) if bad.size else int(len(ids))


def tv32(counts, h, m):
    """the miscalibration of a list of m entries with class counts `counts` against the history counts h: exact int64, one fp64
    division, one rounding to fp32"""
    H = int(np.sum(h, dtype=np.int64))
    if H == 0:
        return np.float32(0.0)
    D = int(np.abs(np.asarray(h, np.int64) * m - np.asarray(counts, np.int64) * H).sum())
    return np.float32(np.float64(D) / np.float64(2 * H * m))


def calibrate_row(S, I, list_class, n_groups, h, lam, k):
    """S / I: [n_lists][m_in] lists of one row, list_class their classes, h [n_groups + 1] the history counts
    -> (scores [k] float32, ids [k] int32, stat [2] float32, picks as (list, position) pairs)"""
    C, L = n_groups + 1, len(list_class)
    lam32 = np.float32(lam)
    a = np.float32(1.0) - lam32
    h = np.asarray(h, np.int64)
    H = int(h.sum())
    lens = [valid_len(I[j]) for j in range(L)]
    out_s, out_i = np.full(k, NEG_INF, np.float32), np.full(k, -1, np.int32)
    ent = [(j, p) for j in range(L) for p in range(lens[j])]
    kk = min(k, len(ent))
    if kk == 0:
        return out_s, out_i, np.zeros(2, np.float32), []
    es = np.array([S[j][p] for j, p in ent], np.float32)
    ei = np.array([I[j][p] for j, p in ent], np.int64)
    plain = topk_order(es, ei)[:kk]
    s_hi, s_lo = es[plain[0]], es[plain[-1]]
    flat = bool(s_hi == s_lo)
    span = s_hi - s_lo
    plain_counts = np.bincount([list_class[ent[e][0]] for e in plain], minlength=C)
    cur, cnt, picks = [0] * L, np.zeros(C, np.int64), []
    for t in range(kk):
        m = t + 1
        act = [j for j in range(L) if cur[j] < lens[j]]
        hs = np.array([S[j][cur[j]] for j in act], np.float32)
        hi = np.array([I[j][cur[j]] for j in act], np.int64)
        cls = np.array([list_class[j] for j in act])
        with np.errstate(all="ignore"):
            rel = np.zeros(len(act), np.float32) if flat else (hs - s_lo) / span
        if H > 0:
            x = h * m - cnt * H
            D = np.abs(x).sum() - np.abs(x[cls]) + np.abs(x[cls] - H)
            tv = (D.astype(np.float64) / np.float64(2 * H * m)).astype(np.float32)
        else:
            tv = np.zeros(len(act), np.float32)
        obj = a * rel - lam32 * tv
        tied = np.nonzero(obj == obj.max())[0]
        w = tied[topk_order(hs[tied], hi[tied])[0]]
        j = act[w]
        picks.append((j, cur[j]))
        out_s[t], out_i[t] = S[j][cur[j]], I[j][cur[j]]
        cur[j] += 1
        cnt[list_class[j]] += 1
    stat = np.array([tv32(plain_counts, h, kk), tv32(cnt, h, kk)], np.float32)
    return out_s, out_i, stat, picks


def calibrate_lists(S, I, list_class, n_groups, hist, lam, k):
    """S / I [n_lists, n_rows, m_in], hist [n_rows, n_groups + 1] -> (scores [n_rows, k], ids [n_rows, k], stats [n_rows, 2])"""
    n = S.shape[1]
    out_s, out_i, st = np.empty((n, k), np.float32), np.empty((n, k), np.int32), np.empty((n, 2), np.float32)
    for u in range(n):
        out_s[u], out_i[u], st[u], _ = calibrate_row(S[:, u], I[:, u], list_class, n_groups, hist[u], lam, k)
    return out_s, out_i, st


def plain_lists(S, I, k):
    """the first k entries of the merge of the lists, per row, padded: what lambda = 0 has to give (and ltg_topk_merge)"""
    L, n, m_in = S.shape
    out_s, out_i = np.full((n, k), NEG_INF, np.float32), np.full((n, k), -1, np.int32)
    for u in range(n):
        es = np.concatenate([S[j, u, :valid_len(I[j, u])] for j in range(L)])
        ei = np.concatenate([I[j, u, :valid_len(I[j, u])] for j in range(L)])
        o = topk_order(es, ei)[:k]
        out_s[u, :len(o)], out_i[u, :len(o)] = es[o], ei[o]
    return out_s, out_i


def hist_groups(indptr, indices, hist_lo, labels, n_groups):
    """ltg_hist_groups in numpy: [n_rows, n_groups + 1] int32"""
    labels = np.asarray(labels)
    out = np.zeros((len(indptr) - 1, n_groups + 1), np.int32)
    for u in range(len(indptr) - 1):
        g = hist_lo + np.asarray(indices[indptr[u]:indptr[u + 1]], np.int64)
        g = g[(g >= 0) & (g < labels.size)]
        out[u] = np.bincount(np.minimum(labels[g].astype(np.int64), n_groups), minlength=n_groups + 1)
    return out


# ------------------------------------------------------------------------------------------------ the definition again, as a plain loop
def f32(x):
    """the fp32 nearest to the Python float x (ties to even), as a Python float"""
    return struct.unpack("f", struct.pack("f", x))[0]


def _before(s1, i1, s2, i2):
    """does entry 1 come before entry 2 in ltg_topk's order (Python floats: -0.0 == 0.0)"""
    return s1 > s2 or (s1 == s2 and i1 < i2)


def loop_row(S, I, list_class, n_groups, h, lam, k):
    """-> (ids, scores as Python floats, (tv of the plain list, tv of the output)), unpadded"""
    C, L = n_groups + 1, len(list_class)
    lam = f32(lam)
    a = f32(1.0 - lam)
    h = [int(x) for x in h]
    H = sum(h)
    lists = []
    for j in range(L):
        row = []
        for s, i in zip(S[j], I[j]):
            if int(i) < 0:
                break
            row.append((float(s), int(i)))
        lists.append(row)
    n = sum(len(row) for row in lists)
    kk = min(k, n)
    if kk == 0:
        return [], [], (0.0, 0.0)

    def best_head(cur, better):
        w = -1
        for j in range(L):
            if cur[j] < len(lists[j]) and (w < 0 or better(j, w)):
                w = j
        return w

    def tv(counts, m):
        if H == 0:
            return 0.0
        D = 0
        for c in range(C):
            D += abs(h[c] * m - counts[c] * H)
        return f32(D / (2 * H * m))            # (Python's int / int is the correctly rounded quotient, as the fp64 division of two exact doubles)

    cur, counts, merged = [0] * L, [0] * C, []
    for _ in range(kk):
        j = best_head(cur, lambda x, y: _before(*lists[x][cur[x]], *lists[y][cur[y]]))
        merged.append(lists[j][cur[j]][0])
        cur[j] += 1
        counts[list_class[j]] += 1
    tv_plain = tv(counts, kk)
    s_hi, s_lo = merged[0], merged[-1]

    def rel(s):
        return 0.0 if s_hi == s_lo else f32(f32(s - s_lo) / f32(s_hi - s_lo))

    cur, counts, ids, scores = [0] * L, [0] * C, [], []
    for t in range(kk):
        def obj(j):
            c = list_class[j]
            plus = list(counts)
            plus[c] += 1
            return f32(f32(a * rel(lists[j][cur[j]][0])) - f32(lam * tv(plus, t + 1)))

        def better(x, y):
            ox, oy = obj(x), obj(y)
            return ox > oy or (ox == oy and _before(*lists[x][cur[x]], *lists[y][cur[y]]))

        j = best_head(cur, better)
        scores.append(lists[j][cur[j]][0])
        ids.append(lists[j][cur[j]][1])
        cur[j] += 1
        counts[list_class[j]] += 1
    return ids, scores, (tv_plain, tv(counts, kk))


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("regular", "ties", "equal", "zeros", "H0", "unlisted", "padlist", "usedup", "short", "bigH", "ragged")


def sorted_list(scores, ids, m_in):
    """one list in ltg_topk's format: ordered, padded to m_in with id -1 / score -inf"""
    o = topk_order(scores, ids)
    s, i = np.full(m_in, NEG_INF, np.float32), np.full(m_in, -1, np.int32)
    s[:len(o)], i[:len(o)] = np.asarray(scores, np.float32)[o], np.asarray(ids, np.int32)[o]
    return s, i


def build_case(seed, n_rows, n_groups, list_class, m_in, k, kinds=KINDS):
    """-> (S [n_lists, n_rows, m_in] float32, I int32, hist [n_rows, n_groups + 1] int32, the kind of every row).  Row u is of kind
    kinds[u % len(kinds)]:
      regular   full lists of Gaussian scores, a random history
      ties      scores from seven values: ties inside and across the classes
      equal     every score the same
      zeros     scores from {-1, -0.0, +0.0, 1}
      H0        an empty history
      unlisted  the whole history in a class that has no list (or, when every class has one, in the class of an all-padding list)
      padlist   the first list is all padding
      usedup    the first list holds three entries and owns the whole history: the class is used up
      short     fewer than k entries over all lists (n < k)
      bigH      a history of 5 000 items: 2 H m exceeds 2^24
      ragged    lists of random lengths"""
    rng = np.random.default_rng(seed)
    C, L = n_groups + 1, len(list_class)
    S = np.full((L, n_rows, m_in), NEG_INF, np.float32)
    I = np.full((L, n_rows, m_in), -1, np.int32)
    hist = np.zeros((n_rows, C), np.int32)
    row_kind = []
    unlisted = [c for c in range(C) if c not in list_class]
    for u in range(n_rows):
        kind = kinds[u % len(kinds)]
        row_kind.append(kind)
        lens = [m_in] * L
        if kind == "ragged":
            lens = [int(rng.integers(0, m_in + 1)) for _ in range(L)]
        elif kind == "short":
            lens = [int(x) for x in rng.multinomial(max(0, k - 1 - int(rng.integers(0, max(1, k // 2)))), np.ones(L) / L)]
            lens = [min(x, m_in) for x in lens]
        elif kind == "usedup":
            lens[0] = min(3, m_in)
        if kind == "padlist" or (kind == "unlisted" and not unlisted):
            lens[0] = 0
        ids = rng.permutation(7 * L * m_in + 11)[: L * m_in].astype(np.int32).reshape(L, m_in)
        for j in range(L):
            if kind == "ties":
                sc = rng.integers(-3, 4, lens[j]) / 4.0
            elif kind == "equal":
                sc = np.full(lens[j], 0.625)
            elif kind == "zeros":
                sc = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0]), lens[j])
            else:
                sc = rng.standard_normal(lens[j])
            S[j, u], I[j, u] = sorted_list(sc.astype(np.float32), ids[j, :lens[j]], m_in)
        H = 5000 if kind == "bigH" else int(rng.integers(1, 200))
        if kind == "H0":
            pass
        elif kind == "unlisted":
            hist[u, unlisted[0] if unlisted else list_class[0]] = H
        elif kind == "usedup":
            hist[u, list_class[0]] = H
        else:
            hist[u] = rng.multinomial(H, rng.dirichlet(np.ones(C)))
    return S, I, hist, row_kind
