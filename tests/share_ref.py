"""The reference of the share-targeted lists (ltg_topk_share) in numpy, as include/ltg.h states it: per row a merge of the
promoted and the rest list by (tk_key, id), the step words as uint64, np.sort for the threshold.  Plus a brute force over every allocation
of steps (for tiny cases) and the builder of the inputs the CPU and the GPU tests share."""
import itertools
from fractions import Fraction

import numpy as np

import capped_ref as C

NEG_INF = np.float32(-np.inf)
NO_STEP = np.uint64(0xFFFFFFFFFFFFFFFF)


def order_words(s, i):
    """(tk_key << 32) | ~id of list entries: descending words == ltg_topk's order (score descending, -0.0 == +0.0, ties lower id first)"""
    low = (~np.asarray(i, np.int64)) & np.int64(0xFFFFFFFF)
    return (C.tk_key(s).astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)


def list_len(ids):
    """the non-padding entries of one list: the first id < 0 ends it"""
    neg = np.nonzero(np.asarray(ids) < 0)[0]
    return int(neg[0]) if neg.size else len(ids)


def merged(ps, pi, rs, ri, n_pro, n_rest):
    """the first n_pro promoted and n_rest rest entries merged in ltg_topk's order -> (scores, ids, is_promoted)"""
    s = np.concatenate([ps[:n_pro], rs[:n_rest]]).astype(np.float32)
    i = np.concatenate([pi[:n_pro], ri[:n_rest]]).astype(np.int32)
    pro = np.concatenate([np.ones(n_pro, bool), np.zeros(n_rest, bool)])
    order = np.argsort(order_words(s, i), kind="stable")[::-1]
    return s[order], i[order], pro[order]


def row_steps(ps, pi, rs, ri, k, u):
    """-> (a, kk, words uint64 [steps]) of row u"""
    n_p, n_r = list_len(pi), list_len(ri)
    kk = min(k, n_p + n_r)
    _, _, pro = merged(ps, pi, rs, ri, n_p, n_r)
    a = int(pro[:kk].sum())
    b = kk - a
    steps = min(b, n_p - a)
    t = np.arange(1, steps + 1)
    with np.errstate(invalid="ignore"):
        c = (rs[b - t].astype(np.float32) - ps[a + t - 1].astype(np.float32)).astype(np.float32)
    bits = c.view(np.uint32).copy()
    bits[c == 0] = 0                                     # +-0 is +0.0
    words = (bits.astype(np.uint64) << np.uint64(32)) | (np.uint64(u * k) + (t - 1).astype(np.uint64))
    return a, kk, words


def share_lists(pro_s, pro_i, rest_s, rest_i, k, want):
    """-> (scores [n, k] float32, ids [n, k] int32, state [8] int32, extra): extra = dict(a, kk, t = the steps taken per row, words = the
    list of every row's step words)"""
    n = pro_i.shape[0]
    rows = [row_steps(pro_s[u], pro_i[u], rest_s[u], rest_i[u], k, u) for u in range(n)]
    a = np.array([r[0] for r in rows], np.int64)
    kk = np.array([r[1] for r in rows], np.int64)
    words = [r[2] for r in rows]
    A, N = int(a.sum()), int(sum(len(w) for w in words))
    take = min(max(0, int(want) - A), N)
    t = np.zeros(n, np.int64)
    thr_bits = 0
    if take > 0:
        allw = np.sort(np.concatenate(words))
        thr = allw[take - 1]
        t = np.array([int((w <= thr).sum()) for w in words], np.int64)
        thr_bits = int(thr >> np.uint64(32))
    out_s, out_i = np.full((n, k), NEG_INF, np.float32), np.full((n, k), -1, np.int32)
    for u in range(n):
        s, i, _ = merged(pro_s[u], pro_i[u], rest_s[u], rest_i[u], int(a[u] + t[u]), int(kk[u] - a[u] - t[u]))
        out_s[u, :len(s)], out_i[u, :len(i)] = s, i
    state = np.array([A, N, take, int((t > 0).sum()), np.array([thr_bits], np.uint32).view(np.int32)[0], int(kk.sum()), 0, 0], np.int32)
    return out_s, out_i, state, dict(a=a, kk=kk, t=t, words=words)


def step_cost(words, t):
    """the exact total cost of taking the first t[u] steps of every row (words: share_lists' extra)"""
    tot = Fraction(0)
    for w, tu in zip(words, t):
        for x in w[:int(tu)]:
            tot += Fraction(float(np.array([int(x) >> 32], np.uint32).view(np.float32)[0]))
    return tot


def cheapest_allocation(words, take):
    """brute force over every per-row step count with sum == take -> the least exact total cost (None if no allocation exists)"""
    best = None
    for t in itertools.product(*[range(len(w) + 1) for w in words]):
        if sum(t) != take:
            continue
        c = step_cost(words, t)
        best = c if best is None or c < best else best
    return best


def split_by_label(cand_s, cand_i, promoted, m_in):
    """every row's candidates split into the promoted and the rest list, each cut to m_in and padded with -1 / -inf"""
    n = cand_i.shape[0]
    out = [np.full((n, m_in), NEG_INF, np.float32), np.full((n, m_in), -1, np.int32), np.full((n, m_in), NEG_INF, np.float32),
           np.full((n, m_in), -1, np.int32)]
    for u in range(n):
        live = cand_i[u] >= 0
        sel = np.zeros(len(live), bool)
        sel[live] = promoted[cand_i[u][live]]
        for side, m in ((0, live & sel), (2, live & ~sel)):
            s, i = cand_s[u][m][:m_in], cand_i[u][m][:m_in]
            out[side][u, :len(s)], out[side + 1][u, :len(i)] = s, i
    return tuple(out)


def share_case(n, I, k, c, quant=None, seed=None, m_in=None):
    """synthetic lists: capped_ref.zipf_case's candidates (every row's c best of I items), the promoted label = the items whose hits in the
    plain top-k columns are at or under the median, every row's candidates split by label and cut to m_in (default k)
    -> (pro_s, pro_i, rest_s, rest_i, promoted [I] bool)"""
    s, i, _ = C.zipf_case(n + I if seed is None else seed, n, I, c, quant=quant)
    top = i[:, :k]
    hits = np.bincount(top[top >= 0], minlength=I)
    promoted = hits <= np.median(hits)
    return split_by_label(s, i, promoted, k if m_in is None else m_in) + (promoted,)


def counts_as_case(state, extra):
    """what the issue asks of a parity case, on the reference: the threshold binds (0 < take < N), at least a quarter of the rows change,
    and the rows take at least two distinct numbers of steps"""
    return 0 < state[2] < state[1] and state[3] * 4 >= len(extra["t"]) and len(np.unique(extra["t"])) >= 2
