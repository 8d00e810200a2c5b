"""The reference of the exposure-capped lists (ltg_cap_index / ltg_cap_rounds / ltg_cap_finish), stated twice: capped_rounds,
the synchronous threshold rounds of the definition in numpy, and capped_sequential, textbook user-proposing deferred acceptance that
processes ONE proposal at a time with a heap per item and walks the users in another order.  Plus a blocking-pair checker that reads
nothing but the candidates, the caps and a table of lists, and the builders of the inputs the CPU and the GPU tests share."""
import heapq

import numpy as np

NEG_INF = np.float32(-np.inf)


# ------------------------------------------------------------------------------------------------ the order items rank users by
def tk_key(s):
    """ltg_topk's order-preserving 32-bit key of float32 values: -0.0 -> +0.0, larger key == larger float"""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def words(cand_s, lse=None):
    """[n, c] uint64: au_comp(s, row) of csrc/ltg_audience.h, s = fp32(cand_s - lse[row]) (lse None: cand_s)"""
    cand_s = np.ascontiguousarray(cand_s, np.float32)
    n = cand_s.shape[0]
    with np.errstate(invalid="ignore"):
        s = cand_s if lse is None else (cand_s - np.asarray(lse, np.float32)[:, None]).astype(np.float32)
    nz = (s.view(np.uint32) == np.uint32(0x80000000)).astype(np.uint64)
    row = (np.uint64(0x7FFFFFFF) - np.arange(n, dtype=np.uint64))[:, None]
    return (tk_key(s).astype(np.uint64) << np.uint64(32)) | (row << np.uint64(1)) | nz


def entry_mask(cand_i, cap):
    """[n, c] bool: the entries that can ever be proposed -- before the row's first padding id, inside the catalogue, cap > 0"""
    cand_i = np.asarray(cand_i)
    live = np.cumsum(cand_i < 0, axis=1) == 0
    inside = live & (cand_i < len(cap))
    ok = inside.copy()
    ok[inside] = np.asarray(cap)[cand_i[inside]] > 0
    return ok, inside


# ------------------------------------------------------------------------------------------------ the definition: synchronous rounds
def capped_rounds(cand_s, cand_i, lse, cap, k, max_rounds=None):
    """-> (active [n, c] bool, thr [I] uint64, rounds): a round = every row's first k admissible entries, then every over-full item
    raises its threshold to its cap-th largest active word; `rounds` counts the rounds up to and including the first that raises none"""
    cap = np.asarray(cap, np.int64)
    n, c = cand_i.shape
    W = words(cand_s, lse)
    ok, _ = entry_mask(cand_i, cap)
    idc = np.where(ok, cand_i, 0).astype(np.int64)
    thr = np.zeros(len(cap), np.uint64)
    rounds = 0
    while True:
        rounds += 1
        adm = ok & (W >= thr[idc])
        act = adm & (np.cumsum(adm, axis=1) <= k)
        ids_a, w_a = idc[act], W[act]
        cnt = np.bincount(ids_a, minlength=len(cap))
        over = np.nonzero(cnt > cap)[0]
        if over.size == 0:
            return act, thr, rounds
        order = np.lexsort((w_a, ids_a))                 # by item, words ascending inside an item
        ids_s, w_s = ids_a[order], w_a[order]
        end = np.searchsorted(ids_s, over, side="right")
        thr[over] = w_s[end - cap[over]]
        if max_rounds is not None and rounds >= max_rounds:
            raise RuntimeError("no fixed point after %d rounds" % rounds)


def lists_of(cand_s, cand_i, active, k):
    """the active entries of every row in candidate order -> (scores [n, k] float32, ids [n, k] int32), padded with -inf / -1"""
    n = cand_i.shape[0]
    out_s, out_i = np.full((n, k), NEG_INF, np.float32), np.full((n, k), -1, np.int32)
    pos = np.cumsum(active, axis=1) - 1
    r, j = np.nonzero(active)
    out_s[r, pos[r, j]] = cand_s[r, j]
    out_i[r, pos[r, j]] = cand_i[r, j]
    return out_s, out_i


def capped_lists(cand_s, cand_i, lse, cap, k):
    """-> (scores, ids, stats): stats = dict(rounds, over = the entries the walks passed over, short = the rows with a short list)"""
    act, _, rounds = capped_rounds(cand_s, cand_i, lse, cap, k)
    s, i = lists_of(cand_s, cand_i, act, k)
    _, inside = entry_mask(cand_i, cap)
    taken = np.cumsum(act, axis=1)
    walked = (taken < k) | act                          # up to and including the k-th active entry
    over = int((inside & walked & ~act).sum())
    return s, i, dict(rounds=rounds, over=over, short=int((i[:, k - 1] < 0).sum()))


# ------------------------------------------------------------------------------------------------ restated: one proposal at a time
def capped_sequential(cand_s, cand_i, lse, cap, k, user_order=None):
    """deferred acceptance with a min-heap of the held words per item, one proposal at a time, users started in `user_order` (default:
    last row first) and a rejected user served at once (depth first) -> active [n, c] bool"""
    n, c = cand_i.shape
    W = words(cand_s, lse)
    ok, _ = entry_mask(cand_i, cap)
    ptr, held = [0] * n, [0] * n
    heaps = {}
    active = np.zeros((n, c), bool)
    todo = list(range(n)) if user_order is None else list(user_order)[::-1]     # a stack: the default pops the last row first
    while todo:
        u = todo.pop()
        while held[u] < k and ptr[u] < c:
            j = ptr[u]
            ptr[u] += 1
            if not ok[u, j]:
                if cand_i[u, j] < 0:
                    ptr[u] = c                           # padding ends the row
                continue
            i, w = int(cand_i[u, j]), int(W[u, j])
            h = heaps.setdefault(i, [])
            if len(h) < cap[i]:
                heapq.heappush(h, (w, u, j))
            elif w > h[0][0]:
                _, v, jv = heapq.heapreplace(h, (w, u, j))
                active[v, jv] = False
                held[v] -= 1
                todo.append(v)                           # v proposes again, after u or at once if u is done
            else:
                continue
            active[u, j] = True
            held[u] += 1
    return active


# ------------------------------------------------------------------------------------------------ the checker
def blocking_pairs(cand_s, cand_i, lse, cap, k, ids):
    """the number of blocking pairs of the table ids [n, k] (read as sets; padding -1): a user u and a candidate j of u that is not in
    u's list, whose cap is > 0, that u prefers to the last entry of the list (or u has a free slot), and whose item has a free place or
    holds a user it ranks below u.  Reads only the inputs and the table."""
    cap = np.asarray(cap, np.int64)
    n, c = cand_i.shape
    W = words(cand_s, lse)
    ok, _ = entry_mask(cand_i, cap)
    listed = np.zeros((n, c), bool)
    for u in range(n):
        listed[u] = np.isin(cand_i[u], ids[u][ids[u] >= 0])
    listed &= ok
    hits = np.bincount(cand_i[listed], minlength=len(cap))
    worst = np.full(len(cap), np.iinfo(np.uint64).max, np.uint64)          # the lowest word an item holds
    np.minimum.at(worst, cand_i[listed], W[listed])
    full = listed.sum(1) >= k
    last = np.where(listed.any(1), c - 1 - np.argmax(listed[:, ::-1], axis=1), -1)
    pos = np.arange(c)[None, :]
    preferred = ok & ~listed & (~full[:, None] | (pos < last[:, None]))
    idc = np.where(ok, cand_i, 0)
    wants = (hits[idc] < cap[idc]) | (W > worst[idc])
    return int((preferred & wants).sum())


# ------------------------------------------------------------------------------------------------ inputs
def topk_rows(logits, c):
    """every row's c best columns in ltg_topk's order (score descending, -0.0 == +0.0, ties lower id first) -> (scores, ids)"""
    logits = np.ascontiguousarray(logits, np.float32)
    n, I = logits.shape
    key = tk_key(logits).astype(np.int64)
    order = np.argsort(-key * I + np.arange(I)[None, :], axis=1, kind="stable")[:, :c]
    s = np.take_along_axis(logits, order, axis=1)
    pad = max(0, c - I)
    if pad:
        s = np.concatenate([s, np.full((n, pad), NEG_INF, np.float32)], axis=1)
        order = np.concatenate([order, np.full((n, pad), -1, order.dtype)], axis=1)
    return s, order.astype(np.int32)


def zipf_case(seed, n, I, c, noise=1.0, quant=None, pad_rows=0):
    """synthetic candidates: logits = log Zipf popularity + noise (quant: rounded to multiples of it, so that many users tie on an item
    and the row decides), the row's top c; lse = the row's log-sum-exp in fp32; pad_rows: that many rows are cut short with padding
    -> (cand_s [n, c] float32, cand_i [n, c] int32, lse [n] float32)"""
    rng = np.random.default_rng(seed)
    pop = -np.log(np.arange(1, I + 1, dtype=np.float64))
    pop = pop[rng.permutation(I)]                        # the head is not the low ids
    x = pop[None, :] + noise * rng.standard_normal((n, I))
    if quant is not None:
        x = np.round(x / quant) * quant
    logits = x.astype(np.float32)
    m = logits.max(1, keepdims=True)
    lse = (m[:, 0] + np.log(np.exp(logits - m).astype(np.float32).sum(1, dtype=np.float32))).astype(np.float32)
    if quant is not None:
        lse = (np.round(lse / quant) * quant).astype(np.float32)     # ties across users survive the subtraction
    s, i = topk_rows(logits, c)
    for u in rng.choice(n, size=min(pad_rows, n), replace=False):
        cut = int(rng.integers(0, c))
        s[u, cut:], i[u, cut:] = NEG_INF, -1
    return s, i, lse


def exposure(ids, n_items):
    return np.bincount(ids[ids >= 0], minlength=n_items)


def counts_as_case(cand_s, cand_i, lse, cap, k):
    """what the issue asks of a parity case, on the reference: at least a quarter of the rows differ from the plain top-k, and at least
    one item sits exactly at its cap -> (share of rows that differ, items at their cap)"""
    _, ids, _ = capped_lists(cand_s, cand_i, lse, cap, k)
    differ = float((ids != cand_i[:, :k]).any(1).mean())
    hits = exposure(ids, len(cap))
    at_cap = int(((hits == np.asarray(cap)) & (np.asarray(cap) > 0)).sum())
    return differ, at_cap
