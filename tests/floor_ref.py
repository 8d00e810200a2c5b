"""The reference of the exposure-floor lists (ltg_floor_index / ltg_floor_rounds / ltg_floor_finish), stated twice:
floor_rounds, the synchronous rounds of falling per-user limits of the definition in numpy, and floor_sequential, textbook item-proposing
deferred acceptance that processes ONE proposal at a time with a heap per user and starts the items in another order.  Plus the
composition of the lists from a table of active entries, a blocking-pair checker that reads nothing but the inputs and such a table,
and the builders of the inputs the CPU and the GPU tests share.  The order items rank users by, the candidates and the exposure count
are the capped lists' (tests/capped_ref.py)."""
import heapq

import numpy as np

from capped_ref import exposure, tk_key, topk_rows, words, zipf_case  # noqa: F401  (re-exported: the tests import this module alone)

NEG_INF = np.float32(-np.inf)
STATE = 8


def floor_mask(cand_i, need):
    """-> (floor [n, c] bool: the floor entries -- before the row's first padding id, inside the catalogue, need > 0; live [n, c] bool)"""
    cand_i = np.asarray(cand_i)
    live = np.cumsum(cand_i < 0, axis=1) == 0
    inside = live & (cand_i < len(need))
    fl = inside.copy()
    fl[inside] = np.asarray(need)[cand_i[inside]] > 0
    return fl, live


# ------------------------------------------------------------------------------------------------ the definition: synchronous rounds
def select(W, idc, adm, need):
    """sel [I] uint64: the need-th largest word among an item's admissible floor entries, 0 where it has no more than need of them"""
    sel = np.zeros(len(need), np.uint64)
    ids_a, w_a = idc[adm], W[adm]
    cnt = np.bincount(ids_a, minlength=len(need))
    over = np.nonzero((cnt > need) & (need > 0))[0]
    if over.size:
        order = np.lexsort((w_a, ids_a))                 # by item, words ascending inside an item
        ids_s, w_s = ids_a[order], w_a[order]
        end = np.searchsorted(ids_s, over, side="right")
        sel[over] = w_s[end - need[over]]
    return sel


def floor_rounds(cand_s, cand_i, lse, need, k, reserve, max_rounds=None):
    """-> (active [n, c] bool, lim [n], rounds, lowerings): a round = every item's need best admissible entries, then every row with more
    than `reserve` of them at positions >= k - reserve lowers its limit to the reserve-th; `rounds` counts the rounds up to and including
    the first that lowers no limit, `lowerings` the (row, round) pairs that lowered one"""
    need = np.asarray(need, np.int64)
    n, c = cand_i.shape
    R = int(reserve)
    W = words(cand_s, lse)
    fl, _ = floor_mask(cand_i, need)
    idc = np.where(fl, cand_i, 0).astype(np.int64)
    pos = np.arange(c)[None, :]
    zone = pos >= k - R
    lim = np.full(n, c - 1 if R > 0 else k - 1, np.int64)
    rounds = lowerings = 0
    while True:
        rounds += 1
        adm = fl & (pos <= lim[:, None])
        act = adm & (W >= select(W, idc, adm, need)[idc])
        za = act & zone
        zc = np.cumsum(za, axis=1)
        low = np.nonzero(zc[:, -1] > R)[0]
        if low.size == 0:
            return act, lim, rounds, lowerings
        lim[low] = np.argmax(za[low] & (zc[low] == R), axis=1) if R > 0 else k - 1
        lowerings += int(low.size)
        if max_rounds is not None and rounds >= max_rounds:
            raise RuntimeError("no fixed point after %d rounds" % rounds)


# ------------------------------------------------------------------------------------------------ the composition
def compose(cand_s, cand_i, active, k, reserve=None):
    """the lists of a table of active entries -> (scores [n, k] float32, ids [n, k] int32, t [n]): t = the smallest value for which the
    active entries at positions >= k - t are at most t; the list = the first k - t live candidates, then those entries in candidate
    order; padded with -inf / -1.  reserve: asserted to bound t"""
    n, c = cand_i.shape
    live = np.cumsum(cand_i < 0, axis=1) == 0
    out_s, out_i = np.full((n, k), NEG_INF, np.float32), np.full((n, k), -1, np.int32)
    ts = np.zeros(n, np.int64)
    for u in range(n):
        t = 0
        while int(active[u, k - t:].sum()) > t:
            t += 1
            assert t <= k, u
        assert int(active[u, k - t:].sum()) == t and (reserve is None or t <= reserve), u
        head = np.nonzero(live[u, :k - t])[0]
        tail = k - t + np.nonzero(active[u, k - t:])[0]
        js = np.concatenate([head, tail]).astype(np.int64)
        out_s[u, :len(js)], out_i[u, :len(js)] = cand_s[u, js], cand_i[u, js]
        ts[u] = t
    return out_s, out_i, ts


def state_block(cand_i, need, active, ts, rounds, lowerings, batch=1):
    """the int32 state block a converged device run leaves when it enqueues the rounds in batches of `batch` -> ([STATE] int64, held [I])"""
    need = np.asarray(need, np.int64)
    fl, _ = floor_mask(cand_i, need)
    held = np.bincount(np.asarray(cand_i)[active & fl], minlength=len(need))
    ran = -(-rounds // batch) * batch
    st = [lowerings, ran, int(((need > 0) & (held < need)).sum()), int((ts > 0).sum()), rounds - 1, int(ts.sum()), int((need > 0).sum()), 0]
    return np.array(st, np.int64), held


def floor_lists(cand_s, cand_i, lse, need, k, reserve, batch=1):
    """-> (scores, ids, active, held, state): everything the device returns, from the definition"""
    act, _, rounds, lowerings = floor_rounds(cand_s, cand_i, lse, need, k, reserve)
    s, i, ts = compose(cand_s, cand_i, act, k, reserve)
    st, held = state_block(cand_i, need, act, ts, rounds, lowerings, batch)
    return s, i, act, held, st


# ------------------------------------------------------------------------------------------------ restated: one proposal at a time
def floor_sequential(cand_s, cand_i, lse, need, k, reserve, item_order=None):
    """item-proposing deferred acceptance, one proposal at a time: an item proposes down its entries, best word first, while it holds
    fewer than need acceptances; a user accepts every proposal before its zone and keeps, of those in the zone, the `reserve` with the
    lowest positions (a max-heap of the held positions); the item a user lets go proposes again at once (depth first).  Items start in
    `item_order` (default: the last id first) -> active [n, c] bool"""
    need = np.asarray(need, np.int64)
    n, c = cand_i.shape
    R = int(reserve)
    W = words(cand_s, lse)
    fl, _ = floor_mask(cand_i, need)
    props = {}
    for u, j in zip(*np.nonzero(fl)):
        props.setdefault(int(cand_i[u, j]), []).append((int(W[u, j]), int(u), int(j)))
    for p in props.values():
        p.sort(reverse=True)
    nxt = {i: 0 for i in props}
    got = {i: 0 for i in props}
    heaps = [[] for _ in range(n)]                       # (-position, item) of the zone entries a user holds
    active = np.zeros((n, c), bool)
    todo = sorted(props) if item_order is None else [i for i in list(item_order)[::-1] if i in props]
    while todo:
        i = todo.pop()
        while got[i] < need[i] and nxt[i] < len(props[i]):
            _, u, j = props[i][nxt[i]]
            nxt[i] += 1
            if j >= k - R:
                h = heaps[u]
                if len(h) < R:
                    heapq.heappush(h, (-j, i))
                elif R > 0 and j < -h[0][0]:
                    mj, v = heapq.heapreplace(h, (-j, i))
                    active[u, -mj] = False
                    got[v] -= 1
                    todo.append(v)                       # v proposes again, after i or at once if i is done
                else:
                    continue
            active[u, j] = True
            got[i] += 1
    return active


# ------------------------------------------------------------------------------------------------ the checker
def blocking_pairs(cand_s, cand_i, lse, need, k, reserve, active):
    """the number of blocking pairs of a table of active entries: a floor entry (u, j) that is not active, whose item holds fewer than
    need entries or an active entry with a smaller word, and whose user has j before its zone, or fewer than `reserve` active entries in
    the zone, or one of them behind j.  Reads only the inputs and the table."""
    need = np.asarray(need, np.int64)
    n, c = cand_i.shape
    R = int(reserve)
    W = words(cand_s, lse)
    fl, _ = floor_mask(cand_i, need)
    active = np.asarray(active, bool) & fl
    idc = np.where(fl, cand_i, 0).astype(np.int64)
    held = np.bincount(idc[active], minlength=len(need))
    worst = np.full(len(need), np.iinfo(np.uint64).max, np.uint64)          # the lowest word an item holds
    np.minimum.at(worst, idc[active], W[active])
    pos = np.arange(c)[None, :]
    za = active & (pos >= k - R)
    last = np.where(za.any(1), c - 1 - np.argmax(za[:, ::-1], axis=1), -1)
    item_wants = (held[idc] < need[idc]) | (W > worst[idc])
    user_wants = (pos < k - R) | (za.sum(1) < R)[:, None] | (last[:, None] > pos)
    return int((fl & ~active & item_wants & user_wants).sum())


# ------------------------------------------------------------------------------------------------ inputs
def median_need(cand_i, n_items, k, M):
    """need = M on the items whose plain exposure at k is at or below the median, 0 elsewhere"""
    hits = exposure(np.asarray(cand_i)[:, :k], n_items)
    return np.where(hits <= np.median(hits), M, 0).astype(np.int32)
