"""numpy references of the minimum-slots rule (ltg_topk_groups / ltg_topk_quota), shared by tests/test_quota_cpu.py and
tests/test_gpu_quota.py.  Items are LOCAL column ids of a row; labels are indexed by GLOBAL id = item_lo + column."""
import numpy as np


def ranked(row, fold, item_lo=0):
    """the eligible columns of a row, best first: score descending, equal scores lower id first (-0.0 == +0.0 under <)"""
    ok = np.ones(row.size, bool)
    if fold is not None:
        ok[np.asarray(fold, np.int64)] = False
    loc = np.nonzero(ok)[0]
    return loc[np.lexsort((loc + item_lo, -row[loc]))]


def greedy(row, fold, labels, quota, k, item_lo=0):
    """walk the ranking: an item is taken if its group still owes slots, or if a slot is left that no group's outstanding minimum claims"""
    order = ranked(row, fold, item_lo)
    lab = labels[order + item_lo]
    G = len(quota)
    need = np.minimum(np.asarray(quota, np.int64), [(lab == g).sum() for g in range(G)])
    out = []
    for it, g in zip(order.tolist(), lab.tolist()):
        if len(out) == k:
            break
        if g < G and need[g] > 0:
            need[g] -= 1
            out.append(it)
        elif k - len(out) - need.sum() > 0:
            out.append(it)
    return np.array(out, np.int64)


def composed(row, fold, labels, quota, k, k_in, item_lo=0):
    """from lists alone: the plain list (first k_in) and, per group, its own list's first quota[g]"""
    order = ranked(row, fold, item_lo)
    lab = labels[order + item_lo]
    U = []
    for g, q in enumerate(quota):
        U += order[lab == g][:q].tolist()
    members = set(U)
    rest = [i for i in order[:k_in].tolist() if i not in members][:k - len(U)]
    S = np.array(U + rest, np.int64)
    return S[np.lexsort((S + item_lo, -row[S]))] if S.size else S


def lists(L, folds, pick, k, item_lo=0):
    """(scores [n, k], GLOBAL ids [n, k]) padded with -inf / -1 as ltg_topk pads; pick(r) -> the LOCAL columns of row r in list order"""
    n = L.shape[0]
    S = np.full((n, k), -np.inf, np.float32)
    ID = np.full((n, k), -1, np.int32)
    for r in range(n):
        o = pick(r)[:k]
        S[r, :len(o)] = L[r, o]
        ID[r, :len(o)] = o + item_lo
    return S, ID


def masked_lists(L, folds, labels, mask, k, item_lo=0):
    """ltg_topk_groups' contract: the k best eligible items whose label's bit (min(label, 8)) is in mask"""
    def pick(r):
        o = ranked(L[r], None if folds is None else folds[r], item_lo)
        return o[((mask >> np.minimum(labels[o + item_lo], 8).astype(np.int64)) & 1) == 1]
    return lists(L, folds, pick, k, item_lo)


def greedy_lists(L, folds, labels, quota, k, item_lo=0):
    """ltg_topk_quota's contract, from the full rows"""
    return lists(L, folds, lambda r: greedy(L[r], None if folds is None else folds[r], labels, quota, k, item_lo), k, item_lo)
