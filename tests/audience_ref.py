"""numpy reference of the item audiences (ltg_item_audience): per query column the k best eligible rows, score descending, equal scores
lower row first (-0.0 == +0.0), padded with id -1 / score -inf.  score = L[:, c] - lse in float32 (one IEEE subtraction, which numpy
reproduces bit for bit), or L[:, c] when lse is None; row r is eligible for column c iff c is not in folds[r]."""
import numpy as np


def scores_of(L, lse, c):
    col = np.ascontiguousarray(L[:, c], dtype=np.float32)
    return col if lse is None else (col - np.asarray(lse, np.float32)).astype(np.float32)


def eligible(folds, n_rows, c):
    """bool [n_rows]: folds = per row the LOCAL columns it holds (None: nothing held)"""
    ok = np.ones(n_rows, bool)
    if folds is not None:
        for r in range(n_rows):
            if np.any(np.asarray(folds[r]) == c):
                ok[r] = False
    return ok


def holds_matrix(folds, n_rows, n_cols):
    """bool [n_rows, n_cols]: row r holds column c"""
    H = np.zeros((n_rows, n_cols), bool)
    if folds is not None:
        for r in range(n_rows):
            H[r, np.asarray(folds[r], np.int64)] = True
    return H


def audience_lists(L, lse, folds, q_col, k, row_lo=0, held=None):
    """-> (scores [n_q, k] float32, ids [n_q, k] int32 = row_lo + row).  held: holds_matrix(folds, ...) if the caller has it already"""
    n = L.shape[0]
    q_col = np.asarray(q_col).reshape(-1)
    S = np.full((len(q_col), k), -np.inf, np.float32)
    ID = np.full((len(q_col), k), -1, np.int32)
    if held is None and folds is not None:
        held = holds_matrix(folds, n, L.shape[1])
    with np.errstate(invalid="ignore"):
        for j, c in enumerate(q_col.tolist()):
            rows = np.arange(n) if held is None else np.nonzero(~held[:, c])[0]
            sc = scores_of(L, lse, c)[rows]
            o = np.lexsort((rows, -sc))[:k]
            S[j, :len(o)] = sc[o]
            ID[j, :len(o)] = rows[o] + row_lo
    return S, ID


def brute_force(L, lse, folds, q_col, k, row_lo=0):
    """the same lists by repeated selection of the best remaining row: no sort, no key"""
    n = L.shape[0]
    S = np.full((len(q_col), k), -np.inf, np.float32)
    ID = np.full((len(q_col), k), -1, np.int32)
    for j, c in enumerate(list(q_col)):
        left = [r for r in range(n) if folds is None or c not in list(folds[r])]
        for i in range(k):
            if not left:
                break
            best = left[0]
            for r in left[1:]:
                a = np.float32(L[r, c]) - np.float32(lse[r]) if lse is not None else np.float32(L[r, c])
                b = np.float32(L[best, c]) - np.float32(lse[best]) if lse is not None else np.float32(L[best, c])
                if a > b:                        # (-0.0 > 0.0 is False: equal; the earlier row stays)
                    best = r
            left.remove(best)
            S[j, i] = np.float32(L[best, c]) - np.float32(lse[best]) if lse is not None else np.float32(L[best, c])
            ID[j, i] = best + row_lo
    return S, ID
