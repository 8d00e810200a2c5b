"""numpy reference of the critic-checked lists (ltg_pair_critic / ltg_critic_finish / ltg_topk_gate).

    crit(u, b) = mean over a in A_u of s(a, b)      s = the pair logit of the niche companions (companions_ref.score_ref)
    A_u = the history items of u that are popular with features; b = a list entry that is niche with features

side_maps    (niche ids, ids with features, n_items) -> the two sides' ids (ascending) and the item id -> image row maps (-1: not there)
anchors_of   a user's anchors from a CSR history (global id = hist_lo + index), in history order
fixed        fp32 pair logits -> the 64-bit fixed-point integers q = rint(s * 2^24) (round half even); exact: s * 2^24 is a double
mean_fixed   (sum of q, count) -> float32((double) sum / ((double) count * 2^24))
critic_ref   everything the kernels write, from a table of fp32 pair logits S [popular rows, niche rows] -- the device's own scores give
             the bit-for-bit reference, float32(score_ref) of reference images the discriminator's
gate_ref     the gated list of one or more rows
"""
import numpy as np

import companions_ref as CR

SCALE = 16777216.0      # 2^24


def side_maps(niche_ids, valid_ids, n_items):
    """-> (pop_ids, niche_ids, pop_row, niche_row): int32 arrays"""
    niche = np.unique(np.asarray(list(niche_ids), np.int64))
    valid = np.unique(np.asarray(list(valid_ids), np.int64))
    sides = [np.setdiff1d(valid, niche).astype(np.int32), np.intersect1d(valid, niche).astype(np.int32)]
    maps = []
    for a in sides:
        m = np.full(n_items, -1, np.int32)
        m[a] = np.arange(a.size, dtype=np.int32)
        maps.append(m)
    return sides[0], sides[1], maps[0], maps[1]


def anchors_of(indptr, indices, u, pop_row, hist_lo=0):
    """-> the global ids of row u's anchors, in history order (int64)"""
    g = np.asarray(indices[indptr[u]:indptr[u + 1]], np.int64) + int(hist_lo)
    g = g[(g >= 0) & (g < pop_row.size)]
    return g[pop_row[g] >= 0]


def fixed(s):
    s = np.asarray(s, np.float32)
    return np.rint(s.astype(np.float64) * SCALE).astype(np.int64)


def mean_fixed(total, count):
    return np.float32(np.float64(np.int64(total)) / (np.float64(count) * SCALE))


def best_of(s, gid):
    """the best anchor in lists_ref's order: score descending, equal scores the lower id, -0.0 == +0.0 -> (score, id)"""
    o = np.lexsort((np.asarray(gid, np.int64), -(np.asarray(s) + 0.0)))[0]
    return s[o], int(gid[o])


def critic_ref(S, indptr, indices, pop_row, niche_row, ids, top, hist_lo=0):
    """S [n_pop, n_niche] float32 pair logits; ids [n, k_in] the lists -> dict: sum int64 [n, top], cnt int32 [n] (the anchors of THESE
    histories), best_s float32 / best_i int32 [n, top]; and, taking cnt for the user's whole count, crit float32 [n, top], scored bool
    [n, top], n_scored int32 [n]"""
    S = np.asarray(S, np.float32)
    ids = np.asarray(ids)
    n, n_items = ids.shape[0], pop_row.size
    out = dict(sum=np.zeros((n, top), np.int64), cnt=np.zeros(n, np.int32), best_s=np.full((n, top), -np.inf, np.float32),
               best_i=np.full((n, top), -1, np.int32))
    cand = np.zeros((n, top), bool)
    for u in range(n):
        a = anchors_of(indptr, indices, u, pop_row, hist_lo)
        out["cnt"][u] = a.size
        for e in range(top):
            g = int(ids[u, e])
            if not (0 <= g < n_items and niche_row[g] >= 0):
                continue
            cand[u, e] = True
            if a.size == 0:
                continue
            s = S[pop_row[a], niche_row[g]]
            out["sum"][u, e] = fixed(s).sum()
            out["best_s"][u, e], out["best_i"][u, e] = best_of(s, a)
    out.update(finish_ref(out["sum"], out["cnt"], cand))
    return out


def finish_ref(total, cnt, cand):
    """sums and counts over ALL parts, cand [n, top] the candidate entries -> dict(crit, scored, n_scored)"""
    scored = cand & (np.asarray(cnt)[:, None] > 0)
    crit = np.zeros(scored.shape, np.float32)
    for u, e in zip(*np.nonzero(scored)):
        crit[u, e] = mean_fixed(total[u, e], cnt[u])
    return dict(crit=crit, scored=scored, n_scored=scored.sum(1).astype(np.int32))


def reference_scores(D, pop_ids, niche_ids):
    """the discriminator's fp32 pair logits of every (popular, niche) pair, from the fp64 reference images"""
    Ea, Eb = CR.image_ref(CR.pack_ref(D, "popular", pop_ids)), CR.image_ref(CR.pack_ref(D, "niche", niche_ids))
    return CR.score_ref(Ea, Eb, D["w4"], D["b4"]).astype(np.float32)


def gate_ref(cand_s, cand_i, crit, flag, tau, k):
    """cand_s / cand_i / crit / flag [n, c_in] (flag >= 0: scored) -> (scores [n, k], ids [n, k], stat [n, 3] = scored, rejected before the
    list was full, length): a non-padding entry passes iff it is unscored or crit >= tau; the first k passing entries are the list"""
    cand_s, cand_i, crit, flag = np.asarray(cand_s, np.float32), np.asarray(cand_i), np.asarray(crit, np.float32), np.asarray(flag)
    tau = np.float32(tau)
    n, c_in = cand_i.shape
    out_s, out_i = np.full((n, k), -np.inf, np.float32), np.full((n, k), -1, np.int32)
    stat = np.zeros((n, 3), np.int32)
    for r in range(n):
        m = 0
        for j in range(c_in):
            if cand_i[r, j] < 0:
                continue
            scored = flag[r, j] >= 0
            stat[r, 0] += scored
            if scored and not crit[r, j] >= tau:
                stat[r, 1] += m < k
                continue
            if m < k:
                out_s[r, m], out_i[r, m] = cand_s[r, j], cand_i[r, j]
            m += 1
        stat[r, 2] = min(m, k)
    return out_s, out_i, stat
