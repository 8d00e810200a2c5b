"""The numpy reference of the replay of an exploration log (ltg_list_mass / ltg_replay_rows / serving.Replay): the mass of
a LOGGED list under target Plackett-Luce policies (T_p, F'), the target log-probability of every logged slot, the prefix importance
weights and their per-group sums, everything in float64 from the float32 logits and the float32 inv_temp.

A second, independent part enumerates every ordered list of the eight-item catalogue of explore_ref (PAIR_LOGITS, item 5 a fold-in
item, k = 3) with its probability under a policy, so that the estimator can be held to the target's exact expectation."""
import itertools

import numpy as np

import explore_ref as E

F32 = np.float32
ENUM_FOLD = 5                                            # the fold-in item of the enumeration
ENUM_K = 3
ENUM_PAIRS = (((1.0, 0), (0.5, 0)), ((1.0, 0), (2.0, 1)), ((0.5, 1), (1.0, 1)))      # (T0, F0) -> (T1, F')


def ineligible(fold, excl, item_lo=0):
    """the slab's columns that are not eligible under the target: fold-in items, and the GLOBAL ids of excl that the slab owns"""
    inel = np.asarray(fold, bool).copy()
    for e in excl:
        if item_lo <= e < item_lo + len(inel):
            inel[e - item_lo] = True
    return inel


def list_mass(s, fold, ids, inv_temps, excl=(), f_in=0, item_lo=0):
    """ltg_list_mass on one row of one slab: s / fold [I] over the slab's columns, ids [k] the logged list (GLOBAL, -1 = padding), excl the
    target's head (GLOBAL ids) -> (score [k] float32, state [k] int32, M float32, rest [n_pol] float64)"""
    I, k = len(s), len(ids)
    inel = ineligible(fold, excl, item_lo)
    score, state = np.full(k, -np.inf, F32), np.zeros(k, np.int32)
    taken = np.zeros(I, bool)
    for j, g in enumerate(ids):
        if j >= f_in and item_lo <= g < item_lo + I:
            c = g - item_lo
            if inel[c]:
                state[j] = 2
            else:
                state[j], score[j], taken[c] = 1, s[c], True
    el = ~inel
    M = s[el].max() if el.any() else F32(-np.inf)
    left = s[el & ~taken].astype(np.float64)
    left = left[np.isfinite(left)]
    rest = np.array([np.exp((left - np.float64(M)) * np.float64(F32(it))).sum() if left.size else 0.0 for it in inv_temps], np.float64)
    return score, state, F32(M), rest


def combine(parts, inv_temps):
    """the slabs' (score, state, M, rest) of one row -> the whole row's, as the host combines them across item shards (float64 rest)"""
    M = F32(max(p[2] for p in parts))
    rest = np.zeros(len(inv_temps))
    for p in parts:
        if np.isfinite(p[2]):
            rest += p[3] * np.exp((np.float64(p[2]) - np.float64(M)) * np.array([np.float64(F32(it)) for it in inv_temps]))
    return np.maximum.reduce([p[0] for p in parts]), np.maximum.reduce([p[1] for p in parts]), M, rest


def replay_row(ids, logp0, y, head, f_in, score, state, M, rest, inv_temps, labels, n_groups, clip):
    """ltg_replay_rows on one row in float64 -> dict(logp1 [P, k] (0 padding / matching head, -inf unsupported), x [P, k] (nan where no
    sampled supported entry), c [P, k], w [P, k], A / B [P, n_groups + 1], W [P], first_bad)"""
    k, P, G = len(ids), len(inv_temps), int(n_groups)
    ids = np.asarray(ids)
    real = ids >= 0
    sup = np.zeros(k, bool)
    for j in range(k):
        if real[j]:
            sup[j] = (head[j] == ids[j]) if j < f_in else (state[j] == 1)
    bad = np.nonzero(real & ~sup)[0]
    first_bad = int(bad[0]) if bad.size else k
    samp = sup & (np.arange(k) >= f_in)
    out = dict(logp1=np.zeros((P, k)), x=np.full((P, k), np.nan), c=np.zeros((P, k)), w=np.zeros((P, k)), A=np.zeros((P, G + 1)),
               B=np.zeros((P, G + 1)), W=np.zeros(P), first_bad=first_bad)
    lab = np.where(real, np.asarray(labels)[np.where(real, ids, 0)], 255).astype(np.int64)
    last = int(np.nonzero(real)[0][-1]) if real.any() else -1
    for p, it in enumerate(inv_temps):
        x = np.where(samp, (np.where(samp, np.asarray(score, np.float64), 0.0) - np.float64(M)) * np.float64(F32(it)), -np.inf)
        e = np.where(samp, np.exp(x), 0.0)
        tail = np.cumsum(e[::-1])[::-1] + np.float64(rest[p])
        with np.errstate(divide="ignore", invalid="ignore"):
            l1 = np.where(samp, x - np.log(tail), np.where(real & ~sup, -np.inf, 0.0))
        d = np.where(sup, np.where(sup, l1, 0.0) - np.asarray(logp0, np.float64), 0.0)
        c = np.cumsum(d)
        w = np.where(real & (np.arange(k) < first_bad), np.exp(np.minimum(c, np.log(np.float64(clip)))), 0.0)
        out["logp1"][p], out["x"][p], out["c"][p], out["w"][p] = l1, np.where(samp, x, np.nan), c, w
        wy = w * np.asarray(y, np.float64)
        for g in range(G):
            out["A"][p, g], out["B"][p, g] = wy[lab == g].sum(), w[lab == g].sum()
        out["A"][p, G], out["B"][p, G] = wy.sum(), w.sum()
        out["W"][p] = 0.0 if first_bad < k else (w[last] if last >= 0 else np.exp(min(0.0, np.log(np.float64(clip)))))
    return out


def replay_full_row(s, fold, ids, logp0, y, f_in, inv_temps, labels, n_groups, clip):
    """the whole definition on one row of the whole catalogue: the target's head, the mass, the weights -> replay_row's dict plus
    head / score / state / M / rest"""
    head = E.plain_topk(s, fold, f_in)[0] if f_in else np.zeros(0, np.int32)
    score, state, M, rest = list_mass(s, fold, ids, inv_temps, excl=head, f_in=f_in)
    out = replay_row(ids, logp0, y, head, f_in, score, state, M, rest, inv_temps, labels, n_groups, clip)
    out.update(head=head, score=score, state=state, M=M, rest=rest)
    return out


# ---------------------------------------------------------------------------------------------- the exact enumeration
def enumerate_policy(T, F, logits=E.PAIR_LOGITS, fold_item=ENUM_FOLD, k=ENUM_K):
    """every ordered list of k eligible items with its probability under the policy (T, F): the plain top-F, then Plackett-Luce at T over
    what is left -> (lists [n, k] int32, prob [n] float64, logp [n, k] float64); lists outside the policy's support are not returned"""
    I = len(logits)
    fold = np.zeros(I, bool)
    fold[fold_item] = True
    head = list(E.plain_topk(logits, fold, F)[0]) if F else []
    it = np.float64(E.inv_temp_of(T))
    w = np.exp(logits.astype(np.float64) * it)
    pool = [i for i in range(I) if not fold[i] and i not in head]
    lists, probs, logps = [], [], []
    for tail in itertools.permutations(pool, k - F):
        lp = [0.0] * F
        for n_taken, i in enumerate(tail):
            left = sum(float(w[m]) for m in pool if m not in tail[:n_taken])      # (positive terms only)
            lp.append(float(np.log(w[i] / left)))
        lists.append(head + list(tail))
        logps.append(lp)
        probs.append(float(np.exp(np.sum(lp))))
    return np.array(lists, np.int32), np.array(probs), np.array(logps)


def enum_tables(seed=11):
    """the fixed reward table Y[item][slot] and the labels {0, 1, 2 | 3 .. 7} of the identity checks"""
    Y = np.random.default_rng(seed).random((8, ENUM_K))
    return Y, np.array([0, 0, 0, 1, 1, 1, 1, 1], np.uint8)


def target_value(T, F, Y, labels, n_groups=2):
    """the target policy's exact expectation per group (slot n_groups = all) of sum_j Y[id_j][j], and of the number of slots -> (A, B)"""
    lists, prob, _ = enumerate_policy(T, F)
    A, B = np.zeros(n_groups + 1), np.zeros(n_groups + 1)
    for ids, p in zip(lists, prob):
        for j, i in enumerate(ids):
            for g in (int(labels[i]), n_groups):
                A[g] += p * Y[i, j]
                B[g] += p
    return A, B
