"""The numpy reference of the exploration lists (ltg_topk_sample / ltg_topk_sample_mass / ltg_topk_sample_finish): top-K
sampled without replacement under the Plackett-Luce policy at temperature T, optionally behind a fixed head, with the conditional
log-probability of every pick.

The draw is Gumbel-top-k.  The noise comes from oracle.ltg_oracle.rng_uniform (the counter RNG the kernels share bit for bit) at stream 8,
counter = the draw, element = global row * n_items_global + global id; g = -log(-log(u)) in float32 (numpy's float32 log -- the one place
where the device may differ, by the rounding of two logf).  key = s * inv_temp + g in float32: one multiply, one add, numpy never
contracts them.  The mass and logp are computed in float64 from the float32 logits and the float32 inv_temp.

A second, independent function restates the definition sequentially: draw one item from the renormalised distribution over what is left,
record its probability, remove it, repeat."""
import numpy as np

from oracle import ltg_oracle as O

STREAM_SERVE_GUMBEL = 8
F32 = np.float32
PAIR_LOGITS = np.array([0, .3, -.4, .9, .5, -.2, .7, .1], F32)        # the eight-item catalogue of the distribution checks


def inv_temp_of(T):
    """float32(1 / T), formed on the host in double as serving.Explore forms it"""
    return F32(1.0 / float(T))


def gumbel_of_uniform(u):
    """g = -log(-log(u)) in float32; u == 0 -> -inf"""
    u = np.asarray(u, F32)
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def counter_noise(seed, draw, row, n_items_global, gids):
    """the Gumbel noise of the GLOBAL row `row` at the GLOBAL ids gids -> float32 [len(gids)]"""
    idx = np.uint64(row) * np.uint64(n_items_global) + np.asarray(gids).astype(np.uint64)
    return gumbel_of_uniform(O.rng_uniform(seed, STREAM_SERVE_GUMBEL, draw, idx).astype(F32))


def keys_of(s, inv_temp, g):
    """key = s * inv_temp + g, float32 multiply then float32 add"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(s, F32) * F32(inv_temp)).astype(F32) + np.asarray(g, F32)


def order_of(key, gid):
    """ltg_topk's order: key descending (-0.0 == +0.0), equal keys the lower id first -> positions"""
    return np.lexsort((np.asarray(gid), -np.asarray(key, F32)))


def plain_topk(s, fold, k, gid=None):
    """ltg_topk of one row: s [I] float32, fold [I] bool -> (ids [k] int32 padded with -1, scores [k] padded with -inf)"""
    gid = np.arange(len(s)) if gid is None else np.asarray(gid)
    el = np.nonzero(~np.asarray(fold))[0]
    o = el[order_of(s[el], gid[el])][:k]
    ids, sc = np.full(k, -1, np.int32), np.full(k, -np.inf, F32)
    ids[:len(o)], sc[:len(o)] = gid[o], s[o]
    return ids, sc


def sample_slab(s, fold, k, inv_temp, g, excl=(), item_lo=0):
    """ltg_topk_sample on one row of one slab: s / fold / g [I] over the slab's columns, excl = GLOBAL ids that are not eligible
    (those outside the slab and padding index nothing) -> (ids [k] GLOBAL int32 padded -1, keys [k] float32 padded -inf)"""
    I = len(s)
    inel = np.asarray(fold).copy()
    for e in excl:
        if item_lo <= e < item_lo + I:
            inel[e - item_lo] = True
    el = np.nonzero(~inel)[0]
    key = keys_of(s[el], inv_temp, np.asarray(g, F32)[el])
    o = order_of(key, el)[:k]
    ids, ks = np.full(k, -1, np.int32), np.full(k, -np.inf, F32)
    ids[:len(o)], ks[:len(o)] = el[o] + item_lo, key[o]
    return ids, ks


def mass_of(s, fold, inv_temp, picks, excl=(), item_lo=0):
    """ltg_topk_sample_mass on one row of one slab, in float64 -> (scores [len(picks)] float32, M float32, rest float64)"""
    I = len(s)
    inel = np.asarray(fold).copy()
    for e in excl:
        if item_lo <= e < item_lo + I:
            inel[e - item_lo] = True
    sc = np.full(len(picks), -np.inf, F32)
    picked = np.zeros(I, bool)
    for j, p in enumerate(picks):
        if item_lo <= p < item_lo + I:
            sc[j] = s[p - item_lo]
            picked[p - item_lo] = True
    el = ~inel
    M = s[el].max() if el.any() else F32(-np.inf)
    left = s[el & ~picked].astype(np.float64)
    left = left[np.isfinite(left)]
    rest = float(np.exp((left - np.float64(M)) * np.float64(F32(inv_temp))).sum()) if left.size else 0.0
    return sc, F32(M), rest


def logp_of(sc, M, rest, inv_temp):
    """ltg_topk_sample_finish in float64: sc [m] the picks' logits (-inf = padding) -> (logp [m] float64, x [m] float64)"""
    sc64 = np.asarray(sc, np.float64)
    real = np.isfinite(sc64)
    x = np.where(real, (np.where(real, sc64, 0.0) - np.float64(M)) * np.float64(F32(inv_temp)), -np.inf)
    e = np.where(real, np.exp(x), 0.0)
    tail = np.cumsum(e[::-1])[::-1] + rest
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.where(real, x - np.log(tail), 0.0)
    return lp, x


def explore_row(s, fold, k, F, inv_temp, g):
    """the whole definition on one row of the whole catalogue -> dict(ids [k], scores [k], keys [k - F], logp [k] float64, x [k - F], head)"""
    head, head_s = plain_topk(s, fold, F) if F else (np.zeros(0, np.int32), np.zeros(0, F32))
    ids, keys = sample_slab(s, fold, k - F, inv_temp, g, excl=head)
    sc, M, rest = mass_of(s, fold, inv_temp, ids, excl=head)
    lp, x = logp_of(sc, M, rest, inv_temp)
    return dict(ids=np.concatenate([head, ids]).astype(np.int32), scores=np.concatenate([head_s, sc]).astype(F32), keys=keys,
                logp=np.concatenate([np.zeros(F), lp]), x=x, head=head, M=M, rest=rest)


def sequential_row(s, fold, k, F, inv_temp, g):
    """the plain sequential definition fed the same noise: the head, then k - F times: the distribution exp(x) / sum over what is
    left, one Gumbel-max draw from it (log p + g, equal values the lower id), its log-probability, remove it -> (ids, logp) lists"""
    left = [i for i in range(len(s)) if not fold[i]]
    ids, lps = [], []
    for _ in range(F):
        if not left:
            break
        best = min(left, key=lambda i: (-float(s[i]) if s[i] == s[i] else 0.0, i))
        ids.append(best)
        lps.append(0.0)
        left.remove(best)
    it = float(F32(inv_temp))
    for _ in range(k - F):
        if not left:
            break
        x = np.array([float(s[i]) * it for i in left])
        top = x.max()
        if np.isinf(top):                                # every logit left is -inf: outside the contract of logp, the ids stay defined
            logp = np.full(len(left), -np.inf)
        else:
            logp = x - top - np.log(np.exp(x - top).sum())
        val = logp + np.array([float(g[i]) for i in left])
        if np.isinf(top):
            val = np.array([float(keys_of(s[i], inv_temp, g[i])) for i in left])
        j = min(range(len(left)), key=lambda t: (-val[t], left[t]))
        ids.append(left[j])
        lps.append(float(logp[j]))
        left.pop(j)
    return ids, lps


def near_tie(s, fold, k, inv_temp, g, excl=(), gap=1e-5):
    """the row's top-(k + 1) reference keys hold an adjacent pair closer than `gap`: the device's two logf may order them the other way"""
    _, ks = sample_slab(s, fold, k + 1, inv_temp, g, excl=excl)
    ks = ks[np.isfinite(ks)].astype(np.float64)
    return bool(ks.size > 1 and (ks[:-1] - ks[1:]).min() < gap)


# ---------------------------------------------------------------------------------------------- the distribution check
def pair_probabilities(T):
    """the Plackett-Luce probability of every ordered pair of the eight-item catalogue at temperature T -> {(a, b): p}"""
    w = np.exp(PAIR_LOGITS.astype(np.float64) * np.float64(inv_temp_of(T)))
    p = w / w.sum()
    return {(a, b): p[a] * p[b] / (1.0 - p[a]) for a in range(8) for b in range(8) if a != b}


def pair_chi2(pairs, T):
    """chi-square of the observed ordered pairs [n, 2] against pair_probabilities(T) -> (statistic, smallest expected cell)"""
    pairs = np.asarray(pairs)
    n = pairs.shape[0]
    obs = np.zeros((8, 8))
    np.add.at(obs, (pairs[:, 0], pairs[:, 1]), 1)
    chi, low = 0.0, np.inf
    for (a, b), p in pair_probabilities(T).items():
        chi += (obs[a, b] - n * p) ** 2 / (n * p)
        low = min(low, n * p)
    assert obs.trace() == 0
    return chi, low


def pair_lists(T, seed=98765, draw=0, n=16384):
    """the reference's lists of the distribution check: n rows of the same eight logits, k = 2 -> ids [n, 2]"""
    gid = np.arange(8)
    fold = np.zeros(8, bool)
    it = inv_temp_of(T)
    return np.stack([sample_slab(PAIR_LOGITS, fold, 2, it, counter_noise(seed, draw, r, 8, gid))[0] for r in range(n)])


# ---------------------------------------------------------------------------------------------- rows for the parity tests
RNG_CASES = [(5000, 20, 1.0), (1027, 100, 0.5), (5000, 20, 0.1)]      # (n_items, k, T): Gaussian logits of std 2, 256 rows each
RNG_ROWS = 256


def rng_case(case, seed=98765):
    """the rows of RNG-mode case `case` -> (logits [256, I] float32, fold [256, I] bool, k, inv_temp, seed).  The share of rows with a
    near-tie among the top k + 1 keys depends on the draw of the logits: at (1027, 100, 0.5) about 44 keys per unit lie around the
    100th, so a row has a gap below 1e-5 with probability near 2.5 %, and of five data seeds tried one gave 0.8 %, two 2.3 %, one 3.1 %
    and one 3.9 %.  The data seed is fixed to the one at 0.8 %, so that the exact-id check of the GPU test covers 98 % of the rows."""
    I, k, T = RNG_CASES[case]
    rng = np.random.default_rng(8000 + case)
    logits = (2.0 * rng.standard_normal((RNG_ROWS, I))).astype(F32)
    fold = rng.random((RNG_ROWS, I)) < 0.01
    return logits, fold, k, inv_temp_of(T), seed


def rng_case_reference(case, draw=0):
    """-> (ids [256, k], keys [256, k], near-tie flags [256], all reference keys [256, I] with nan at fold-in items)"""
    logits, fold, k, it, seed = rng_case(case)
    n, I = logits.shape
    gid = np.arange(I)
    ids, keys, tie, allk = np.empty((n, k), np.int32), np.empty((n, k), F32), np.zeros(n, bool), np.full((n, I), np.nan, F32)
    for r in range(n):
        g = counter_noise(seed, draw, r, I, gid)
        ids[r], keys[r] = sample_slab(logits[r], fold[r], k, it, g)
        tie[r] = near_tie(logits[r], fold[r], k, it, g)
        allk[r] = np.where(fold[r], np.nan, keys_of(logits[r], it, g))
    return ids, keys, tie, allk


KINDS = ("regular", "equal", "short", "allfold", "neginf", "zeros", "fewkeys")


def build_rows(seed, I, kinds=KINDS, reps=2):
    """rows of every kind over I items -> (logits [n, I] float32, fold [n, I] bool, g [n, I] float32 injected noise, kinds [n])
      regular   Gaussian logits of std 2, a few fold-in items, Gumbel noise
      equal     every logit and every noise value equal: the order is the ids'
      short     all but a few items are fold-in items: fewer eligible than most k
      allfold   every item is a fold-in item
      neginf    a third of the logits are -inf
      zeros     logits -0.0 / +0.0 and noise -0.0 / +0.0: every key is a zero of either sign, all equal
      fewkeys   zero noise and logits out of five values, two of them neighbouring floats: many equal keys around every threshold"""
    rng = np.random.default_rng(seed)
    rows = []
    for kind in kinds * reps:
        s = (2.0 * rng.standard_normal(I)).astype(F32)
        fold = rng.random(I) < 0.05
        g = gumbel_of_uniform(rng.random(I, dtype=F32))
        if kind == "equal":
            s[:], g[:] = F32(0.75), F32(-0.5)
        elif kind == "short":
            fold[:] = True
            fold[rng.choice(I, min(I, 3), replace=False)] = False
        elif kind == "allfold":
            fold[:] = True
        elif kind == "neginf":
            s[rng.random(I) < 0.33] = -np.inf
        elif kind == "zeros":
            s = np.where(rng.random(I) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
            g = np.where(rng.random(I) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
        elif kind == "fewkeys":
            vals = np.array([1.0, np.nextafter(F32(1.0), F32(2.0)), -3.0, 2.5, 1.0 - 2.0 ** -24], F32)
            s = vals[rng.choice(5, I, p=[0.3, 0.3, 0.1, 0.05, 0.25])]
            g = np.zeros(I, F32)
        rows.append((s, fold, g, kind))
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), [r[3] for r in rows])


def csr_of(fold, lo=0, hi=None):
    """the fold-in rows of the columns lo .. hi as a CSR with LOCAL ids -> (indptr int32, indices int32)"""
    sub = np.asarray(fold)[:, lo:hi]
    indptr = np.concatenate([[0], np.cumsum(sub.sum(1))]).astype(np.int32)
    indices = np.nonzero(sub)[1].astype(np.int32)
    return indptr, (indices if indices.size else np.zeros(1, np.int32))
