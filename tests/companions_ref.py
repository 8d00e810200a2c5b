"""numpy reference of the niche companions (ltg_pair_pack / ltg_pair_companions).  D is an oracle discriminator dict
(oracle.ltg_oracle.init_discriminator: emb, w1, b1, w2, b2, w3, b3, w4 [h3, 1], b4 [1]).

    s(a, b) = b4 + sum_j w4[j] tanh(U[a][j] + V[b][j])      U = tanh(emb w1 + b1) w3[:h1]      V = tanh(emb w2 + b2) w3[h1:] + b3

pack_ref    the pre-activation a side adds to the fc layer (U or V) in fp64 -- what an image row stores as E = exp(2 x)
image_ref   E of pack_ref's x, clamped as the device clamps it
score_ref   the fp64 scores of GIVEN images: tanh of 0.5 log Eq + 0.5 log Ec -- with the device's own fp32 images it is the oracle of the
            pair kernel alone, with image_ref's it is the discriminator
lists_ref   ltg_topk's order over a score table: score descending, equal scores lower id first, -0.0 == +0.0, padding id -1 / score -inf
"""
import numpy as np

CLAMP = 40.0


def pack_ref(D, side, ids):
    """-> x [n, h3] float64, unclamped"""
    f = lambda a: np.asarray(a, np.float64)
    ids = np.asarray(ids, np.int64)
    h1 = D["w1"].shape[1]
    e = f(D["emb"])[ids]
    if side == "popular":
        return np.tanh(e @ f(D["w1"]) + f(D["b1"])) @ f(D["w3"])[:h1]
    assert side == "niche"
    return np.tanh(e @ f(D["w2"]) + f(D["b2"])) @ f(D["w3"])[h1:] + f(D["b3"])


def image_ref(x):
    return np.exp(2.0 * np.clip(np.asarray(x, np.float64), -CLAMP, CLAMP))


def score_ref(Eq, Ec, w4, b4):
    """Eq [n_q, >= h3], Ec [n_c, >= h3] (columns past h3 = len(w4) are ignored) -> [n_q, n_c] float64"""
    w4 = np.asarray(w4, np.float64).reshape(-1)
    h3 = w4.size
    lq = 0.5 * np.log(np.asarray(Eq, np.float64)[:, :h3])
    lc = 0.5 * np.log(np.asarray(Ec, np.float64)[:, :h3])
    b4 = float(np.asarray(b4, np.float64).reshape(-1)[0])
    out = np.empty((lq.shape[0], lc.shape[0]))
    for r in range(lq.shape[0]):
        out[r] = np.tanh(lc + lq[r]) @ w4 + b4
    return out


def eligible(q_gid, c_gid):
    return np.asarray(c_gid)[None, :] != np.asarray(q_gid)[:, None]


def lists_ref(S, q_gid, c_gid, k):
    """S [n_q, n_c] scores (any float type; compared as they are) -> (scores [n_q, k] of S's dtype, ids [n_q, k] int32)"""
    S = np.asarray(S)
    c_gid = np.asarray(c_gid, np.int64)
    ok = eligible(q_gid, c_gid)
    sc = np.full((S.shape[0], k), -np.inf, S.dtype)
    ids = np.full((S.shape[0], k), -1, np.int32)
    for r in range(S.shape[0]):
        loc = np.nonzero(ok[r])[0]
        o = loc[np.lexsort((c_gid[loc], -(S[r, loc] + 0.0)))[:k]]     # (+ 0.0: -0.0 and +0.0 are one key)
        sc[r, :o.size] = S[r, o]
        ids[r, :o.size] = c_gid[o]
    return sc, ids
