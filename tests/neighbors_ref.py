"""numpy reference of the item-to-item neighbours (ltg_item_pack / ltg_item_neighbors; include/ltg.h): the operand image bit for bit,
scores of image rows in fp64 with the per-pair error bound of the fp32 accumulation, and the lists by ltg_topk's total order."""
import numpy as np

KP = 608                      # K of the operand image (H zero-padded)
ACC_ULPS = 608 * 2.0 ** -23   # 608 accumulations of exact bf16 x bf16 products, at most one fp32 ulp of the running sum each


def f32_to_bf16(x):
    """round-to-nearest-even bf16 bits (uint16) of finite float32 values"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def bf16_to_f32(b):
    return (np.asarray(b).astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def pack_image(W, metric):
    """W [I, H] float32 -> [I, 608] uint16.  dot: bf16 RNE of the value.  cosine: squared norm summed in fp64, inv = float32(1 / sqrt),
    bf16 RNE of the single fp32 product x * inv; a zero row stays zero."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    I, H = W.shape
    assert H <= KP
    if metric == "cosine":
        n2 = (W.astype(np.float64) ** 2).sum(1)
        with np.errstate(divide="ignore"):
            inv = np.where(n2 > 0, 1.0 / np.sqrt(n2), 0.0).astype(np.float32)
        W = W * inv[:, None]                      # one fp32 product per element
    else:
        assert metric == "dot"
    img = np.zeros((I, KP), np.uint16)
    img[:, :H] = f32_to_bf16(W)
    return img


def scores64(q_img, t_img):
    """the exact products of the bf16 operands summed in fp64: [n_q, I]"""
    return bf16_to_f32(q_img).astype(np.float64) @ bf16_to_f32(t_img).astype(np.float64).T


def score_bound(q_img, t_img):
    """per pair: 608 * 2^-23 * sum_i |a_i b_i| -- what 608 fp32 accumulations of exact products can lose ([n_q, I]; <= 7.3e-5 for unit rows)"""
    return ACC_ULPS * (np.abs(bf16_to_f32(q_img)).astype(np.float64) @ np.abs(bf16_to_f32(t_img)).astype(np.float64).T)


def key32(s):
    """ltg_topk's order-preserving key of float32 scores (-0.0 == +0.0)"""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def eligible(n_items, item_lo, q_gid, labels=None, group_mask=0x1FF):
    """[n_q, n_items] bool: item j (global id item_lo + j) may be returned for query r"""
    gid = item_lo + np.arange(n_items, dtype=np.int64)
    ok = gid[None, :] != np.asarray(q_gid, np.int64)[:, None]
    if labels is not None:
        lab = np.minimum(np.asarray(labels)[item_lo:item_lo + n_items].astype(np.int64), 8)
        ok &= (((int(group_mask) >> lab) & 1) != 0)[None, :]
    return ok


def topk_lists(S, ok, k, item_lo=0):
    """S [n_q, I] float32 scores, ok [n_q, I] eligibility -> (scores [n_q, k] float32, ids [n_q, k] int32): score descending, equal
    scores lower global id first, padding id -1 / score -inf -- via the 64-bit (key, ~id) words the device orders by"""
    S = np.ascontiguousarray(S, dtype=np.float32)
    n, I = S.shape
    gid = (item_lo + np.arange(I, dtype=np.int64)).astype(np.uint32)
    comp = (key32(S).astype(np.uint64) << np.uint64(32)) | (~gid).astype(np.uint64)[None, :]
    comp[~ok] = 0
    if I > k:
        part = np.argpartition(comp, I - k, axis=1)[:, I - k:]
    else:
        part = np.broadcast_to(np.arange(I), (n, I)).copy()
    c = np.take_along_axis(comp, part, 1)
    o = np.argsort(c, axis=1)[:, ::-1]
    part, c = np.take_along_axis(part, o, 1), np.take_along_axis(c, o, 1)
    ids = np.full((n, k), -1, np.int32)
    sc = np.full((n, k), -np.inf, np.float32)
    m = part.shape[1]
    valid = c != 0
    ids[:, :m] = np.where(valid, part + item_lo, -1)
    sc[:, :m] = np.where(valid, np.take_along_axis(S, part, 1) + np.float32(0.0), -np.inf)
    return sc, ids


def neighbors(q_img, t_img, q_gid, k, labels=None, group_mask=0x1FF, item_lo=0, scores=None):
    """the reference lists of ltg_item_neighbors for scores that are exact in fp32 (or given)"""
    S = scores if scores is not None else (bf16_to_f32(q_img) @ bf16_to_f32(t_img).T)
    return topk_lists(S, eligible(t_img.shape[0], item_lo, q_gid, labels, group_mask), k, item_lo)


def brute_force(S, q_gid, k, labels=None, group_mask=0x1FF, item_lo=0):
    """the same lists by a plain loop and Python's sort (tests the vectorised form above)"""
    n, I = S.shape
    ids = np.full((n, k), -1, np.int32)
    sc = np.full((n, k), -np.inf, np.float32)
    for r in range(n):
        cand = []
        for j in range(I):
            g = item_lo + j
            if g == q_gid[r]:
                continue
            if labels is not None and not (group_mask >> min(int(labels[g]), 8)) & 1:
                continue
            cand.append((-float(S[r, j]), g))
        cand.sort()
        for i, (ns, g) in enumerate(cand[:k]):
            ids[r, i] = g
            sc[r, i] = np.float32(-ns) + np.float32(0.0)
    return sc, ids
