"""numpy reference of the list explanations (ltg_topk_explain; include/ltg.h): per (user row, list entry) the r history items of that
user nearest to the entry, built from neighbors_ref -- the scores are products of image rows, the lists ltg_topk's total order -- plus a
plain-loop version that checks the vectorised one and the inputs the exact-parity tests share."""
import numpy as np

import diversify_ref as D
import neighbors_ref as NR

HB = 64                       # EX_HB of csrc/ltg_explain.h: the history rows per block (the test histories straddle it)
MAX_TOP, MAX_R = 256, 8


def exact_scores(q_img, t_img):
    """the fp32 products of image rows; exact (any summation order) for images like diversify_ref.exact_image"""
    return NR.bf16_to_f32(q_img) @ NR.bf16_to_f32(t_img).T


def explain_lists(img, image_lo, ids, indptr, indices, hist_lo, top, r, scores=exact_scores):
    """img [rows, 608] uint16 (row i = global id image_lo + i), ids [n, k_in] int32 lists, (indptr, indices) the CSR histories (global id =
    hist_lo + index, ascending per row) -> (scores [n, top, r] float32, ids [n, top, r] int32): NR.topk_lists over the scores of every
    entry's image row against the image rows of the user's history, candidates = history items inside the image other than the entry;
    an entry outside the image gets paddings"""
    ids = np.asarray(ids, np.int64)
    n, rows = ids.shape[0], img.shape[0]
    out_s = np.full((n, top, r), -np.inf, np.float32)
    out_i = np.full((n, top, r), -1, np.int32)
    for u in range(n):
        h = hist_lo + np.asarray(indices[indptr[u]:indptr[u + 1]], np.int64)
        h = h[(h >= image_lo) & (h < image_lo + rows)]
        assert (np.diff(h) > 0).all()                                   # ascending: a position order is an id order
        g = ids[u, :top]
        e_in = np.nonzero((g >= image_lo) & (g < image_lo + rows))[0]
        if h.size == 0 or e_in.size == 0:
            continue
        S = scores(img[g[e_in] - image_lo], img[h - image_lo]).astype(np.float32)
        ok = h[None, :] != g[e_in][:, None]
        s, pos = NR.topk_lists(S, ok, r)                                # ("ids" = positions in h)
        out_s[u, e_in] = s
        out_i[u, e_in] = np.where(pos >= 0, h[np.maximum(pos, 0)], -1)
    return out_s, out_i


def explain_loop(img, image_lo, ids, indptr, indices, hist_lo, top, r):
    """the same table by plain loops and Python's sort (exact-score images only)"""
    f = NR.bf16_to_f32(img).astype(np.float64)
    n, rows = len(ids), img.shape[0]
    out_s = np.full((n, top, r), -np.inf, np.float32)
    out_i = np.full((n, top, r), -1, np.int32)
    for u in range(n):
        for e in range(top):
            g = int(ids[u][e])
            if not image_lo <= g < image_lo + rows:
                continue
            cand = []
            for x in indices[indptr[u]:indptr[u + 1]]:
                h = hist_lo + int(x)
                if image_lo <= h < image_lo + rows and h != g:
                    cand.append((-float(np.dot(f[g - image_lo], f[h - image_lo])), h))
            cand.sort()
            for j, (ns, h) in enumerate(cand[:r]):
                out_i[u, e, j] = h
                out_s[u, e, j] = np.float32(-ns) + np.float32(0.0)
    return out_s, out_i


# ---------------------------------------------------------------------------------------------------------------- exact inputs
EXACT_CASES = [(1, 1, 1), (20, 16, 3), (100, 17, 8), (100, 100, 3), (256, 256, 8), (300, 256, 1)]       # (k_in, top, r)
EXACT_ROWS = 37
ROW_MINUS1, ROW_STRAY, ROW_EMPTY, ROW_SELF, ROW_OUTSIDE, ROW_BELOW = 5, 6, 7, 9, 4, 3


def history_lengths(r):
    return [0, 1, r - 1, 15, 16, 17, HB - 1, HB, HB + 1, 3 * HB + 5, 300]


def exact_inputs(k_in, top, r, image_rows, image_lo=0, rows=EXACT_ROWS, seed=17):
    """-> (ids [rows, k_in] int32, indptr, indices): lists of distinct random ids of the image -- row ROW_MINUS1 with a -1 in the middle
    of the explained part, ROW_STRAY with one id outside the image, ROW_EMPTY all padding -- and ascending histories of GLOBAL ids
    (hist_lo = 0) whose lengths cycle through history_lengths(r); ROW_SELF's history holds entries of its own list, ROW_OUTSIDE's an id
    past the image, and with image_lo > 0 ROW_BELOW's one in front of it"""
    rng = np.random.default_rng(seed + 1000 * k_in + 10 * top + r)
    ids = np.stack([image_lo + rng.choice(image_rows, k_in, replace=False) for _ in range(rows)]).astype(np.int32)
    ids[ROW_MINUS1, top // 2] = -1
    ids[ROW_STRAY, min(1, top - 1)] = image_lo + image_rows if image_lo == 0 else image_lo - 1
    ids[ROW_EMPTY, :] = -1
    lens = history_lengths(r)
    hist = []
    for u in range(rows):
        h = image_lo + rng.choice(image_rows, lens[u % len(lens)], replace=False).astype(np.int64)
        if u == ROW_SELF:
            h = np.concatenate([h, ids[u, :min(3, top)].astype(np.int64)])
        if u == ROW_OUTSIDE:
            h = np.concatenate([h, [image_lo + image_rows + 3]])
        if u == ROW_BELOW and image_lo > 8:
            h = np.concatenate([h, [8]])
        hist.append(np.unique(h))
    indptr = np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int32)
    indices = np.concatenate(hist).astype(np.int32)
    return ids, indptr, indices


exact_image = D.exact_image
