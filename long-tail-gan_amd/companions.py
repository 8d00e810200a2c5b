#!/usr/bin/env python3
"""Niche-companions CLI with similar.py's surface:

    cd <dir holding config.ini> && python <repo>/long-tail-gan_amd/companions.py <dataset_dir> <checkpoint>
        [--k 20] [--items popular|niche|FILE] [--out companions.tsv] [--npz companions.npz]

restores a checkpoint written by train.py and asks its DISCRIMINATOR -- the network trained on (popular, niche) pairs that real users hold
-- which items belong beside each query item: for a popular query its k likeliest niche companions (the head-to-tail shelf), for a niche
query its k likeliest popular anchors.  The score of a pair is the discriminator's logit without dropout (ltg_pair_companions: one fused
kernel, the 'queries x candidates' score table is never written).  --items: the query items -- the popular or the niche items
(load_pop_niche_tags' NICHE_TAGS), or a file of sids of ONE side, one per line; the candidates are the other side.  Both are restricted to
the items with features (load_valid_item_ids): the discriminator never saw any other (Q9).

Writes one TSV line per query item, `sid<TAB>sid_1:prob_1,sid_2:prob_2,...` in rank order with prob = sigmoid(score) to 6 places (padding
dropped), and with --npz the arrays items / ids / scores.  The last stdout line: items, coverage@k (distinct companions / candidates) and
mean_prob@1.  Under `python -m torch.distributed.run --nproc-per-node N` the candidates are sharded by item slab; rank 0 writes.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ltgan  # noqa: F401  (alias of this package directory)
    from ltgan import data_processing as dp
    from ltgan.similar import query_items
else:
    from . import data_processing as dp
    from .similar import query_items

MAX_K = 256       # LTG_PAIR_MAX_K


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="companions.py", description="niche companions of items from a Long-Tail-GAN checkpoint's discriminator")
    ap.add_argument("dataset_dir")
    ap.add_argument("checkpoint")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--items", default="popular")
    ap.add_argument("--out", default="companions.tsv")
    ap.add_argument("--npz", default=None)
    a = ap.parse_args(argv)
    if not 1 <= a.k <= MAX_K:
        ap.error("--k must be in [1, %d]" % MAX_K)
    if a.items == "all":
        ap.error("--items all: the queries are one side of the popular / niche split (popular, niche or a file of sids of one side)")
    return a


def split_sides(spec, niche, valid, n_items):
    """--items -> (side of the queries, queries, candidates): the queries `spec` selects (similar.py's query_items; a file keeps its order)
    and the items of the other side, ascending, both restricted to `valid` (the ids with features).  A file that mixes the sides raises."""
    ok = np.zeros(n_items, bool)
    ok[np.fromiter((int(x) for x in valid), np.int64, len(valid))] = True
    is_niche = np.zeros(n_items, bool)
    is_niche[np.fromiter((int(x) for x in niche), np.int64, len(niche))] = True
    q = query_items(spec, niche, n_items)
    q = q[ok[q]]
    if spec in ("popular", "niche"):
        side = spec
    else:
        sides = np.unique(is_niche[q])
        if sides.size > 1:
            raise ValueError("--items %s mixes popular and niche items: the queries must be of one side" % spec)
        side = "niche" if sides.size and sides[0] else "popular"
    cand = np.nonzero(ok & (~is_niche if side == "niche" else is_niche))[0].astype(np.int32)
    return side, q.astype(np.int32), cand


def sigmoid(s):
    s = np.asarray(s, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-s))


def write_companions(items, ids, scores, tsv_path=None, npz_path=None):
    """ids / scores [n_q, k] (padding id -1 dropped from the TSV); row r is query item items[r]"""
    items, ids, scores = np.asarray(items), np.asarray(ids), np.asarray(scores, np.float32)
    if tsv_path:
        prob = sigmoid(scores)
        with open(tsv_path, "w") as f:
            for q, row, pr in zip(items.tolist(), ids.tolist(), prob.tolist()):
                f.write("%d\t%s\n" % (q, ",".join("%d:%.6f" % (i, p) for i, p in zip(row, pr) if i >= 0)))
    if npz_path:
        np.savez(npz_path, items=items.astype(np.int32), ids=ids.astype(np.int32), scores=scores)


def companions_summary(ids, scores, n_cand):
    """items, coverage@k (distinct companions / candidates) and the mean probability of the first companion"""
    ids, scores = np.asarray(ids), np.asarray(scores)
    nb = ids[ids >= 0]
    first = ids[:, 0] >= 0 if ids.size else np.zeros(0, bool)
    return dict(items=int(ids.shape[0]), coverage=float(np.unique(nb).size) / n_cand if n_cand else float("nan"),
                mean_prob=float(sigmoid(scores[first, 0]).mean()) if first.any() else float("nan"))


def summary_line(m, k):
    return "items: %d\tcoverage@%d: %.6f\tmean_prob@1: %.6f" % (m["items"], k, m["coverage"], m["mean_prob"])


def companions(args, h0_size, h1_size, h2_size, h3_size, LEARNING_RATE, precision="bf16", **_):
    from ltgan.serving import PairCompanions, ShardedPairCompanions, close_model, open_model
    d = args.dataset_dir
    eng, _, _, rank, world, print = open_model(d, args.checkpoint, (h0_size, h1_size, h2_size, h3_size), LEARNING_RATE, precision)  # noqa: A001
    n_items = eng.I_global
    show2id, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(d, "item2id.txt"), os.path.join(d, "item_list.txt"),
                                                     os.path.join(d, "niche_items.txt"), n_items)
    valid = dp.load_valid_item_ids(os.path.join(d, "item_list.txt"), show2id)
    side, q, cand = split_sides(args.items, niche, valid, n_items)
    kw = dict(k=args.k, queries=side)
    pc = ShardedPairCompanions(eng, **kw) if world > 1 else PairCompanions(eng, **kw)
    ids, scores = pc.run(q, cand)
    m = companions_summary(ids, scores, cand.size)
    if rank == 0:
        write_companions(q, ids, scores, args.out, args.npz)
    print(summary_line(m, args.k))
    close_model(world)
    return q, ids, scores, m


if __name__ == "__main__":
    a = parse_args(sys.argv[1:])
    from ltgan.train import read_config
    companions(a, **read_config())
