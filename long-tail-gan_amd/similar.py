#!/usr/bin/env python3
"""Similar-item CLI with recommend.py's surface:

    cd <dir holding config.ini> && python <repo>/long-tail-gan_amd/similar.py <dataset_dir> <checkpoint>
        [--k 20] [--space decoder|encoder] [--metric cosine|dot] [--items all|popular|niche|FILE]
        [--groups niche|pop:N --only NAME[,NAME...]] [--out similar.tsv] [--npz similar.npz]

restores a checkpoint written by train.py and keeps, for every query item, its k nearest items in the generator's item table: `decoder` =
the rows of W_p1t (what the model scores items with), `encoder` = the rows of W_q0 (what it reads histories with); `cosine` or `dot` of
the bf16 operand rows (ltg_item_neighbors: one fused kernel, the 'items x items' score matrix is never written).  An item is never its
own neighbour.  --items: the query items -- all, the popular or the niche items (load_pop_niche_tags' NICHE_TAGS), or a file of sids,
one per line.  --only NAME[,NAME...] keeps only NEIGHBOURS of those groups of --groups (longtail.py's groups: `niche` = popular / niche,
`pop:N` = pop0 .. pop<N-1>, pop0 = head): `--items popular --groups niche --only niche` is the shelf of niche neighbours of every head item.

Writes one TSV line per query item, `sid<TAB>sid_1,sid_2,...` in rank order (padding dropped), and with --npz the arrays items / ids /
scores.  The last stdout line: items, niche_share@k (neighbour slots that are niche items) and coverage@k (distinct neighbours /
n_items).  Under `python -m torch.distributed.run --nproc-per-node N` the items are sharded as in test.py; rank 0 writes.
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
    from ltgan import longtail as lt
else:
    from . import data_processing as dp
    from . import longtail as lt

MAX_K = 256       # LTG_NBR_MAX_K


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="similar.py", description="similar-item lists from a Long-Tail-GAN checkpoint")
    ap.add_argument("dataset_dir")
    ap.add_argument("checkpoint")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--space", choices=("decoder", "encoder"), default="decoder")
    ap.add_argument("--metric", choices=("cosine", "dot"), default="cosine")
    ap.add_argument("--items", default="all")
    ap.add_argument("--groups", default="niche")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default="similar.tsv")
    ap.add_argument("--npz", default=None)
    a = ap.parse_args(argv)
    if not 1 <= a.k <= MAX_K:
        ap.error("--k must be in [1, %d]" % MAX_K)
    a.only_groups = None
    try:
        a.group_kind, a.n_groups = lt.parse_groups(a.groups)
        if a.only is not None:
            a.only_groups = parse_only(a.only, lt.group_names(a.group_kind, a.n_groups))
    except ValueError as e:
        ap.error(str(e))
    return a


def parse_only(spec, names):
    """'NAME[,NAME...]' -> the sorted group indices; an unknown or repeated name, or none at all, raises ValueError"""
    out = []
    for part in spec.split(","):
        name = part.strip()
        if name not in names:
            raise ValueError("--only: unknown group %r (the groups are %s)" % (name, ", ".join(names)))
        if names.index(name) in out:
            raise ValueError("--only names group %r twice" % (name,))
        out.append(names.index(name))
    return sorted(out)


def query_items(spec, niche, n_items):
    """--items -> ascending int32 sids: all / popular / niche, or a file with one sid per line (kept in the file's order)"""
    is_niche = np.zeros(n_items, bool)
    is_niche[np.fromiter((int(x) for x in niche), np.int64, len(niche))] = True
    if spec == "all":
        return np.arange(n_items, dtype=np.int32)
    if spec == "niche":
        return np.nonzero(is_niche)[0].astype(np.int32)
    if spec == "popular":
        return np.nonzero(~is_niche)[0].astype(np.int32)
    with open(spec) as f:
        q = np.array([int(line) for line in f.read().split()], dtype=np.int64)
    if q.size and (q.min() < 0 or q.max() >= n_items):
        raise ValueError("--items %s: sid outside [0, %d)" % (spec, n_items))
    return q.astype(np.int32)


def write_similar(items, ids, scores, tsv_path=None, npz_path=None):
    """ids / scores [n_q, k] (padding id -1 dropped from the TSV); row r is query item items[r]"""
    items, ids = np.asarray(items), np.asarray(ids)
    if tsv_path:
        with open(tsv_path, "w") as f:
            for q, row in zip(items.tolist(), ids.tolist()):
                f.write("%d\t%s\n" % (q, ",".join(str(i) for i in row if i >= 0)))
    if npz_path:
        np.savez(npz_path, items=items.astype(np.int32), ids=ids.astype(np.int32), scores=np.asarray(scores, np.float32))


def similar_summary(ids, niche, n_items):
    """items, niche share@k (neighbour slots that are niche items) and coverage@k (distinct neighbours / n_items)"""
    ids = np.asarray(ids)
    nb = ids[ids >= 0]
    is_niche = np.zeros(n_items, bool)
    is_niche[np.fromiter((int(x) for x in niche), np.int64, len(niche))] = True
    return dict(items=int(ids.shape[0]), niche_share=float(is_niche[nb].mean()) if nb.size else float("nan"),
                coverage=float(np.unique(nb).size) / n_items)


def summary_line(m, k):
    return "items: %d\tniche_share@%d: %.6f\tcoverage@%d: %.6f" % (m["items"], k, m["niche_share"], k, m["coverage"])


def similar(args, h0_size, h1_size, h2_size, h3_size, LEARNING_RATE, precision="bf16", **_):
    from ltgan.serving import ItemNeighbors, ShardedItemNeighbors, close_model, open_model
    d = args.dataset_dir
    eng, _, _, rank, world, print = open_model(d, args.checkpoint, (h0_size, h1_size, h2_size, h3_size), LEARNING_RATE, precision)  # noqa: A001
    n_items = eng.I_global
    _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(d, "item2id.txt"), os.path.join(d, "item_list.txt"),
                                               os.path.join(d, "niche_items.txt"), n_items)
    labels = n_groups = None
    if args.only_groups is not None:
        labels, names = lt.build_groups(d, args.group_kind, args.n_groups, n_items)
        n_groups = len(names)
    q = query_items(args.items, niche, n_items)
    kw = dict(k=args.k, space=args.space, metric=args.metric, labels=labels, n_groups=n_groups, only=args.only_groups)
    nb = ShardedItemNeighbors(eng, **kw) if world > 1 else ItemNeighbors(eng, **kw)
    ids, scores = nb.run(q)
    m = similar_summary(ids, niche, n_items)
    if rank == 0:
        write_similar(q, ids, scores, args.out, args.npz)
    print(summary_line(m, args.k))
    close_model(world)
    return q, ids, scores, m


if __name__ == "__main__":
    a = parse_args(sys.argv[1:])
    from ltgan.train import read_config
    similar(a, **read_config())
