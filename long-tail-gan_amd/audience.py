#!/usr/bin/env python3
"""Item-audience CLI with similar.py's surface:

    cd <dir holding config.ini> && python <repo>/long-tail-gan_amd/audience.py <dataset_dir> <checkpoint>
        [--k 100] [--items all|popular|niche|FILE] [--split test|validation] [--keep-prob 0.75] [--score logprob|logit]
        [--out audience.tsv] [--npz audience.npz]

restores a checkpoint written by train.py, runs recommend.py's forward over the users of `<split>_tr.csv` (the same chunks, dropout and RNG
counter, so the audiences come from the forward recommend.py ranks) and keeps, for every query item, the k users the model thinks
likeliest to take it: the largest `logprob` = logit - lse (the log-probability the user's softmax gives the item; raw logits are not
comparable across users) or, with --score logit, the largest raw logit.  A user whose fold-in row already holds the item is never listed.
The selection runs down the columns of each chunk's logits on the GPU (ltg_item_audience + ltg_topk_merge across chunks: the logits never
leave the GPU and no 'users x items' score matrix is written); no user lists are computed.  --items: the query items -- all, the popular
or the niche items (load_pop_niche_tags' NICHE_TAGS), or a file of sids, one per line.

Writes one TSV line per query item, `sid<TAB>uid_1,uid_2,...` in rank order (padding dropped; uid = the CSV's uid, as recommend.py numbers
users), and with --npz the arrays items / uids / scores (uids: -1 = padding).  The last stdout line: items, users and user_coverage@k
(distinct users appearing in any list / users).  Under `python -m torch.distributed.run --nproc-per-node N` the items are sharded as in
test.py; rank 0 writes.
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
    from ltgan.recommend import RNG_STEP
    from ltgan.similar import query_items
else:
    from . import data_processing as dp
    from .recommend import RNG_STEP
    from .similar import query_items

MAX_K = 256       # LTG_AUD_MAX_K


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="audience.py", description="item audiences (the k likeliest users of every item) from a Long-Tail-GAN checkpoint")
    ap.add_argument("dataset_dir")
    ap.add_argument("checkpoint")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--items", default="all")
    ap.add_argument("--split", choices=("test", "validation"), default="test")
    ap.add_argument("--keep-prob", type=float, default=0.75)
    ap.add_argument("--score", choices=("logprob", "logit"), default="logprob")
    ap.add_argument("--out", default="audience.tsv")
    ap.add_argument("--npz", default=None)
    a = ap.parse_args(argv)
    if not 1 <= a.k <= MAX_K:
        ap.error("--k must be in [1, %d]" % MAX_K)
    if not 0.0 < a.keep_prob <= 1.0:
        ap.error("--keep-prob must be in (0, 1]")
    return a


def write_audience(items, rows, scores, uid_start, tsv_path=None, npz_path=None):
    """rows / scores [n_q, k]: user rows of the split (padding -1 dropped from the TSV) and their scores; line r is query item items[r];
    uid = uid_start + row.  -> the uids [n_q, k] int64 (-1 = padding)"""
    items, rows = np.asarray(items), np.asarray(rows)
    uids = np.where(rows >= 0, rows.astype(np.int64) + int(uid_start), -1)
    if tsv_path:
        with open(tsv_path, "w") as f:
            for q, line in zip(items.tolist(), uids.tolist()):
                f.write("%d\t%s\n" % (q, ",".join(str(u) for u in line if u >= 0)))
    if npz_path:
        np.savez(npz_path, items=items.astype(np.int32), uids=uids, scores=np.asarray(scores, np.float32))
    return uids


def audience_summary(rows, n_users):
    """items, users and user coverage@k (distinct users appearing in any list / users)"""
    rows = np.asarray(rows)
    seen = rows[rows >= 0]
    return dict(items=int(rows.shape[0]), users=int(n_users), coverage=float(np.unique(seen).size) / max(1, int(n_users)))


def summary_line(m, k):
    return "items: %d\tusers: %d\tuser_coverage@%d: %.6f" % (m["items"], m["users"], k, m["coverage"])


def audience(args, h0_size, h1_size, h2_size, h3_size, LEARNING_RATE, precision="bf16", batch_size_test=20000, **_):
    from ltgan.dataset import EvalData
    from ltgan.serving import Audience, Recommender, ShardedRecommender, close_model, open_model
    d = args.dataset_dir
    eng, lo, hi, rank, world, print = open_model(d, args.checkpoint, (h0_size, h1_size, h2_size, h3_size), LEARNING_RATE, precision)  # noqa: A001
    n_items = eng.I_global
    tr, te, uid0 = dp.load_tr_te_data(os.path.join(d, "%s_tr.csv" % args.split), os.path.join(d, "%s_te.csv" % args.split), n_items)
    _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(d, "item2id.txt"), os.path.join(d, "item_list.txt"),
                                               os.path.join(d, "niche_items.txt"), n_items)
    q = query_items(args.items, niche, n_items)
    aud = Audience(q, k=args.k, score=args.score)
    if world > 1:
        rec = ShardedRecommender(eng, EvalData(tr, te, eng.device, item_lo=lo, item_hi=hi), k=0, chunk=batch_size_test, audience=aud)
    else:
        rec = Recommender(eng, EvalData(tr, te, eng.device), k=0, chunk=batch_size_test, audience=aud)
    rec.run(rng_step=RNG_STEP, keep_prob=args.keep_prob)
    rows, scores = aud.table()
    m = audience_summary(rows, tr.shape[0])
    if rank == 0:
        write_audience(q, rows, scores, uid0, args.out, args.npz)
    print(summary_line(m, args.k))
    close_model(world)
    return q, rows, scores, m


if __name__ == "__main__":
    a = parse_args(sys.argv[1:])
    from ltgan.train import read_config
    audience(a, **read_config())
