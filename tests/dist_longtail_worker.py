"""Worker of tests/test_gpu_longtail.py::test_sharded_report: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank on
cuda:0).  The item-sharded long-tail report (ShardedRecommender with report=: sharded forward, per-slab ltg_topk, the two all-gathers,
ltg_topk_merge, ltg_topk_metrics; no exchange of its own) against
  - exactly: ltg_topk_metrics on ltg_topk over the all-gathered slab logits of the same sharded forward, and rank 0's tables;
  - loosely: the unsharded report with the same weights and counter (the encoder all-reduce sums in another order, so near-ties swap):
    every reported mean within the 3e-3 tests/test_gpu_cli.py allows between test.py sharded and unsharded, users / items exact.
The differences seen are printed (SEEN ...).  On one MI355X, custom:1001 with 230 users, 2 ranks (slabs 512 / 489) and 3 ranks (slabs
384 / 384 / 233): every mean, share, coverage and the Gini coefficient came out identical (difference 0).  A record, not a bound."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import scipy.sparse as sp
    import serving_harness as H
    from ltgan import longtail as lt
    from ltgan.dataset import EvalData
    from ltgan.sharded import ShardedRecommender
    from ltgan.synthetic import synthetic_index
    from ltgan.trainer import LongTailReport, Recommender
    workload, users = sys.argv[1], int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    idx, _ = synthetic_index(workload, users=users, seed=5)
    I = idx.n_items
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    # item biases of a trained model's size (see dist_topk_worker.py): near-ties then are ties of logits of order one
    bias = torch.from_numpy(np.random.default_rng(3).uniform(1.0, 3.0, I).astype(np.float32)).to(dev)
    ref.g_p[7].copy_(bias)
    eng.g_p[7].copy_(bias[lo:hi])
    n_ev = min(idx.N, users)
    fold = idx.train[:n_ev]
    # held-out rows: the six most biased items the user has not folded in (so the lists hold some), and six random ones
    rs = np.random.default_rng(11)
    order = np.argsort(-bias.cpu().numpy(), kind="stable")
    r_, c_ = [], []
    for u in range(n_ev):
        seen = set(fold.indices[fold.indptr[u]:fold.indptr[u + 1]].tolist())
        top = [int(i) for i in order[:40] if int(i) not in seen][:6]
        rnd = [int(i) for i in rs.integers(0, I, 6) if int(i) not in seen]
        if u % 17 == 5:
            top, rnd = [], []                                          # users without held-out items
        for i in sorted(set(top + rnd)):
            r_.append(u)
            c_.append(i)
    te = sp.csr_matrix((np.ones(len(r_), np.float32), (r_, c_)), shape=(n_ev, I))
    labels, names = lt.pop_groups_from_counts(np.asarray(fold.sum(axis=0)).ravel().astype(np.int64), 3)
    ev_full = EvalData(fold, te, dev)
    ev_sh = EvalData(fold, te, dev, item_lo=lo, item_hi=hi)
    k_exp, step = 60, 900
    # ---- exact: one chunk, so that the sharded forward's slab logits of every row are still in the activations
    rep = LongTailReport(labels, 3, k_exp=k_exp)
    sh = ShardedRecommender(eng, ev_sh, k=rep.k, chunk=n_ev, report=rep)
    ids, _ = sh.run(rng_step=step)
    out, hits = rep.table()
    full = H.gathered_logits(sh.acts.logits[:n_ev], lo, hi, I, world)
    want_s = torch.empty(n_ev, rep.k, dtype=torch.float32, device=dev)
    want_i = torch.empty(n_ev, rep.k, dtype=torch.int32, device=dev)
    tr_full, te_full = ev_full.rows(0, n_ev)
    ref.topk(full, tr_full, rep.k, want_s, want_i)
    want_out = torch.zeros(n_ev, 4, 4, dtype=torch.float32, device=dev)
    want_hits = torch.zeros(I, dtype=torch.int32, device=dev)
    ref.topk_metrics(want_i, te_full, rep.labels, 3, want_out, want_hits, k_exp=k_exp)
    torch.cuda.synchronize()
    assert np.array_equal(out.view(np.uint32), want_out.cpu().numpy().view(np.uint32)), "sharded report differs from the gathered logits'"
    assert np.array_equal(hits, want_hits.cpu().numpy())
    assert hits.sum() == n_ev * k_exp                                  # NOT all-reduced: every rank counted every user once
    H.same_on_every_rank(rep.out, rep.item_hits)
    # ---- several chunks (the last one short), against the unsharded report
    rep_c = LongTailReport(labels, 3, k_exp=k_exp)
    ShardedRecommender(eng, ev_sh, k=rep_c.k, chunk=100, report=rep_c).run(rng_step=step)
    rep_r = LongTailReport(labels, 3, k_exp=k_exp)
    Recommender(ref, ev_full, k=rep_r.k, chunk=100, report=rep_r).run(rng_step=step)
    out_c, hits_c = rep_c.table()                                      # (another forward than the one chunk's: the counter is rng_step + lo)
    assert hits_c.sum() == n_ev * k_exp
    a = lt.aggregate(out_c, hits_c, labels, names, k_exp)
    b = lt.aggregate(*rep_r.table(), labels, names, k_exp)
    seen = {}
    for ra, rb in zip(a["groups"] + [a["all"]], b["groups"] + [b["all"]]):
        assert (ra["name"], ra["items"], ra["users"]) == (rb["name"], rb["items"], rb["users"]) and ra["users"] > 0, (ra, rb)
        for key in ("ndcg", "recall20", "recall50", "share", "coverage"):
            seen[key] = max(seen.get(key, 0.0), abs(ra[key] - rb[key]))
            assert abs(ra[key] - rb[key]) < 3e-3, (ra["name"], key, ra[key], rb[key])
    assert abs(a["all"]["gini"] - b["all"]["gini"]) < 3e-3
    assert a["all"]["ndcg"] > 0.0
    H.close_ranks("SEEN max |sharded - unsharded| over the rows: %s gini %.3g\nLONGTAIL_SHARDED_OK world=%d workload=%s users=%s slabs=%s" % (
        " ".join("%s %.3g" % kv for kv in seen.items()), abs(a["all"]["gini"] - b["all"]["gini"]), world, workload,
        [g["users"] for g in a["groups"]], H.slab_sizes(I, world)))


if __name__ == "__main__":
    main()
