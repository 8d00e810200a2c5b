"""Worker of tests/test_gpu_topk.py::test_sharded_recommender: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank on
cuda:0).  The item-sharded recommender (sharded forward, per-slab ltg_topk, one all-gather, ltg_topk_merge) against
  - exactly: ltg_topk over the all-gathered slab logits of the same sharded forward (the exchange and the merge lose nothing);
  - loosely: the unsharded Recommender with the same weights and counter (the encoder all-reduce sums in another order, so the logits
    are not bit-identical: >= 97 % of rows identical, elsewhere only near-ties swapped)."""
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
    from ltgan.dataset import EvalData
    from ltgan.sharded import ShardedRecommender
    from ltgan.synthetic import synthetic_index
    from ltgan.trainer import Recommender
    workload, users = sys.argv[1], int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    idx, _ = synthetic_index(workload, users=users, seed=5)
    I = idx.n_items
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    # item biases of a trained model's size: the logits of a fresh initialisation are ~1e-2, where the 1e-7 the encoder all-reduce's
    # order moves a logit by would be a relative 1e-5 -- the near-tie bound below is stated for logits of order one
    bias = torch.from_numpy(np.random.default_rng(3).uniform(1.0, 3.0, I).astype(np.float32)).to(dev)
    ref.g_p[7].copy_(bias)
    eng.g_p[7].copy_(bias[lo:hi])
    n_ev = min(idx.N, users)
    fold = idx.train[:n_ev]
    rs = np.random.default_rng(11)
    te_rows = np.repeat(np.arange(n_ev), 6)
    te = sp.csr_matrix((np.ones(len(te_rows), np.float32), (te_rows, rs.integers(0, I, len(te_rows)))), shape=(n_ev, I))
    ev_full = EvalData(fold, te, dev)
    ev_sh = EvalData(fold, te, dev, item_lo=lo, item_hi=hi)
    k = 100
    step = 900
    # ---- exact: one chunk, so that the sharded forward's slab logits of every row are still in the activations
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=n_ev)
    ids, sc = sh.run(rng_step=step)
    full = H.gathered_logits(sh.acts.logits[:n_ev], lo, hi, I, world)
    want_s = torch.empty(n_ev, k, dtype=torch.float32, device=dev)
    want_i = torch.empty(n_ev, k, dtype=torch.int32, device=dev)
    tr_full, _ = ev_full.rows(0, n_ev)
    ref.topk(full, tr_full, k, want_s, want_i)
    torch.cuda.synchronize()
    assert np.array_equal(ids, want_i.cpu().numpy()), "sharded table differs from ltg_topk on the gathered logits"
    assert np.array_equal(sc.view(np.uint32), want_s.cpu().numpy().view(np.uint32))
    H.same_on_every_rank(torch.from_numpy(ids).to(dev))
    # ---- several chunks (the last one short), against the unsharded recommender
    ids_c, sc_c = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step)
    ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100).run(rng_step=step)
    same = (ids_c == ids_r).all(1)
    assert same.mean() >= 0.97, ("rows with identical ids", same.mean())
    for r in np.nonzero(~same)[0]:
        d = ids_c[r] != ids_r[r]
        a, b = sc_c[r, d].astype(np.float64), sc_r[r, d].astype(np.float64)
        assert np.all(np.abs(a - b) <= 1e-5 * np.maximum(np.abs(a), np.abs(b))), ("not a near-tie", r, a, b)
    H.close_ranks("TOPK_SHARDED_OK world=%d workload=%s rows_identical=%.4f slabs=%s" % (world, workload, same.mean(), H.slab_sizes(I, world)))


if __name__ == "__main__":
    main()
