"""Worker of tests/test_gpu_posterior.py::test_sharded_recommender_with_posterior: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with posterior= (sharded forward; every rank builds the same image from the replicated
mu | logvar and scores its own slab; per-slab lists gathered and merged; one float all-reduce of the entry tables; with a rule that reads
the lse, one all-gather of the per-slab lse) against the unsharded Recommender on the whole catalogue: ids, scores and the entry tables
bit for bit, the lse within 1e-5, in one chunk and over several chunks with a short last one.

The two forwards agree bit for bit by the model of serving_harness.exact_sum_model, so what is left is the claim under test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LSE_TOL = 1e-5


def main():
    import serving_harness as H
    from ltgan.sharded import ExposureCap, Posterior, ShardedRecommender
    from ltgan.trainer import LongTailReport, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    k, step = 100, 900
    bits = H.bits
    worst = 0.0
    for chunk, kw in ((n_ev, dict(samples=16, beta=1.0, draw=2)), (100, dict(samples=16, beta=1.0, draw=2)), (100, dict(samples=4, beta=-1.0)),
                      (100, dict(samples=1, beta=0.0, draw=5))):
        post, rep = Posterior(stats=True, **kw), LongTailReport(labels, 3)
        sh = ShardedRecommender(eng, ev_sh, k=k, chunk=chunk, posterior=post, report=rep)
        ids, sc = sh.run(rng_step=step, keep_prob=1.0)
        H.same_on_every_rank(sh.ids, sh.scores, post.mean, post.std, post.outside, rep.item_hits)
        assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))      # the report read the posterior's lists
        post_1 = Posterior(stats=True, **kw)
        ids_1, sc_1 = Recommender(ref, ev_full, k=k, chunk=chunk, posterior=post_1).run(rng_step=step, keep_prob=1.0)
        same = (ids == ids_1).all(1)
        assert same.all(), ("rows whose ids differ from the unsharded recommender's", np.nonzero(~same)[0][:10])
        assert np.array_equal(bits(sc), bits(sc_1))
        (m, d), (m_1, d_1) = post.table(), post_1.table()
        assert np.array_equal(m, m_1) and np.array_equal(d, d_1)                          # (by value: a slab that does not own an entry adds 0.0)
        assert post.stats() == post_1.stats()
        if chunk == n_ev:
            first = ids
        elif kw == dict(samples=16, beta=1.0, draw=2):
            assert np.array_equal(ids, first)                                             # (and the chunking changes nothing)
    # a rule that reads the lse: the full-row lse of the scores, combined from the slabs' lse
    cap, cap_1 = ExposureCap(40), ExposureCap(40)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=100, posterior=Posterior(samples=8), cap=cap)
    ids, sc = sh.run(rng_step=step, keep_prob=1.0)
    one = Recommender(ref, ev_full, k=k, chunk=100, posterior=Posterior(samples=8), cap=cap_1)
    ids_1, sc_1 = one.run(rng_step=step, keep_prob=1.0)
    n_last = n_ev - (n_ev - 1) // 100 * 100
    worst = float((sh.acts.lse[:n_last] - one.acts.lse[:n_last]).abs().max())
    assert worst <= LSE_TOL, worst
    assert np.bincount(ids[ids >= 0].ravel(), minlength=I).max() <= 40
    plain, _ = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step, keep_prob=1.0)
    assert not np.array_equal(plain, first)
    H.close_ranks("POSTERIOR_SHARDED_OK world=%d items=%d slabs=%s largest lse difference %.3g" % (world, I, H.slab_sizes(I, world), worst))


if __name__ == "__main__":
    main()
