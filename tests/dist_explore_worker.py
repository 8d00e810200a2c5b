"""Worker of tests/test_gpu_explore.py::test_sharded_recommender_with_explore: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with explore= (sharded forward; per slab the plain top-F and ltg_topk_sample; list all-gathers;
ltg_topk_merge on the keys; ltg_topk_sample_mass per slab and the three small all-reduces; ltg_topk_sample_finish on every rank) against
the unsharded Recommender on the whole catalogue: ids, scores and keys bit for bit, logp within the bound of DESIGN 5.21, in one chunk and
over several chunks with a short last one, with a LongTailReport reading the explored lists.

The two forwards agree bit for bit by the model of serving_harness.exact_sum_model, so what is left is the claim under test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOGP_TOL = 1e-4


def main():
    import serving_harness as H
    from ltgan.sharded import Explore, ShardedRecommender
    from ltgan.trainer import LongTailReport, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    k, T, F, draw, step = 100, 0.7, 5, 2, 900
    bits = H.bits
    worst = 0.0
    for chunk, fixed in ((n_ev, F), (100, F), (100, 0)):
        exp, rep = Explore(T, fixed=fixed, draw=draw), LongTailReport(labels, 3)
        sh = ShardedRecommender(eng, ev_sh, k=k, chunk=chunk, explore=exp, report=rep)
        ids, sc = sh.run(rng_step=step, keep_prob=1.0)
        H.same_on_every_rank(sh.ids, sh.scores, exp.keys, exp.logp, exp.explored, exp.sampled, rep.item_hits)
        assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))      # the report read the explored lists
        exp_1 = Explore(T, fixed=fixed, draw=draw)
        ids_1, sc_1 = Recommender(ref, ev_full, k=k, chunk=chunk, explore=exp_1).run(rng_step=step, keep_prob=1.0)
        same = (ids == ids_1).all(1)
        assert same.all(), ("rows whose ids differ from the unsharded recommender's", np.nonzero(~same)[0][:10])
        assert np.array_equal(bits(sc), bits(sc_1)) and np.array_equal(bits(exp.keys.cpu().numpy()), bits(exp_1.keys.cpu().numpy()))
        d = float(np.abs(exp.table().astype(np.float64) - exp_1.table().astype(np.float64)).max())
        worst = max(worst, d)
        assert d <= LOGP_TOL, d
        assert (exp.table()[:, :fixed] == 0).all() and (exp.table()[:, fixed:] < 0).all()
        st, st_1 = exp.stats(), exp_1.stats()
        assert st["explored_share"] == st_1["explored_share"] and st["sampled"] == n_ev * (k - fixed) and 0.0 < st["explored_share"] < 1.0
        if chunk == n_ev:
            first = ids
        elif fixed == F:
            assert np.array_equal(ids, first)                          # (and the chunking changes nothing)
    plain, _ = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step, keep_prob=1.0)
    assert np.array_equal(plain[:, :F], first[:, :F]) and not np.array_equal(plain, first)
    H.close_ranks("EXPLORE_SHARDED_OK world=%d items=%d slabs=%s largest logp difference %.3g explored share %.4f" % (
        world, I, H.slab_sizes(I, world), worst, st["explored_share"]))


if __name__ == "__main__":
    main()
