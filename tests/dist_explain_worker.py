"""Worker of tests/test_gpu_explain.py::test_sharded_recommender_with_explain: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with explain= (sharded forward; the lists gathered and merged; the image of the whole
catalogue from one all-reduce of the packed slabs; per rank ltg_topk_explain over ITS slab's part of every history; the [n * top, r]
lists all-gathered and merged by ltg_topk_merge) against the unsharded Recommender on the whole catalogue, bit for bit: ids, scores and
the explanation table, over several chunks with a short last one, for plain and for diversified lists, identical on every rank.

The two forwards agree bit for bit by the model of serving_harness.exact_sum_model."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import serving_harness as H
    from ltgan.sharded import Explain, ShardedRecommender
    from ltgan.trainer import Diversify, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    k, top, r, step = 100, 20, 3, 900
    bits = H.bits
    slabs = H.slabs(I, world)
    for div in (False, True):
        mk = (lambda: Diversify(0.3, candidates=200)) if div else (lambda: None)
        why_s, why_r = Explain(r, top=top), Explain(r, top=top)
        sh = ShardedRecommender(eng, ev_sh, k=k, chunk=100, diversify=mk(), explain=why_s)
        ids_s, sc_s = sh.run(rng_step=step, keep_prob=1.0)
        ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100, diversify=mk(), explain=why_r).run(rng_step=step, keep_prob=1.0)
        assert torch.equal(why_s.image, why_r.image), "the all-reduced image differs from the unsharded engine's"
        assert np.array_equal(ids_s, ids_r) and np.array_equal(bits(sc_s), bits(sc_r)), "the lists differ from the unsharded recommender's"
        (i_s, s_s), (i_r, s_r) = why_s.table(), why_r.table()
        same = (i_s == i_r).all((1, 2))
        print("rank %d diversify %d: users with identical explanations %.4f" % (rank, div, same.mean()))
        assert same.all(), ("users whose explanations differ from the unsharded run's", np.nonzero(~same)[0][:10])
        assert np.array_equal(bits(s_s), bits(s_r))
        # the explanations span the slabs: some entry's reasons come from more than one of them
        owner = np.searchsorted(np.array([b for _, b in slabs]), np.where(i_s >= 0, i_s, 0), side="right")
        assert world == 1 or ((owner.max(2) != owner.min(2)) & (i_s >= 0).all(2)).any()
        assert (i_s >= 0).all()                                            # 16 history items, none of them in a list: r reasons each
        H.same_on_every_rank(sh.ids, sh.scores, why_s.why_i, why_s.why_s)
    H.close_ranks("EXPLAIN_SHARDED_OK world=%d items=%d slabs=%s" % (world, I, H.slab_sizes(I, world)))


if __name__ == "__main__":
    main()
