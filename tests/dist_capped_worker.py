"""Worker of tests/test_gpu_capped.py::test_sharded_recommender_with_cap: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every
rank on cuda:0).  ShardedRecommender with cap= (sharded forward; with score logprob the full-row lse combined from the slabs' partials;
per slab ltg_topk at the candidates' length; list all-gathers; ltg_topk_merge; then the same matching on every rank, nothing exchanged)
against the unsharded Recommender on the whole catalogue, bit for bit, for both scores, over several chunks with a short last one and
with a LongTailReport reading the capped lists.

The two forwards' logits agree bit for bit by the model of serving_harness.exact_sum_model.  The full-row lse of the sharded forward is
combined from per-slab partials and may differ from the unsharded one in its last bits; the worker prints how many rows do."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import serving_harness as H
    from ltgan.sharded import ExposureCap, ShardedRecommender
    from ltgan.trainer import LongTailReport, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    k, step = 100, 900
    bits = H.bits
    plain, _ = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step, keep_prob=1.0)
    C = int(np.bincount(plain.ravel(), minlength=I).max()) // 3                          # a cap that binds: a third of the head's exposure
    assert C >= 2
    line = []
    for score in ("logprob", "logit"):
        cap_s, cap_r = ExposureCap(C, score=score), ExposureCap(C, score=score)
        rep = LongTailReport(labels, 2)
        sh = ShardedRecommender(eng, ev_sh, k=k, chunk=100, cap=cap_s, report=rep)
        ids, sc = sh.run(rng_step=step, keep_prob=1.0)
        assert (sh.rowpart_all is not None) == (score == "logprob")                      # the logit needs no extra collective
        hits = np.bincount(ids[ids >= 0], minlength=I)
        assert hits.max() == C and np.array_equal(rep.table()[1], hits)                  # the report read the capped lists
        H.same_on_every_rank(sh.ids, sh.scores, cap_s.cand_i, cap_s.cand_s, cap_s.state, rep.item_hits,
                             *((cap_s.lse,) if score == "logprob" else ()))
        ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100, cap=cap_r).run(rng_step=step, keep_prob=1.0)
        assert torch.equal(cap_s.cand_i, cap_r.cand_i) and torch.equal(cap_s.cand_s.view(torch.int32), cap_r.cand_s.view(torch.int32))
        if score == "logprob":
            off = int((cap_s.lse.view(torch.int32) != cap_r.lse.view(torch.int32)).sum())
            print("rank %d: rows whose combined lse differs from the unsharded one in its bits: %d of %d" % (rank, off, n_ev), flush=True)
        same = (ids == ids_r).all(1)
        print("rank %d %s: rows with identical ids %.4f" % (rank, score, same.mean()), flush=True)
        assert same.all(), ("rows whose ids differ from the unsharded recommender's", score, np.nonzero(~same)[0][:10])
        assert np.array_equal(bits(sc), bits(sc_r)) and cap_s.stats() == cap_r.stats(), score
        assert not np.array_equal(ids, plain)
        line.append("%s %s" % (score, cap_s.stats()))
    H.close_ranks("CAPPED_SHARDED_OK world=%d items=%d slabs=%s %s" % (world, I, H.slab_sizes(I, world), "; ".join(line)))


if __name__ == "__main__":
    main()
