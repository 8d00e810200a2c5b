"""Worker of tests/test_gpu_floor.py::test_sharded_recommender_with_floor: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every
rank on cuda:0).  ShardedRecommender with floor= (sharded forward; with score logprob the full-row lse combined from the slabs' partials;
per slab ltg_topk at the candidates' length; list all-gathers; ltg_topk_merge; then the same matching on every rank, nothing exchanged)
against the unsharded Recommender on the whole catalogue, bit for bit, for both scores, over several chunks with a short last one and
with a LongTailReport reading the final lists.

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
    from ltgan.sharded import ExposureFloor, ShardedRecommender
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
    hits0 = np.bincount(plain.ravel(), minlength=I)
    M, Rv = max(2, int(np.median(hits0))), 10
    need = np.where(hits0 <= np.median(hits0), M, 0).astype(np.int32)                    # a floor that binds: the lower half up to the median
    assert ((need > 0) & (hits0 < need)).any()
    line = []
    for score in ("logprob", "logit"):
        fl_s, fl_r = ExposureFloor(need, Rv, score=score), ExposureFloor(need, Rv, score=score)
        rep = LongTailReport(labels, 2)
        sh = ShardedRecommender(eng, ev_sh, k=k, chunk=100, floor=fl_s, report=rep)
        ids, sc = sh.run(rng_step=step, keep_prob=1.0)
        assert (sh.rowpart_all is not None) == (score == "logprob")                      # the logit needs no extra collective
        hits = np.bincount(ids[ids >= 0], minlength=I)
        assert (hits >= np.minimum(need, fl_s.held())).all() and np.array_equal(rep.table()[1], hits)      # the report read the final lists
        H.same_on_every_rank(sh.ids, sh.scores, fl_s.cand_i, fl_s.cand_s, fl_s.state, fl_s.held_d, rep.item_hits,
                             *((fl_s.lse,) if score == "logprob" else ()))
        ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100, floor=fl_r).run(rng_step=step, keep_prob=1.0)
        assert torch.equal(fl_s.cand_i, fl_r.cand_i) and torch.equal(fl_s.cand_s.view(torch.int32), fl_r.cand_s.view(torch.int32))
        if score == "logprob":
            off = int((fl_s.lse.view(torch.int32) != fl_r.lse.view(torch.int32)).sum())
            print("rank %d: rows whose combined lse differs from the unsharded one in its bits: %d of %d" % (rank, off, n_ev), flush=True)
        same = (ids == ids_r).all(1)
        print("rank %d %s: rows with identical ids %.4f" % (rank, score, same.mean()), flush=True)
        assert same.all(), ("rows whose ids differ from the unsharded recommender's", score, np.nonzero(~same)[0][:10])
        assert np.array_equal(bits(sc), bits(sc_r)) and fl_s.stats() == fl_r.stats() and np.array_equal(fl_s.held(), fl_r.held()), score
        assert not np.array_equal(ids, plain)
        line.append("%s %s" % (score, fl_s.stats()))
    H.close_ranks("FLOOR_SHARDED_OK world=%d items=%d slabs=%s %s" % (world, I, H.slab_sizes(I, world), "; ".join(line)))


if __name__ == "__main__":
    main()
