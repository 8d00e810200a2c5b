"""Worker of tests/test_gpu_share.py::test_sharded_recommender_with_share: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every
rank on cuda:0).  ShardedRecommender with share= (sharded forward; per slab two ltg_topk_groups lists, the promoted groups' and the
complement's; list all-gathers; ltg_topk_merge; then the same ltg_topk_share on every rank, nothing exchanged) against the unsharded
Recommender on the whole catalogue, bit for bit, over several chunks with a short last one and with a LongTailReport reading the final
lists.

The two forwards' logits agree bit for bit by the model of serving_harness.exact_sum_model."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import serving_harness as H
    from ltgan.sharded import ShardedRecommender, ShareTarget
    from ltgan.trainer import LongTailReport, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    labels = rng.integers(0, 3, I).astype(np.uint8)      # two groups; label 2 is in no group and belongs to the rest lists
    k, step = 100, 900
    bits = H.bits
    plain, plain_sc = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step, keep_prob=1.0)
    zero = ShareTarget(labels, 2, [1], 0.0)              # share = 0: the plain table, and the sizes of the problem
    ids0, sc0 = ShardedRecommender(eng, ev_sh, k=k, chunk=100, share=zero).run(rng_step=step, keep_prob=1.0)
    assert np.array_equal(ids0, plain) and np.array_equal(bits(sc0), bits(plain_sc))
    z = zero.stats()
    assert z["taken"] == 0 and z["available"] > 100
    share = z["plain_share"] + (z["available"] // 3) / (n_ev * k)        # a third of the way to the limit: the threshold binds
    tgt_s, tgt_r = ShareTarget(labels, 2, [1], share), ShareTarget(labels, 2, [1], share)
    rep = LongTailReport(labels, 2)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=100, share=tgt_s, report=rep)
    ids, sc = sh.run(rng_step=step, keep_prob=1.0)
    assert sh.rowpart_all is None                        # no lse, no extra collective
    assert np.array_equal(rep.table()[1], np.bincount(ids[ids >= 0], minlength=I))       # the report read the final lists
    H.same_on_every_rank(sh.ids, sh.scores, tgt_s.pro_i, tgt_s.pro_s, tgt_s.rest_i, tgt_s.rest_s, tgt_s.state, rep.item_hits)
    ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100, share=tgt_r).run(rng_step=step, keep_prob=1.0)
    for a, b in ((tgt_s.pro_i, tgt_r.pro_i), (tgt_s.rest_i, tgt_r.rest_i), (tgt_s.pro_s.view(torch.int32), tgt_r.pro_s.view(torch.int32)),
                 (tgt_s.rest_s.view(torch.int32), tgt_r.rest_s.view(torch.int32))):
        assert torch.equal(a, b)
    same = (ids == ids_r).all(1)
    print("rank %d: rows with identical ids %.4f" % (rank, same.mean()), flush=True)
    assert same.all(), ("rows whose ids differ from the unsharded recommender's", np.nonzero(~same)[0][:10])
    assert np.array_equal(bits(sc), bits(sc_r)) and tgt_s.stats() == tgt_r.stats()
    st = tgt_s.stats()
    assert 0 < st["taken"] < st["available"] and st["reached"] and st["rows_changed"] > 0 and not np.array_equal(ids, plain)
    assert int(np.isin(ids, np.nonzero(labels == 1)[0]).sum()) == tgt_s.want
    H.close_ranks("SHARE_SHARDED_OK world=%d items=%d slabs=%s %s" % (world, I, H.slab_sizes(I, world), st))


if __name__ == "__main__":
    main()
