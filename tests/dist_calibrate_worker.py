"""Worker of tests/test_gpu_calibrate.py::test_sharded_recommender_with_calibrate: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with calibrate= (sharded forward; per slab one ltg_topk_groups list per class; list all-gathers;
ltg_topk_merge; ltg_hist_groups on the slab's part of the histories and one int32 all-reduce of the counts; ltg_topk_calibrate on every
rank) against, bit for bit: the class histogram of the whole histories; and the unsharded Recommender on the whole catalogue, ids, scores
and stats, in one chunk and over several chunks with a short last one, with a LongTailReport reading the calibrated lists.

The two forwards agree bit for bit by the model of serving_harness.exact_sum_model, so what is left is the claim under test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import calibrate_ref as R
    import serving_harness as H
    from ltgan.sharded import Calibrate, ShardedRecommender
    from ltgan.trainer import LongTailReport, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    labels = rng.integers(0, 4, I).astype(np.uint8)                    # n_groups = 3: label 3 is "in no group"
    k, lam, step = 100, 0.8, 900
    bits = H.bits
    # ---- one chunk: the all-reduced histogram is the histogram of the whole histories
    cal = Calibrate(labels, 3, lam)
    rep = LongTailReport(labels, 3)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=n_ev, calibrate=cal, report=rep)
    ids, sc = sh.run(rng_step=step, keep_prob=1.0)
    want_h = R.hist_groups(fold.indptr, fold.indices, 0, labels, 3)
    assert np.array_equal(cal.hist.view(n_ev, 4).cpu().numpy(), want_h) and (want_h.sum(1) == 16).all()
    assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))          # the report read the calibrated lists
    H.same_on_every_rank(sh.ids, sh.scores, cal.stat, cal.hist, rep.item_hits)
    cal_1 = Calibrate(labels, 3, lam)
    ids_1, sc_1 = Recommender(ref, ev_full, k=k, chunk=n_ev, calibrate=cal_1).run(rng_step=step, keep_prob=1.0)
    assert np.array_equal(ids, ids_1), "sharded calibrated ids differ from the unsharded recommender's"
    assert np.array_equal(bits(sc), bits(sc_1)) and np.array_equal(bits(cal.stats()), bits(cal_1.stats()))
    # ---- several chunks, the last one short, against the unsharded Recommender on the whole catalogue: bit for bit
    cal_c, cal_r = Calibrate(labels, 3, lam), Calibrate(labels, 3, lam)
    ids_c, sc_c = ShardedRecommender(eng, ev_sh, k=k, chunk=100, calibrate=cal_c).run(rng_step=step, keep_prob=1.0)
    ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100, calibrate=cal_r).run(rng_step=step, keep_prob=1.0)
    same = (ids_c == ids_r).all(1)
    print("rank %d: rows with identical ids %.4f" % (rank, same.mean()))
    assert same.all(), ("rows whose ids differ from the unsharded recommender's", np.nonzero(~same)[0][:10])
    assert np.array_equal(bits(sc_c), bits(sc_r)) and np.array_equal(bits(cal_c.stats()), bits(cal_r.stats()))
    assert np.array_equal(ids_c, ids)                                  # (and the chunking changes nothing)
    plain, _ = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step, keep_prob=1.0)
    assert not np.array_equal(plain, ids_c)
    st = cal_c.stats()
    assert st[:, 1].mean() < st[:, 0].mean()
    H.close_ranks("CALIBRATE_SHARDED_OK world=%d items=%d slabs=%s miscal %.4f -> %.4f" % (world, I, H.slab_sizes(I, world),
                                                                                             st[:, 0].mean(), st[:, 1].mean()))


if __name__ == "__main__":
    main()
