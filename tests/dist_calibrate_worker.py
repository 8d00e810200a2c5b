"""Worker of tests/test_gpu_calibrate.py::test_sharded_recommender_with_calibrate: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with calibrate= (sharded forward; per slab one ltg_topk_groups list per class; list all-gathers;
ltg_topk_merge; ltg_hist_groups on the slab's part of the histories and one int32 all-reduce of the counts; ltg_topk_calibrate on every
rank) against, bit for bit: the class histogram of the whole histories; and the unsharded Recommender on the whole catalogue, ids, scores
and stats, in one chunk and over several chunks with a short last one, with a LongTailReport reading the calibrated lists.

The sharded forward all-reduces the encoder's partial pre-activations, which in general sums in another order than the unsharded forward
(tests/dist_topk_worker.py).  Here that sum is exact, so the two forwards agree bit for bit and what is left is the claim under test:
W_q0 holds multiples of 1/64 in [-1, 1], every user has 16 fold-in items and dropout is off, so every partial sum is a multiple of 1/64
below 16 and the row scale is 1/4."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import scipy.sparse as sp
    import calibrate_ref as R
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.sharded import Calibrate, ShardedRecommender, item_slab
    from ltgan.trainer import LongTailReport, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    hs = (16, 24, 40, 32)
    ref = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev)
    lo, hi = item_slab(I, rank, world)
    eng = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev, item_lo=lo, item_hi=hi)
    rng = np.random.default_rng(3)
    bias = torch.from_numpy(rng.uniform(1.0, 3.0, I).astype(np.float32)).to(dev)          # (see dist_topk_worker.py)
    wq0 = torch.from_numpy((rng.integers(-64, 65, (I, ref.H)) / 64.0).astype(np.float32)).to(dev)
    ref.g_p[7].copy_(bias)
    eng.g_p[7].copy_(bias[lo:hi])
    ref.g_p[0].copy_(wq0)
    eng.g_p[0].copy_(wq0[lo:hi])
    cols = np.concatenate([rng.choice(I, 16, replace=False) for _ in range(n_ev)])
    fold = sp.csr_matrix((np.ones(16 * n_ev, np.float32), (np.repeat(np.arange(n_ev), 16), cols)), shape=(n_ev, I))
    fold.sort_indices()
    ev_full = EvalData(fold, fold, dev)
    ev_sh = EvalData(fold, fold, dev, item_lo=lo, item_hi=hi)
    labels = rng.integers(0, 4, I).astype(np.uint8)                    # n_groups = 3: label 3 is "in no group"
    k, lam, step = 100, 0.8, 900
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    # ---- one chunk: the all-reduced histogram is the histogram of the whole histories
    cal = Calibrate(labels, 3, lam)
    rep = LongTailReport(labels, 3)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=n_ev, calibrate=cal, report=rep)
    ids, sc = sh.run(rng_step=step, keep_prob=1.0)
    want_h = R.hist_groups(fold.indptr, fold.indices, 0, labels, 3)
    assert np.array_equal(cal.hist.view(n_ev, 4).cpu().numpy(), want_h) and (want_h.sum(1) == 16).all()
    assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))          # the report read the calibrated lists
    for a in (sh.ids, sh.scores, cal.stat, cal.hist, rep.item_hits):   # every rank holds the same tables
        a0 = a.clone()
        dist.broadcast(a0, 0)
        assert torch.equal(a, a0)
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
    dist.barrier()
    if rank == 0:
        print("CALIBRATE_SHARDED_OK world=%d items=%d slabs=%s miscal %.4f -> %.4f" % (world, I, sorted({y - x for x, y in slabs(I, world)}),
                                                                                        st[:, 0].mean(), st[:, 1].mean()))
    dist.destroy_process_group()


def slabs(I, world):
    from ltgan.sharded import item_slab
    return [item_slab(I, r, world) for r in range(world)]


if __name__ == "__main__":
    main()
