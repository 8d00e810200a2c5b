"""Worker of tests/test_gpu_explain.py::test_sharded_recommender_with_explain: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with explain= (sharded forward; the lists gathered and merged; the image of the whole
catalogue from one all-reduce of the packed slabs; per rank ltg_topk_explain over ITS slab's part of every history; the [n * top, r]
lists all-gathered and merged by ltg_topk_merge) against the unsharded Recommender on the whole catalogue, bit for bit: ids, scores and
the explanation table, over several chunks with a short last one, for plain and for diversified lists, identical on every rank.

The two forwards agree bit for bit by the construction of tests/dist_diversify_worker.py: W_q0 holds multiples of 1/64 in [-1, 1],
every user has 16 fold-in items and dropout is off, so the all-reduced encoder sum is exact."""
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
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.sharded import Explain, ShardedRecommender, item_slab
    from ltgan.trainer import Diversify, Recommender
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
    k, top, r, step = 100, 20, 3, 900
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    slabs = [item_slab(I, q, world) for q in range(world)]
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
        for a in (sh.ids, sh.scores, why_s.why_i, why_s.why_s):            # every rank holds the same tables
            a0 = a.clone()
            dist.broadcast(a0, 0)
            assert torch.equal(a, a0)
    dist.barrier()
    if rank == 0:
        print("EXPLAIN_SHARDED_OK world=%d items=%d slabs=%s" % (world, I, sorted({y - x for x, y in slabs})))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
