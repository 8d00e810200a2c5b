"""Worker of tests/test_gpu_diversify.py::test_sharded_recommender_with_diversify: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with diversify= (sharded forward; per slab ltg_topk at `candidates`; list all-gathers;
ltg_topk_merge; the image of the whole catalogue from one all-reduce of the packed slabs; ltg_topk_diversify on every rank) against, bit
for bit: the image an unsharded engine packs; ltg_topk + ltg_topk_diversify on the all-gathered slab logits of the same forward (one
chunk); and the unsharded Recommender on the whole catalogue, ids, scores and stats, over several chunks with a short last one.

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
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.sharded import ShardedRecommender, item_slab
    from ltgan.trainer import Diversify, LongTailReport, Recommender
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
    labels = rng.integers(0, 3, I).astype(np.uint8)
    k, c, lam, step = 100, 200, 0.3, 900
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    # ---- one chunk: the image, and the lists against the entry points called by hand on the gathered logits
    div = Diversify(lam, candidates=c)
    rep = LongTailReport(labels, 2)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=n_ev, diversify=div, report=rep)
    ids, sc = sh.run(rng_step=step, keep_prob=1.0)
    image = ref.item_pack("decoder", "cosine")
    assert torch.equal(div.image, image), "the all-reduced image differs from the unsharded engine's"
    slabs = [item_slab(I, r, world) for r in range(world)]
    wmax = max(b - a for a, b in slabs)
    mine = torch.zeros(n_ev, wmax, dtype=torch.float32, device=dev)
    mine[:, : hi - lo] = sh.acts.logits[:n_ev]
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine)
    full = torch.cat([p[:, : b - a] for p, (a, b) in zip(parts, slabs)], dim=1).contiguous()
    tr_full, _ = ev_full.rows(0, n_ev)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    c_s, c_i, w_s, w_i, w_st = new(n_ev, c), new(n_ev, c, dt=torch.int32), new(n_ev, k), new(n_ev, k, dt=torch.int32), new(n_ev, 2)
    ref.topk(full, tr_full, c, c_s, c_i)
    ref.topk_diversify(image, 0, c_s, c_i, lam, k, w_s, w_i, w_st)
    torch.cuda.synchronize()
    assert np.array_equal(ids, w_i.cpu().numpy()), "sharded diversified ids differ from the gathered logits'"
    assert np.array_equal(bits(sc), bits(w_s.cpu().numpy())) and np.array_equal(bits(div.stats()), bits(w_st.cpu().numpy()))
    assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))          # the report read the diversified lists
    for a in (sh.ids, sh.scores, div.stat, rep.item_hits):             # every rank holds the same tables
        a0 = a.clone()
        dist.broadcast(a0, 0)
        assert torch.equal(a, a0)
    # ---- several chunks, the last one short, against the unsharded Recommender on the whole catalogue: bit for bit
    div_c, div_r = Diversify(lam, candidates=c), Diversify(lam, candidates=c)
    ids_c, sc_c = ShardedRecommender(eng, ev_sh, k=k, chunk=100, diversify=div_c).run(rng_step=step, keep_prob=1.0)
    ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100, diversify=div_r).run(rng_step=step, keep_prob=1.0)
    same = (ids_c == ids_r).all(1)
    print("rank %d: rows with identical ids %.4f" % (rank, same.mean()))
    assert same.all(), ("rows whose ids differ from the unsharded recommender's", np.nonzero(~same)[0][:10])
    assert np.array_equal(bits(sc_c), bits(sc_r)) and np.array_equal(bits(div_c.stats()), bits(div_r.stats()))
    assert np.array_equal(ids_c, ids)                                  # (and the chunking changes nothing)
    plain, _ = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step, keep_prob=1.0)
    assert not np.array_equal(plain, ids_c) and np.array_equal(plain[:, 0], ids_c[:, 0])
    dist.barrier()
    if rank == 0:
        print("DIVERSIFY_SHARDED_OK world=%d items=%d slabs=%s" % (world, I, sorted({y - x for x, y in slabs})))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
