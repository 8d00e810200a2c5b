"""Worker of tests/test_gpu_critic.py::test_sharded_critic_and_gate: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank on
cuda:0).  ShardedRecommender with critic= and with gate= (sharded forward; the lists and the gate's candidates gathered and merged; the
discriminator replicated, so every rank packs both side images itself; per rank ltg_pair_critic over ITS slab's part of every history;
the fixed-point sums and the anchor counts all-reduced as integers, the best anchors all-gathered and merged by ltg_topk_merge; then every
rank finishes and gates identically) against the unsharded Recommender on the whole catalogue, bit for bit: ids, scores, the critic's
tables and the gate's stats, over several chunks with a short last one, identical on every rank.

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
    from ltgan.serving import Critic, CriticGate, Recommender, ShardedRecommender
    from ltgan.sharded import item_slab
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    hs = (16, 24, 40, 37)
    ref = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev)
    lo, hi = item_slab(I, rank, world)
    eng = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev, item_lo=lo, item_hi=hi)
    assert eng.feature_len == ref.feature_len == I and torch.equal(eng.d_emb, ref.d_emb)
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
    niche = set(rng.choice(I, I // 2, replace=False).tolist())
    valid = set(range(I)) - set(rng.choice(I, 40, replace=False).tolist())
    k, top, step = 100, 60, 900
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a
    slabs = [item_slab(I, q, world) for q in range(world)]

    def same_tables(a, b, what):
        for key in ("crit", "anchor_i", "anchor_s", "n_anchor"):
            assert np.array_equal(bits(a[key]), bits(b[key])), "%s: %s differs from the unsharded run's" % (what, key)

    # 1. the critic of the plain lists
    c_s, c_r = Critic(niche, valid, top=top), Critic(niche, valid, top=top)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=100, critic=c_s)
    ids_s, sc_s = sh.run(rng_step=step, keep_prob=1.0)
    ids_r, sc_r = Recommender(ref, ev_full, k=k, chunk=100, critic=c_r).run(rng_step=step, keep_prob=1.0)
    assert np.array_equal(ids_s, ids_r) and np.array_equal(bits(sc_s), bits(sc_r)), "the lists differ from the unsharded recommender's"
    t_s, t_r = c_s.table(), c_r.table()
    same_tables(t_s, t_r, "critic")
    assert c_s.summary() == c_r.summary() and c_s.summary()["scored"] > n_ev
    owner = lambda g: np.searchsorted(np.array([b for _, b in slabs]), g, side="right")
    anchors_span = [len({int(owner(x)) for x in fold.indices[fold.indptr[u]:fold.indptr[u + 1]] if x not in niche and x in valid}) for u in range(n_ev)]
    assert world == 1 or max(anchors_span) > 1, "no user's anchors span two slabs"
    assert len(set(owner(t_s["anchor_i"][t_s["anchor_i"] >= 0]).tolist())) == world, "the best anchors come from every slab"

    # 2. the gate, with the critic reading the gated lists
    p = float(1.0 / (1.0 + np.exp(-np.median(t_r["crit"][t_r["anchor_i"] >= 0].astype(np.float64)))))
    g_s, g_r, c2_s, c2_r = CriticGate(niche, valid, p, candidates=180), CriticGate(niche, valid, p, candidates=180), Critic(niche, valid), Critic(niche, valid)
    sh2 = ShardedRecommender(eng, ev_sh, k=k, chunk=100, gate=g_s, critic=c2_s)
    ids_s, sc_s = sh2.run(rng_step=step, keep_prob=1.0)
    ids_r2, sc_r2 = Recommender(ref, ev_full, k=k, chunk=100, gate=g_r, critic=c2_r).run(rng_step=step, keep_prob=1.0)
    assert np.array_equal(ids_s, ids_r2) and np.array_equal(bits(sc_s), bits(sc_r2)), "the gated lists differ from the unsharded recommender's"
    assert np.array_equal(g_s.stats(), g_r.stats()) and g_r.stats()[:, 1].sum() > n_ev and not np.array_equal(ids_r2, ids_r)
    same_tables(c2_s.table(), c2_r.table(), "critic of the gated lists")
    print("rank %d: %d scored entries, %d rejected by the gate" % (rank, c_s.summary()["scored"], int(g_s.stats()[:, 1].sum())))
    for a in (sh.ids, sh.scores, c_s.crit, c_s.anchor_i, c_s.anchor_s, c_s.n_anchor, sh2.ids, sh2.scores, g_s.stat, c2_s.crit, c2_s.anchor_i):
        a0 = a.clone()                                                 # every rank holds the same tables
        dist.broadcast(a0, 0)
        assert torch.equal(a, a0)
    dist.barrier()
    if rank == 0:
        print("CRITIC_SHARDED_OK world=%d items=%d slabs=%s" % (world, I, sorted({y - x for x, y in slabs})))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
