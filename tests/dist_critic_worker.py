"""Worker of tests/test_gpu_critic.py::test_sharded_critic_and_gate: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank on
cuda:0).  ShardedRecommender with critic= and with gate= (sharded forward; the lists and the gate's candidates gathered and merged; the
discriminator replicated, so every rank packs both side images itself; per rank ltg_pair_critic over ITS slab's part of every history;
the fixed-point sums and the anchor counts all-reduced as integers, the best anchors all-gathered and merged by ltg_topk_merge; then every
rank finishes and gates identically) against the unsharded Recommender on the whole catalogue, bit for bit: ids, scores, the critic's
tables and the gate's stats, over several chunks with a short last one, identical on every rank.

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
    from ltgan.serving import Critic, CriticGate, Recommender, ShardedRecommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 37), rank, world)
    assert eng.feature_len == ref.feature_len == I and torch.equal(eng.d_emb, ref.d_emb)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    niche = set(rng.choice(I, I // 2, replace=False).tolist())
    valid = set(range(I)) - set(rng.choice(I, 40, replace=False).tolist())
    k, top, step = 100, 60, 900
    bits = lambda a: H.bits(a) if a.dtype == np.float32 else a         # (the critic's tables hold integers too)
    slabs = H.slabs(I, world)

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
    H.same_on_every_rank(sh.ids, sh.scores, c_s.crit, c_s.anchor_i, c_s.anchor_s, c_s.n_anchor, sh2.ids, sh2.scores, g_s.stat, c2_s.crit,
                         c2_s.anchor_i)
    H.close_ranks("CRITIC_SHARDED_OK world=%d items=%d slabs=%s" % (world, I, H.slab_sizes(I, world)))


if __name__ == "__main__":
    main()
