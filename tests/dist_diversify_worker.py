"""Worker of tests/test_gpu_diversify.py::test_sharded_recommender_with_diversify: `torchrun --nproc-per-node N` on ONE GPU (gloo backend,
every rank on cuda:0).  ShardedRecommender with diversify= (sharded forward; per slab ltg_topk at `candidates`; list all-gathers;
ltg_topk_merge; the image of the whole catalogue from one all-reduce of the packed slabs; ltg_topk_diversify on every rank) against, bit
for bit: the image an unsharded engine packs; ltg_topk + ltg_topk_diversify on the all-gathered slab logits of the same forward (one
chunk); and the unsharded Recommender on the whole catalogue, ids, scores and stats, over several chunks with a short last one.

The two forwards agree bit for bit by the model of serving_harness.exact_sum_model, so what is left is the claim under test."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import serving_harness as H
    from ltgan.sharded import ShardedRecommender
    from ltgan.trainer import Diversify, LongTailReport, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    k, c, lam, step = 100, 200, 0.3, 900
    bits = H.bits
    # ---- one chunk: the image, and the lists against the entry points called by hand on the gathered logits
    div = Diversify(lam, candidates=c)
    rep = LongTailReport(labels, 2)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=n_ev, diversify=div, report=rep)
    ids, sc = sh.run(rng_step=step, keep_prob=1.0)
    image = ref.item_pack("decoder", "cosine")
    assert torch.equal(div.image, image), "the all-reduced image differs from the unsharded engine's"
    full = H.gathered_logits(sh.acts.logits[:n_ev], lo, hi, I, world)
    tr_full, _ = ev_full.rows(0, n_ev)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    c_s, c_i, w_s, w_i, w_st = new(n_ev, c), new(n_ev, c, dt=torch.int32), new(n_ev, k), new(n_ev, k, dt=torch.int32), new(n_ev, 2)
    ref.topk(full, tr_full, c, c_s, c_i)
    ref.topk_diversify(image, 0, c_s, c_i, lam, k, w_s, w_i, w_st)
    torch.cuda.synchronize()
    assert np.array_equal(ids, w_i.cpu().numpy()), "sharded diversified ids differ from the gathered logits'"
    assert np.array_equal(bits(sc), bits(w_s.cpu().numpy())) and np.array_equal(bits(div.stats()), bits(w_st.cpu().numpy()))
    assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))          # the report read the diversified lists
    H.same_on_every_rank(sh.ids, sh.scores, div.stat, rep.item_hits)
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
    H.close_ranks("DIVERSIFY_SHARDED_OK world=%d items=%d slabs=%s" % (world, I, H.slab_sizes(I, world)))


if __name__ == "__main__":
    main()
