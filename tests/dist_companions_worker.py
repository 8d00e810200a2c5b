"""Worker of tests/test_gpu_companions.py::test_sharded_pair_companions: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank
on cuda:0).  The item-sharded companion search (the discriminator is replicated: every rank packs the whole query chunk itself; each rank
searches the candidates of its own item slab, one all-gather of the lists, ltg_topk_merge) against the unsharded PairCompanions with the
same weights: bit-identical ids AND scores -- a pair's score does not depend on the call that holds the candidate -- on every rank, for
popular and for niche queries, over several chunks (the last one short), with a slab that holds no candidate at all."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import serving_harness as H
    from ltgan.sharded import ShardedPairCompanions
    from ltgan.trainer import PairCompanions
    I = int(sys.argv[1])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 37), rank, world)
    # the same discriminator on both, at a trained model's range (x 2), a few embedding rows duplicated across the slabs (ties by id)
    rng = np.random.default_rng(3)
    emb = ref.d_emb.cpu().numpy().copy()
    emb[rng.integers(0, I, 60)] = emb[1]
    arrs = [p.cpu().numpy() * (1.0 if p.dim() == 1 and i != 6 else 2.0) for i, p in enumerate(ref.d_p)]
    for e in (ref, eng):
        e.set_discriminator(2.0 * emb, arrs)
    niche = np.sort(rng.choice(I, I // 3, replace=False)).astype(np.int32)
    popular = np.setdiff1d(np.arange(I), niche).astype(np.int32)
    n = 0
    for side, q, c, k in (("popular", popular[::3], niche, 20), ("niche", niche[:333], popular, 256), ("popular", popular[:50], niche[niche < I // 2 - 7], 50)):
        want_i, want_s = PairCompanions(ref, k=k, queries=side, chunk=4096).run(q, c)
        got_i, got_s = ShardedPairCompanions(eng, k=k, queries=side, chunk=500).run(q, c)
        assert np.array_equal(got_i, want_i), "sharded ids differ from the unsharded table (%s k=%d)" % (side, k)
        assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), "sharded scores differ (%s k=%d)" % (side, k)
        assert np.all(got_i[:, 0] >= 0)
        H.same_on_every_rank(torch.from_numpy(got_i).to(dev))
        n += got_i.shape[0]
    H.close_ranks("COMPANIONS_SHARDED_OK world=%d items=%d rows=%d slab=%d" % (world, I, n, hi - lo))


if __name__ == "__main__":
    main()
