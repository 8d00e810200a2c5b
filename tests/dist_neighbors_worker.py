"""Worker of tests/test_gpu_neighbors.py::test_sharded_item_neighbors: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank
on cuda:0).  The item-sharded neighbour search (every rank packs its slab, the query rows are all-reduced as int32, per-slab
ltg_item_neighbors, one all-gather of the lists, ltg_topk_merge) against the unsharded ItemNeighbors with the same weights: bit-identical
ids AND scores -- a pair's score does not depend on the slab that holds the item -- on every rank, with and without a group mask, for all
items and for a query list, over several chunks (the last one short)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import serving_harness as H
    from ltgan.sharded import ShardedItemNeighbors
    from ltgan.trainer import ItemNeighbors
    I = int(sys.argv[1])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    # the same tables on both: rows of a trained model's spread, a few exact duplicates across the slabs (ties by id)
    rng = np.random.default_rng(3)
    for p in (0, 3):
        W = rng.standard_normal((I, ref.H)).astype(np.float32) * rng.uniform(0.1, 3.0, (I, 1)).astype(np.float32)
        W[rng.integers(0, I, 50)] = W[1]
        Wd = torch.from_numpy(W).to(dev)
        ref.g_p[p].copy_(Wd)
        eng.g_p[p].copy_(Wd[lo:hi])
    labels = (np.arange(I) % 4).astype(np.uint8)
    qlist = rng.choice(I, 333, replace=False).astype(np.int32)
    n = 0
    for space, metric, k, lab, only, q in (("decoder", "cosine", 20, None, None, None), ("encoder", "cosine", 50, labels, [1, 3], None),
                                          ("decoder", "dot", 256, labels, [0], qlist)):
        kw = dict(k=k, space=space, metric=metric, labels=lab, n_groups=4 if lab is not None else None, only=only)
        want_i, want_s = ItemNeighbors(ref, chunk=4096, **kw).run(q)
        got_i, got_s = ShardedItemNeighbors(eng, chunk=1500, **kw).run(q)
        assert np.array_equal(got_i, want_i), "sharded ids differ from the unsharded table (%s %s k=%d)" % (space, metric, k)
        assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), "sharded scores differ (%s %s k=%d)" % (space, metric, k)
        H.same_on_every_rank(torch.from_numpy(got_i).to(dev))
        n += got_i.shape[0]
    H.close_ranks("NEIGHBORS_SHARDED_OK world=%d items=%d rows=%d slab=%d" % (world, I, n, hi - lo))


if __name__ == "__main__":
    main()
