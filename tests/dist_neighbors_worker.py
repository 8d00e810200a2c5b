"""Worker of tests/test_gpu_neighbors.py::test_sharded_item_neighbors: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank
on cuda:0).  The item-sharded neighbour search (every rank packs its slab, the query rows are all-reduced as int32, per-slab
ltg_item_neighbors, one all-gather of the lists, ltg_topk_merge) against the unsharded ItemNeighbors with the same weights: bit-identical
ids AND scores -- a pair's score does not depend on the slab that holds the item -- on every rank, with and without a group mask, for all
items and for a query list, over several chunks (the last one short)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from ltgan.engine import Engine
    from ltgan.sharded import ShardedItemNeighbors, item_slab
    from ltgan.trainer import ItemNeighbors
    I = int(sys.argv[1])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    hs = (16, 24, 40, 32)
    ref = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev)
    lo, hi = item_slab(I, rank, world)
    eng = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev, item_lo=lo, item_hi=hi)
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
        t = torch.from_numpy(got_i).to(dev)                      # every rank holds the same table
        t0 = t.clone()
        dist.broadcast(t0, 0)
        assert torch.equal(t, t0)
        n += got_i.shape[0]
    dist.barrier()
    if rank == 0:
        print("NEIGHBORS_SHARDED_OK world=%d items=%d rows=%d slab=%d" % (world, I, n, hi - lo))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
