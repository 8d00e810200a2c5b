"""Worker of tests/test_gpu_companions.py::test_sharded_pair_companions: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank
on cuda:0).  The item-sharded companion search (the discriminator is replicated: every rank packs the whole query chunk itself; each rank
searches the candidates of its own item slab, one all-gather of the lists, ltg_topk_merge) against the unsharded PairCompanions with the
same weights: bit-identical ids AND scores -- a pair's score does not depend on the call that holds the candidate -- on every rank, for
popular and for niche queries, over several chunks (the last one short), with a slab that holds no candidate at all."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from ltgan.engine import Engine
    from ltgan.sharded import ShardedPairCompanions, item_slab
    from ltgan.trainer import PairCompanions
    I = int(sys.argv[1])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    hs = (16, 24, 40, 37)
    ref = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev)
    lo, hi = item_slab(I, rank, world)
    eng = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=77, d_seed=3, device=dev, item_lo=lo, item_hi=hi)
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
        t = torch.from_numpy(got_i).to(dev)                      # every rank holds the same table
        t0 = t.clone()
        dist.broadcast(t0, 0)
        assert torch.equal(t, t0)
        n += got_i.shape[0]
    dist.barrier()
    if rank == 0:
        print("COMPANIONS_SHARDED_OK world=%d items=%d rows=%d slab=%d" % (world, I, n, hi - lo))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
