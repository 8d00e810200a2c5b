"""Worker of tests/test_gpu_quota.py::test_sharded_recommender_with_rule: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every
rank on cuda:0).  ShardedRecommender with rule= (sharded forward; per slab ltg_topk and one ltg_topk_groups per reserved group; list
all-gathers; ltg_topk_merge; ltg_topk_quota on every rank) against, bit for bit, ltg_topk + ltg_topk_groups + ltg_topk_quota on the
all-gathered slab logits of the same forward -- one chunk, so that the forward's logits of every row are still in the activations -- and
against the numpy greedy walk over those logits; the lists are identical on every rank; several chunks with a short last one keep the
rule; a rule with all-zero slots is the plain sharded list; the report bound with the rule reads the ruled lists."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import quota_ref as Q
    import serving_harness as H
    from ltgan.dataset import EvalData
    from ltgan.sharded import ShardedRecommender
    from ltgan.synthetic import synthetic_index
    from ltgan.trainer import LongTailReport, MinSlots
    workload, users = sys.argv[1], int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    idx, _ = synthetic_index(workload, users=users, seed=5)
    I = idx.n_items
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    bias = torch.from_numpy(np.random.default_rng(3).uniform(1.0, 3.0, I).astype(np.float32)).to(dev)    # (see dist_topk_worker.py)
    eng.g_p[7].copy_(bias[lo:hi])
    n_ev = min(idx.N, users)
    fold = idx.train[:n_ev]
    labels = np.random.default_rng(12).integers(0, 4, I).astype(np.uint8)      # groups 0..2, label 3 in no group
    slots, k = [0, 30, 45], 100
    ev_full = EvalData(fold, fold, dev)
    ev_sh = EvalData(fold, fold, dev, item_lo=lo, item_hi=hi)
    step = 900
    # ---- exact: one chunk
    rule = MinSlots(labels, 3, slots)
    rep = LongTailReport(labels, 3)
    sh = ShardedRecommender(eng, ev_sh, k=k, chunk=n_ev, rule=rule, report=rep)
    ids, sc = sh.run(rng_step=step)
    full = H.gathered_logits(sh.acts.logits[:n_ev], lo, hi, I, world)
    tr_full, _ = ev_full.rows(0, n_ev)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    a_s, a_i = new(n_ev, k), new(n_ev, k, dt=torch.int32)
    ref.topk(full, tr_full, k, a_s, a_i)
    groups = [g for g, m in enumerate(slots) if m > 0]
    m = max(slots)
    g_s, g_i = new(len(groups), n_ev, m), new(len(groups), n_ev, m, dt=torch.int32)
    for j, g in enumerate(groups):
        ref.topk_groups(full, tr_full, m, rule.labels, 1 << g, g_s[j], g_i[j])
    w_s, w_i = new(n_ev, k), new(n_ev, k, dt=torch.int32)
    ref.topk_quota(a_s, a_i, g_s, g_i, [slots[g] for g in groups], w_s, w_i)
    torch.cuda.synchronize()
    assert np.array_equal(ids, w_i.cpu().numpy()), "sharded ruled ids differ from the gathered logits'"
    assert np.array_equal(sc.view(np.uint32), w_s.cpu().numpy().view(np.uint32)), "sharded ruled scores differ from the gathered logits'"
    folds = [fold.indices[fold.indptr[r]:fold.indptr[r + 1]] for r in range(n_ev)]
    n_s, n_i = Q.greedy_lists(full.cpu().numpy(), folds, labels, slots, k)
    assert np.array_equal(ids, n_i) and np.array_equal(sc.view(np.uint32), n_s.view(np.uint32)), "ruled lists differ from the greedy walk"
    for g in groups:
        n_g = int((labels == g).sum()) - np.asarray(fold[:, np.nonzero(labels == g)[0]].getnnz(axis=1)).ravel()
        assert n_g.min() >= slots[g] and ((labels[ids] == g).sum(1) >= slots[g]).all()
    assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))          # the report read the ruled lists
    H.same_on_every_rank(sh.ids, sh.scores, rep.item_hits)
    # ---- several chunks, the last one short: the rule holds for every user; all-zero slots == no rule
    ids_c, _ = ShardedRecommender(eng, ev_sh, k=k, chunk=100, rule=MinSlots(labels, 3, slots)).run(rng_step=step)
    for g in groups:
        assert ((labels[ids_c] == g).sum(1) >= slots[g]).all()
    assert all(len(set(r.tolist())) == k for r in ids_c)
    p_i, p_s = ShardedRecommender(eng, ev_sh, k=k, chunk=100).run(rng_step=step)
    z_i, z_s = ShardedRecommender(eng, ev_sh, k=k, chunk=100, rule=MinSlots(labels, 3, [0, 0, 0])).run(rng_step=step)
    assert np.array_equal(p_i, z_i) and np.array_equal(p_s.view(np.uint32), z_s.view(np.uint32))
    H.close_ranks("QUOTA_SHARDED_OK world=%d workload=%s slabs=%s" % (world, workload, H.slab_sizes(I, world)))


if __name__ == "__main__":
    main()
