"""Worker of tests/test_gpu_audience.py::test_sharded_audience: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every rank on
cuda:0).  The item-sharded audience walk (sharded forward, the full-row lse combined from the slabs' partials, per-slab
ltg_item_audience on the columns the rank owns, the table all-reduced) against
  - exactly: the numpy reference on the all-gathered slab logits and the combined lse of the same sharded forward (one chunk);
  - the unsharded Recommender with the same weights and counter over several chunks: the encoder all-reduce sums in another order, so
    the scores are not bit-identical -- at EVERY position of every list the two scores agree within 1e-5 relative (the near-tie bound of
    dist_topk_worker.py, for logits of order one), and the ids agree wherever the unsharded list's neighbouring scores are more than
    2e-5 relative apart.

Both comparisons run with bf16 and with fp32 decoder operands.  The exact one is asserted in both.  The one against the unsharded walk
is asserted with fp32 operands only, and that follows from the number formats, not from the walk: the bound is the one derived for what the
all-reduce order does to a logit of order one (~1e-7).  A bf16 operand carries 8 significant bits, so where the all-reduce moves an
activation across a rounding boundary (h2 moves by 3.5e-08) the operand moves by 2^-9 of its value and the logit by up to
|h2| |w| 2^-9 -- a second source of difference, of the bound's own size at 1 001 items, where the decoder weights are ~0.04, and below it
at 20 000 (~0.01); it is a property of two bf16 forwards, and no selection can remove it.  The bf16 figures are printed, not asserted.
Measured on an MI355X, 230 users, k = 50, 603 queries, chunks of 100 -- largest relative score difference, sharded / unsharded:
  custom:1001  bf16  logit 1.338e-05 (world 2; 7 of 30 150 entries beyond 1e-5), 1.244e-05 (world 4; 5 entries); logprob 2.36e-06
  custom:1001  fp32  logit 1.19e-07, logprob 3.84e-07
and the two forwards' logits themselves, one chunk: bf16 7.1e-06 (custom:1001), 1.1e-06 (ml20m); fp32 1.2e-07 (both)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import scipy.sparse as sp
    import audience_ref as AR
    import serving_harness as H
    from ltgan.dataset import EvalData
    from ltgan.sharded import ShardedRecommender, item_slab
    from ltgan.synthetic import synthetic_index
    from ltgan.trainer import Audience, Recommender
    workload, users = sys.argv[1], int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    idx, _ = synthetic_index(workload, users=users, seed=5)
    I = idx.n_items
    hs = (16, 24, 40, 32)
    n_ev = min(idx.N, users)
    fold = idx.train[:n_ev].tocsr()
    fold.sort_indices()
    te = sp.csr_matrix((n_ev, I), dtype=np.float32)
    lo, hi = item_slab(I, rank, world)
    ev_full = EvalData(fold, te, dev)
    ev_sh = EvalData(fold, te, dev, item_lo=lo, item_hi=hi)
    folds = [fold.indices[fold.indptr[r]:fold.indptr[r + 1]] for r in range(n_ev)]
    k, step = 50, 900
    rs = np.random.default_rng(11)
    n_take = min(I, 600)
    items = np.concatenate([rs.permutation(I)[:n_take], [0, I - 1, I - 1]]).astype(np.int32)   # every slab, shuffled, one repeated
    for precision in ("bf16", "fp32"):
        ref, eng, _, _ = H.slab_engines(I, hs, rank, world, precision=precision)
        # item biases of a trained model's size (dist_topk_worker.py): the near-tie bound below is stated for logits of order one
        bias = torch.from_numpy(np.random.default_rng(3).uniform(1.0, 3.0, I).astype(np.float32)).to(dev)
        ref.g_p[7].copy_(bias)
        eng.g_p[7].copy_(bias[lo:hi])
        for score in ("logprob", "logit"):
            # ---- exact: one chunk, so that the sharded forward's slab logits and lse of every row are still in the activations
            aud = Audience(items, k=k, score=score)
            sh = ShardedRecommender(eng, ev_sh, k=0, chunk=n_ev, audience=aud)
            ids0, _ = sh.run(rng_step=step)
            assert ids0.shape == (n_ev, 0)
            ids, sc = aud.table()
            full = H.gathered_logits(sh.acts.logits[:n_ev], lo, hi, I, world).cpu().numpy()
            lse = sh.acts.lse[:n_ev].cpu().numpy() if score == "logprob" else None
            wS, wID = AR.audience_lists(full, lse, folds, items, k)
            assert np.array_equal(ids, wID), ("sharded table differs from the reference on the gathered logits", score)
            assert np.array_equal(sc.view(np.uint32), wS.view(np.uint32)), score
            H.same_on_every_rank(torch.from_numpy(np.concatenate([ids, sc.view(np.int32)], axis=1)).to(dev))
            # ---- several chunks (the last one short), against the unsharded walk
            # (the unsharded lists one entry longer: the last position of a list has a neighbour to be compared with, too)
            aud_c, aud_r = Audience(items, k=k, score=score), Audience(items, k=k + 1, score=score)
            ShardedRecommender(eng, ev_sh, k=0, chunk=100, audience=aud_c).run(rng_step=step)
            Recommender(ref, ev_full, k=0, chunk=100, audience=aud_r).run(rng_step=step)
            ids_c, sc_c = aud_c.table()
            ids_r, sc_r = aud_r.table()
            ok = ids_r[:, :k] >= 0
            assert np.array_equal(ids_c >= 0, ok)                                                # the same padding
            a, b = sc_c.astype(np.float64), sc_r.astype(np.float64)
            with np.errstate(invalid="ignore"):
                close = (a == b[:, :k]) | (np.abs(a - b[:, :k]) <= 1e-5 * np.maximum(np.abs(a), np.abs(b[:, :k])))
                near = np.abs(b[:, 1:] - b[:, :-1]) <= 2e-5 * np.maximum(np.abs(b[:, 1:]), np.abs(b[:, :-1]))   # entry i and entry i + 1
                rel = np.where(ok & (a != b[:, :k]), np.abs(a - b[:, :k]) / np.maximum(np.abs(a), np.abs(b[:, :k])), 0.0)
            near &= ids_r[:, 1:] >= 0                                                        # (padding is nobody's neighbour)
            near[np.isinf(b[:, 1:]) & np.isinf(b[:, :-1]) & (ids_r[:, 1:] >= 0)] = True      # (two -inf scores are a tie)
            clear = ok.copy()
            clear &= ~near[:, :k]                                                            # the next entry is clearly below
            clear[:, 1:] &= ~near[:, :k - 1]                                                 # the previous one clearly above
            bad_ids = int((ids_c[clear] != ids_r[:, :k][clear]).sum())
            if rank == 0:                                                                    # the figures, before anything is asserted
                print("%s %s world=%d score=%s: largest relative score difference sharded / unsharded %.3e over %d entries, %d beyond "
                      "1e-5; %d ids differ among the %d entries away from near-ties" %
                      (workload, precision, world, score, rel.max(), int(ok.sum()), int((~close[ok]).sum()), bad_ids, int(clear.sum())), flush=True)
            if precision == "fp32":                                                          # (the docstring says why)
                assert close[ok].all(), ("scores differ beyond the near-tie bound", score, float(rel.max()))
                assert bad_ids == 0, ("ids differ away from near-ties", score, bad_ids)
    H.close_ranks("AUDIENCE_SHARDED_OK world=%d workload=%s queries=%d clear=%.4f slabs=%s" % (world, workload, len(items), clear.mean(),
                                                                                              H.slab_sizes(I, world)))


if __name__ == "__main__":
    main()
