#!/usr/bin/env python3
"""Timing of the one-forward long-tail report against what it replaces, on two workloads:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items, niche / popular groups
  c200k       one evaluation chunk at 200 000 items: eval_chunk_rows(200 000) = 2 684 users, six held-out items per user, pop:4 groups

  arm A  Evaluator.run followed by Recommender.run (k = 100): two forwards, ltg_rank_metrics' scan of the row, ltg_topk
  arm B  Recommender(report=LongTailReport).run: one forward, ltg_topk, ltg_topk_metrics

Device events around each arm (the arms end in their own device-to-host copies), 3 warm-up and 20 timed repetitions, the two arms
alternated in one process; median / min / max in microseconds.  Beside them the kernels alone on the same chunk: ltg_topk_metrics and
ltg_rank_metrics (logits and lists left by the arms), and ltg_topk_metrics with item_hits = NULL (what the exposure counts cost).  One JSON line per workload.  The per-kernel lines come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (`--reps 3` keeps it short)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP = 3


def stats(t):
    return dict(median=round(float(np.median(t)), 1), min=round(float(min(t)), 1), max=round(float(max(t)), 1))


def timed_pair(fa, fb, reps):
    """alternate the two arms: -> (times of A, times of B) in us"""
    for _ in range(WARMUP):
        fa()
        fb()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ta, tb = [], []
    for _ in range(reps):
        for fn, t in ((fa, ta), (fb, tb)):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
    return ta, tb


def measure(name, eng, ev, labels, n_groups, reps):
    from ltgan.trainer import Evaluator, LongTailReport, Recommender
    step = 2 * 10 ** 9
    e = Evaluator(eng, ev)
    r = Recommender(eng, ev, k=100)
    rep = LongTailReport(labels, n_groups)
    b = Recommender(eng, ev, k=rep.k, report=rep)

    def arm_a():
        e.run(rng_step=step)
        r.run(rng_step=step)

    def arm_b():
        b.run(rng_step=step)
        rep.table()

    ta, tb = timed_pair(arm_a, arm_b, reps)
    # the two kernels alone, on the first chunk: its logits are rebuilt by one forward, the lists are the arm's
    n = b.chunk
    tr, te = ev.rows(0, n)
    eng.forward(tr, b.acts, keep_prob=0.75, is_training=0.0, rng_step=step)
    out4 = torch.zeros(n, 4, dtype=torch.float32, device=eng.device)
    tk, ts = timed_pair(lambda: eng.topk_metrics(b.ids[:n], te, rep.labels, n_groups, rep.out, rep.item_hits, **rep.cut),
                        lambda: eng.rank_metrics(b.acts, tr, te, out4), reps)
    tn, _ = timed_pair(lambda: eng.topk_metrics(b.ids[:n], te, rep.labels, n_groups, rep.out, None, **rep.cut),
                       lambda: eng.topk_metrics(b.ids[:n], te, rep.labels, n_groups, rep.out, rep.item_hits, **rep.cut), reps)
    same = bool(torch.equal(rep.out[:n, n_groups].view(torch.int32), out4.view(torch.int32)))
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=n, n_groups=n_groups, reps=reps, warmup=WARMUP,
                          arm_a_evaluator_then_recommender_us=stats(ta), arm_b_one_forward_report_us=stats(tb),
                          b_over_a_median=round(float(np.median(tb) / np.median(ta)), 3),
                          k_topk_metrics_us=stats(tk), k_rank_metrics_us=stats(ts), k_topk_metrics_without_item_hits_us=stats(tn), all_slot_bit_equal_to_rank_metrics=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", default="askubuntu,c200k")
    a = ap.parse_args()
    import helpers as Hh
    import scipy.sparse as sp
    from ltgan import data_processing as dp
    from ltgan import longtail as lt
    from ltgan.dataset import EvalData, count_items, materialize_askubuntu
    from ltgan.engine import Engine
    from ltgan.generator import generator_VAECF
    from ltgan.trainer import eval_chunk_rows
    assert torch.cuda.is_available(), "a timing needs the GPU"
    if "askubuntu" in a.workloads:
        with tempfile.TemporaryDirectory() as tmp:
            ds = materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), os.path.join(tmp, "Askubuntu_Sample"))
            n_items = count_items(ds)
            tr, te, _ = dp.load_tr_te_data(os.path.join(ds, "test_tr.csv"), os.path.join(ds, "test_te.csv"), n_items)
            labels, names = lt.build_groups(ds, "niche", 2, n_items)
            gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
        measure("askubuntu", gen.engine, EvalData(tr, te, gen.engine.device), labels, len(names), a.reps)
        del gen
    if "c200k" in a.workloads:
        I = 200000
        rows = eval_chunk_rows(I)
        rng = np.random.default_rng(0)
        X = Hh.random_history(rng, rows, I, mean_nnz=40)
        r = np.repeat(np.arange(rows), 6)
        T = sp.csr_matrix((np.ones(len(r), np.float32), (r, np.random.default_rng(11).integers(0, I, len(r)))), shape=(rows, I))
        T = T - T.multiply(X)                                          # held-out and fold-in disjoint, as load_tr_te_data's splits are
        T.eliminate_zeros()
        labels, names = lt.pop_groups_from_counts(np.asarray(X.sum(axis=0)).ravel().astype(np.int64), 4)
        eng = Engine(I, precision="bf16", seed=1)
        measure("c200k", eng, EvalData(X, T, eng.device), labels, len(names), a.reps)


if __name__ == "__main__":
    main()
