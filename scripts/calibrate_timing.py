#!/usr/bin/env python3
"""Timing of the calibrated lists (trainer.Calibrate: ltg_topk_groups per class + ltg_hist_groups + ltg_topk_calibrate), on the two
workloads of quota_timing.py:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items, pop:4 groups
  c200k       one evaluation chunk at 200 000 items: eval_chunk_rows(200 000) = 2 684 users, pop:4 groups

  arm plain      Recommender.run (k = 100)
  arm min-slots  the same with MinSlots over the four groups (10 / 20 / 30 / 40): the plain list and four per-group ltg_topk_groups passes
  arm calibrate  the same with Calibrate(lam = 0.9) over the same groups: four per-class ltg_topk_groups passes, no plain list

Device events around each arm (every arm ends in its own device-to-host copy of the table), 3 warm-up and 20 timed repetitions, the
arms alternated in one process; median / min / max in microseconds.  Beside them single launches on the first chunk: ltg_topk_groups
(one class, k = 100), ltg_hist_groups and ltg_topk_calibrate (lam = 0.9 and lam = 0), ltg_topk_quota (four lists) for scale.  One JSON
line per workload.  Without --workload every workload runs in a fresh child process under its own `timeout`, and the first child that
does not end clean ends the run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP = 3
LIMIT_S = {"askubuntu": 300, "c200k": 420}


def stats(t):
    return dict(median=round(float(np.median(t)), 1), min=round(float(min(t)), 1), max=round(float(max(t)), 1))


def timed(fns, reps):
    """alternate the arms: -> one list of times (us) per arm"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, out):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
    return out


def measure(name, eng, ev, labels, reps):
    from ltgan.trainer import Calibrate, MinSlots, Recommender
    step, k, lam = 2 * 10 ** 9, 100, 0.9
    r0 = Recommender(eng, ev, k=k)
    rule, cal = MinSlots(labels, 4, [10, 20, 30, 40]), Calibrate(labels, 4, lam)
    r1 = Recommender(eng, ev, k=k, rule=rule)
    r2 = Recommender(eng, ev, k=k, calibrate=cal)
    t0, t1, t2 = timed([lambda: r0.run(rng_step=step), lambda: r1.run(rng_step=step), lambda: r2.run(rng_step=step)], reps)
    st = cal.stats().astype(np.float64)
    # single launches on the first chunk: its logits are rebuilt by one forward, the lists are the arms'
    n = r0.chunk
    tr, _ = ev.rows(0, n)
    eng.forward(tr, r0.acts, keep_prob=0.75, is_training=0.0, rng_step=step)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    s100, i100, so, io, sst = new(n, k), new(n, k, dt=torch.int32), new(n, k), new(n, k, dt=torch.int32), new(n, 2)
    g_s, g_i = cal.class_lists(n, k)
    for j, mask in enumerate(cal.masks):
        eng.topk_groups(r0.acts, tr, k, cal.labels, mask, g_s[j], g_i[j])
    hist = new(n, 5, dt=torch.int32)
    a_s, a_i = rule.plain(n, k)
    q_s, q_i = rule.reserved(n)
    tg, th, tc, tc0, tq = timed([lambda: eng.topk_groups(r0.acts, tr, k, cal.labels, 1 << 3, s100, i100),
                                 lambda: eng.hist_groups(tr, cal.labels, 4, hist, hist_lo=0),
                                 lambda: eng.topk_calibrate(g_s, g_i, cal.classes, 4, hist, lam, k, so, io, sst),
                                 lambda: eng.topk_calibrate(g_s, g_i, cal.classes, 4, hist, 0.0, k, so, io, sst),
                                 lambda: eng.topk_quota(a_s, a_i, q_s, q_i, rule.quota, so, io)], reps)
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=n, k=k, lam=lam, classes=cal.classes, reps=reps, warmup=WARMUP,
                          run_plain_us=stats(t0), run_min_slots_us=stats(t1), run_calibrate_us=stats(t2),
                          calibrate_over_plain_median=round(float(np.median(t2) / np.median(t0)), 3),
                          calibrate_over_min_slots_median=round(float(np.median(t2) / np.median(t1)), 3),
                          k_topk_groups_k100_us=stats(tg), k_hist_groups_us=stats(th), k_topk_calibrate_us=stats(tc),
                          k_topk_calibrate_lam0_us=stats(tc0), k_topk_quota_four_lists_us=stats(tq),
                          miscal_before=round(float(st[:, 0].mean()), 6), miscal_after=round(float(st[:, 1].mean()), 6))), flush=True)


def c200k():
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import eval_chunk_rows
    I = 200000
    rows = eval_chunk_rows(I)
    X = Hh.random_history(np.random.default_rng(0), rows, I, mean_nnz=40)
    eng = Engine(I, precision="bf16", seed=1)
    return eng, EvalData(X, X, eng.device), X


def one(workload, reps):
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from ltgan import data_processing as dp
    from ltgan import longtail as lt
    from ltgan.dataset import EvalData, count_items, materialize_askubuntu
    from ltgan.generator import generator_VAECF
    if workload == "askubuntu":
        with tempfile.TemporaryDirectory() as tmp:
            ds = materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), os.path.join(tmp, "Askubuntu_Sample"))
            n_items = count_items(ds)
            tr, te, _ = dp.load_tr_te_data(os.path.join(ds, "test_tr.csv"), os.path.join(ds, "test_te.csv"), n_items)
            labels, _ = lt.build_groups(ds, "pop", 4, n_items)
            gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
        measure("askubuntu", gen.engine, EvalData(tr, te, gen.engine.device), labels, reps)
    else:
        eng, ev, X = c200k()
        labels, _ = lt.pop_groups_from_counts(np.asarray(X.sum(axis=0)).ravel().astype(np.int64), 4)
        measure("c200k", eng, ev, labels, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", default="askubuntu,c200k")
    ap.add_argument("--workload", default=None, choices=sorted(LIMIT_S))
    a = ap.parse_args()
    if a.workload:
        return one(a.workload, a.reps)
    for w in a.workloads.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S[w]), sys.executable, os.path.abspath(__file__), "--workload", w, "--reps", str(a.reps)])
        if r.returncode != 0:
            sys.exit("the %s workload did not end clean (%d): nothing more is started" % (w, r.returncode))


if __name__ == "__main__":
    main()
