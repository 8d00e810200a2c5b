#!/usr/bin/env python3
"""Timing of the exploration lists (trainer.Explore: ltg_topk_sample + ltg_topk_sample_mass + ltg_topk_sample_finish per chunk), on two
workloads:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items, one chunk
  c25024      4 096 users x 25 024 items, one chunk, random histories

Single launches on the chunk's logits (one forward builds them), k = 100, T = 1, no fixed head: ltg_topk for scale, then the three
launches of the sampled lists, and the whole Recommender.run plain and with Explore (which adds one plain ltg_topk per chunk for the
explored share).  Device events around each launch, 3 warm-up and 20 timed repetitions, the arms alternated in one process; median /
min / max in microseconds.  One JSON line per workload.  Without --workload every workload runs in a fresh child process under its own
`timeout`, and the first child that does not end clean ends the run."""
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
LIMIT_S = {"askubuntu": 300, "c25024": 300}


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


def measure(name, eng, ev, reps):
    from ltgan.trainer import Explore, Recommender
    step, k, T = 2 * 10 ** 9, 100, 1.0
    r0 = Recommender(eng, ev, k=k)
    exp = Explore(T)
    r1 = Recommender(eng, ev, k=k, explore=exp)
    t_plain, t_exp = timed([lambda: r0.run(rng_step=step), lambda: r1.run(rng_step=step)], reps)
    n = r0.chunk
    tr, _ = ev.rows(0, n)
    eng.forward(tr, r0.acts, keep_prob=0.75, is_training=0.0, rng_step=step)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    s_o, i_o, key, ids, sc, lp, mx, rest = new(n, k), new(n, k, dt=torch.int32), new(n, k), new(n, k, dt=torch.int32), new(n, k), new(n, k), new(n), new(n)
    it = float(exp.inv_temp)
    eng.topk_sample(r0.acts, tr, 0, k, it, 0, None, key, ids)
    eng.topk_sample_mass(r0.acts, tr, it, None, ids, sc, mx, rest)
    t_topk, t_sample, t_mass, t_fin = timed([lambda: eng.topk(r0.acts, tr, k, s_o, i_o),
                                             lambda: eng.topk_sample(r0.acts, tr, 0, k, it, 0, None, key, ids),
                                             lambda: eng.topk_sample_mass(r0.acts, tr, it, None, ids, sc, mx, rest),
                                             lambda: eng.topk_sample_finish(sc, mx, rest, it, lp)], reps)
    three = float(np.median(t_sample) + np.median(t_mass) + np.median(t_fin))
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=n, k=k, temperature=T, reps=reps, warmup=WARMUP,
                          k_topk_us=stats(t_topk), k_topk_sample_us=stats(t_sample), k_topk_sample_mass_us=stats(t_mass),
                          k_topk_sample_finish_us=stats(t_fin), three_launches_median_us=round(three, 1),
                          sample_over_topk_median=round(float(np.median(t_sample) / np.median(t_topk)), 2),
                          three_over_topk_median=round(three / float(np.median(t_topk)), 2),
                          run_plain_us=stats(t_plain), run_explore_us=stats(t_exp), launches_per_chunk=4, **exp.stats())), flush=True)


def one(workload, reps):
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from ltgan import data_processing as dp
    from ltgan.dataset import EvalData, count_items, materialize_askubuntu
    from ltgan.engine import Engine
    from ltgan.generator import generator_VAECF
    if workload == "askubuntu":
        with tempfile.TemporaryDirectory() as tmp:
            ds = materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), os.path.join(tmp, "Askubuntu_Sample"))
            n_items = count_items(ds)
            tr, te, _ = dp.load_tr_te_data(os.path.join(ds, "test_tr.csv"), os.path.join(ds, "test_te.csv"), n_items)
            gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
        measure("askubuntu", gen.engine, EvalData(tr, te, gen.engine.device), reps)
    else:
        import helpers as Hh
        I, rows = 25024, 4096
        X = Hh.random_history(np.random.default_rng(0), rows, I, mean_nnz=40)
        eng = Engine(I, precision="bf16", seed=1)
        measure("c25024", eng, EvalData(X, X, eng.device), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", default="askubuntu,c25024")
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
