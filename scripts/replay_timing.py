#!/usr/bin/env python3
"""Timing of the replay of exploration logs (trainer.Replay: ltg_list_mass + ltg_replay_rows per chunk), on the two workloads of
scripts/explore_timing.py:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items, one chunk
  c25024      4 096 users x 25 024 items, one chunk, random histories

The yardstick is ltg_topk_sample_mass, which this feature does not touch.  On the chunk's logits (one forward builds them), k = 100, a log
sampled at T = 1 without a head: first the yardstick against itself (two arms of the same call: the spread every ratio has to be read
beside), then ltg_list_mass at n_pol = 1 against one call of it, ltg_list_mass at n_pol = 8 against eight calls of it, ltg_replay_rows
alone at n_pol = 1 and 8, and the whole Recommender.run (k = 0) with and without replay= at 8 temperatures.  Device events around each
arm, 3 warm-up and 20 timed repetitions, the arms alternated in one process; median / min / max in microseconds.  One JSON line per
workload.  Without --workload every workload runs in a fresh child process under its own `timeout`, and the first child that does not
end clean ends the run."""
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
TEMPS = [1.0, 0.5, 2.0, 0.7, 1.5, 3.0, 0.9, 1.2]


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
    from ltgan.serving import inv_temp_of
    from ltgan.trainer import Explore, Recommender, Replay, ReplayLog
    step, k = 2 * 10 ** 9, 100
    exp = Explore(1.0)
    ids_h, _ = Recommender(eng, ev, k=k, explore=exp).run(rng_step=step, keep_prob=1.0)
    y = (np.random.default_rng(0).random(ids_h.shape) < 0.05).astype(np.float32)
    log = ReplayLog(ids_h, exp.table(), y, n_items=eng.I_global)
    r0 = Recommender(eng, ev, k=0)
    r1 = Recommender(eng, ev, k=0, replay=Replay(log, TEMPS))
    t_plain, t_rep = timed([lambda: r0.run(rng_step=step, keep_prob=1.0), lambda: r1.run(rng_step=step, keep_prob=1.0)], reps)
    n = r0.chunk
    tr, _ = ev.rows(0, n)
    eng.forward(tr, r0.acts, keep_prob=1.0, is_training=0.0, rng_step=step)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    ids = torch.from_numpy(ids_h[:n]).to(eng.device)
    lp0, yd = torch.from_numpy(log.logp0[:n]).to(eng.device), torch.from_numpy(y[:n]).to(eng.device)
    sc, st, mx, rest1, rest8 = new(n, k), new(n, k, dt=torch.int32), new(n), new(1, n), new(8, n)
    its = [inv_temp_of(T) for T in TEMPS]
    labels = torch.zeros(eng.I_global, dtype=torch.uint8, device=eng.device)
    rows1, rows8 = new(n, 1, 2, 2, dt=torch.float64), new(n, 8, 2, 2, dt=torch.float64)
    w1, w8, fb1, fb8 = new(n, 1, dt=torch.float64), new(n, 8, dt=torch.float64), new(n, 1, dt=torch.int32), new(n, 8, dt=torch.int32)
    yard = lambda p=0: eng.topk_sample_mass(r0.acts, tr, float(its[p]), None, ids, sc, mx, rest1[0])

    def yard8():
        for p in range(8):
            yard(p)

    t_ya, t_yb = timed([yard, yard], reps)
    t_y1, t_m1 = timed([yard, lambda: eng.list_mass(r0.acts, tr, ids, None, its[:1], sc, st, mx, rest1)], reps)
    t_y8, t_m8 = timed([yard8, lambda: eng.list_mass(r0.acts, tr, ids, None, its, sc, st, mx, rest8)], reps)
    eng.list_mass(r0.acts, tr, ids, None, its, sc, st, mx, rest8)
    rest1.copy_(rest8[:1])
    t_r1, t_r8 = timed([lambda: eng.replay_rows(its[:1], None, ids, lp0, yd, sc, st, mx, rest1, labels, 1, 100.0, rows1, w1, fb1),
                        lambda: eng.replay_rows(its, None, ids, lp0, yd, sc, st, mx, rest8, labels, 1, 100.0, rows8, w8, fb8)], reps)
    med = lambda t: float(np.median(t))
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=n, k=k, reps=reps, warmup=WARMUP,
                          yardstick_a_us=stats(t_ya), yardstick_b_us=stats(t_yb), yardstick_b_over_a_median=round(med(t_yb) / med(t_ya), 3),
                          yardstick_us=stats(t_y1), list_mass_1_us=stats(t_m1), list_mass_1_over_yardstick_median=round(med(t_m1) / med(t_y1), 3),
                          yardstick_x8_us=stats(t_y8), list_mass_8_us=stats(t_m8), list_mass_8_over_eight_yardsticks_median=round(med(t_m8) / med(t_y8), 3),
                          replay_rows_1_us=stats(t_r1), replay_rows_8_us=stats(t_r8), run_plain_us=stats(t_plain), run_replay_us=stats(t_rep),
                          ess_at_T1=r1.replay.estimates()[1.0]["ess"])), flush=True)


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
