#!/usr/bin/env python3
"""Timing of the exposure-capped lists (trainer.ExposureCap: ltg_topk at the candidates' length per chunk, then ltg_cap_index /
ltg_cap_rounds / ltg_cap_finish once over the split), on two workloads:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items; k = 100, 400 candidates, cap =
              a tenth of the users
  s20k        20 000 users x 20 000 items, synthetic: a freshly initialised generator whose output bias is log Zipf popularity, as steep
              as the users' own spread of a logit, so that the plain lists pile onto a head as a trained model's do and the users still
              differ; k = 100, 400 candidates, cap = a tenth of the users (the plain head is in all but a few lists)

  arm plain   Recommender.run (k = 100) -- the walk this change leaves as it was, so it is also the parent commit's figure on the same
              box and inputs
  arm capped  the same with cap=ExposureCap(cap), score logprob

Device events around each arm (every arm ends in its own device-to-host copy of the table), 2 warm-up and --reps timed repetitions, the
arms alternated in one process; median / min / max in microseconds.  Beside them, on the candidates the capped arm gathered: the whole
matching (index + rounds in batches of 4 with one 32-byte read-back per batch + finish), ltg_cap_index alone, one converged round
(propose + accept when no item is over its cap: the floor of a round), the mean round of the matching, and ltg_cap_finish.  One JSON
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

WARMUP = 2
LIMIT_S = {"askubuntu": 300, "s20k": 420}


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


def measure(name, eng, ev, C, reps):
    from ltgan.trainer import ExposureCap, Recommender
    step, k, c = 2 * 10 ** 9, 100, 400
    cap = ExposureCap(C, candidates=c)
    r0 = Recommender(eng, ev, k=k)
    r1 = Recommender(eng, ev, k=k, cap=cap)
    t0, t1 = timed([lambda: r0.run(rng_step=step), lambda: r1.run(rng_step=step)], reps)
    ids, _ = r1.run(rng_step=step)
    st = cap.stats()
    pl = cap.plain_ids(k)
    plain = np.bincount(pl[pl >= 0], minlength=eng.I_global)
    hits = np.bincount(ids[ids >= 0], minlength=eng.I_global)
    # the pieces, on the candidates of that run
    so, io = torch.empty_like(r1.scores), torch.empty_like(r1.ids)

    def settle():
        eng.cap_rounds(cap.cand_s, cap.cand_i, cap.lse, cap.cap, k, 1, cap.state, cap.ws)

    tm, ti = timed([lambda: cap.match(eng, k, so, io), lambda: eng.cap_index(cap.cand_i, cap.n_items, cap.state, cap.ws)], reps)
    cap.match(eng, k, so, io)                            # converged thresholds again: the index above reset them
    tr_, tf = timed([settle, lambda: eng.cap_finish(cap.cand_s, cap.cand_i, cap.n_items, k, so, io, cap.state, cap.ws)], reps)
    assert torch.equal(io, r1.ids)
    enq = -(-st["rounds"] // cap.batch) * cap.batch      # the rounds the matching enqueues: whole batches
    per_round = (np.median(tm) - np.median(ti) - np.median(tf)) / enq
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=r0.chunk, k=k, candidates=c, cap=C, reps=reps, warmup=WARMUP,
                          run_plain_us=stats(t0), run_capped_us=stats(t1),
                          capped_over_plain_median=round(float(np.median(t1) / np.median(t0)), 3),
                          matching_us=stats(tm), matching_over_plain_run=round(float(np.median(tm) / np.median(t0)), 3),
                          k_cap_index_us=stats(ti), converged_round_us=stats(tr_), k_cap_finish_us=stats(tf),
                          rounds=st["rounds"], rounds_enqueued=enq, mean_round_us=round(float(per_round), 1),
                          max_exposure_plain=int(plain.max()), max_exposure_capped=int(hits.max()),
                          items_at_cap=int((hits == C).sum()), short_lists=st["short"], passed_over=st["passed_over"])), flush=True)


def s20k():
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    n = I = 20000
    rng = np.random.default_rng(0)
    X = Hh.random_history(rng, n, I, mean_nnz=40)
    eng = Engine(I, precision="bf16", seed=1)
    ev = EvalData(X, X, eng.device)
    m = 1024                                             # the users' own spread of a logit, from the first rows
    acts = eng.new_acts(m)
    eng.forward(ev.rows(0, m)[0], acts, keep_prob=0.75, is_training=0.0, rng_step=0)
    sigma = float(acts.logits[:m].std(dim=0).mean())
    bias = -sigma * np.log(np.arange(1, I + 1, dtype=np.float64))[rng.permutation(I)]
    eng.g_p[7].copy_(torch.from_numpy(bias.astype(np.float32)).to(eng.device))
    return eng, ev


def one(workload, reps):
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from ltgan import data_processing as dp
    from ltgan.dataset import EvalData, count_items, materialize_askubuntu
    from ltgan.generator import generator_VAECF
    if workload == "askubuntu":
        with tempfile.TemporaryDirectory() as tmp:
            ds = materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), os.path.join(tmp, "Askubuntu_Sample"))
            n_items = count_items(ds)
            tr, te, _ = dp.load_tr_te_data(os.path.join(ds, "test_tr.csv"), os.path.join(ds, "test_te.csv"), n_items)
            gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
        measure("askubuntu", gen.engine, EvalData(tr, te, gen.engine.device), max(2, tr.shape[0] // 10), reps)
    else:
        eng, ev = s20k()
        measure("s20k", eng, ev, ev.n // 10, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workloads", default="askubuntu,s20k")
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
