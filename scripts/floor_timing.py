#!/usr/bin/env python3
"""Timing of the exposure-floor lists (trainer.ExposureFloor: ltg_topk at the candidates' length per chunk, then ltg_floor_index /
ltg_floor_rounds / ltg_floor_finish once over the split), on two workloads:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items; k = 100, 400 candidates
  s20k        20 000 users x 20 000 items, synthetic: a freshly initialised generator whose output bias is log Zipf popularity, as steep
              as the users' own spread of a logit, so that the plain lists pile onto a head as a trained model's do and leave a tail
              that nobody is shown; k = 100, 400 candidates

  arm plain   Recommender.run (k = 100) -- the walk this change leaves as it was, so it is also the parent commit's figure on the same
              box and inputs
  arm floor   the same with floor=ExposureFloor(need, 10), score logprob; need = M on the items whose plain exposure is at or below the
              median, M = that median (5 where the median is lower: a catalogue whose tail nobody is shown)
  arm capped  the same with cap=ExposureCap(a tenth of the users): the dual rule of the same build, the same candidates

Device events around each arm (every arm ends in its own device-to-host copy of the table), 2 warm-up and --reps timed repetitions, the
arms alternated in one process; median / min / max in microseconds.  Beside them, on the candidates the floor arm gathered: the whole
matching (index + rounds in batches of 4 with one 32-byte read-back per batch + finish), ltg_floor_index alone, one converged round
(select + users when no row is over its reserve: the floor of a round), the mean round of the matching, and ltg_floor_finish.  One JSON
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
LIMIT_S = {"askubuntu": 300, "s20k": 480}


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
    from ltgan.trainer import ExposureCap, ExposureFloor, Recommender
    step, k, c, R = 2 * 10 ** 9, 100, 400, 10
    r0 = Recommender(eng, ev, k=k)
    pl, _ = r0.run(rng_step=step)
    plain = np.bincount(pl[pl >= 0], minlength=eng.I_global)
    M, C = max(5, int(np.median(plain))), max(2, ev.n // 10)
    need = np.where(plain <= np.median(plain), M, 0).astype(np.int32)
    floor = ExposureFloor(need, R, candidates=c)
    r1 = Recommender(eng, ev, k=k, floor=floor)
    r2 = Recommender(eng, ev, k=k, cap=ExposureCap(C, candidates=c))
    t0, t1, t2 = timed([lambda: r0.run(rng_step=step), lambda: r1.run(rng_step=step), lambda: r2.run(rng_step=step)], reps)
    ids, _ = r1.run(rng_step=step)
    st = floor.stats()
    hits = np.bincount(ids[ids >= 0], minlength=eng.I_global)
    # the pieces, on the candidates of that run
    so, io = torch.empty_like(r1.scores), torch.empty_like(r1.ids)

    def settle():
        eng.floor_rounds(floor.cand_s, floor.cand_i, floor.lse, floor.need, k, R, 1, floor.state, floor.ws)

    def finish():
        eng.floor_finish(floor.cand_s, floor.cand_i, floor.lse, floor.need, k, R, so, io, floor.state, floor.ws, held_out=floor.held_d)

    tm, ti = timed([lambda: floor.match(eng, k, so, io), lambda: eng.floor_index(floor.cand_i, floor.n_items, floor.state, floor.ws)], reps)
    floor.match(eng, k, so, io)                          # converged limits again: the index above reset them
    tr_, tf = timed([settle, finish], reps)
    assert torch.equal(io, r1.ids)
    enq = -(-st["rounds"] // floor.batch) * floor.batch  # the rounds the matching enqueues: whole batches
    per_round = (np.median(tm) - np.median(ti) - np.median(tf)) / enq
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=r0.chunk, k=k, candidates=c, floor=M, reserve=R, cap=C, reps=reps,
                          warmup=WARMUP, run_plain_us=stats(t0), run_floor_us=stats(t1), run_capped_us=stats(t2),
                          floor_over_plain_median=round(float(np.median(t1) / np.median(t0)), 3),
                          floor_over_capped_median=round(float(np.median(t1) / np.median(t2)), 3),
                          matching_us=stats(tm), matching_over_plain_run=round(float(np.median(tm) / np.median(t0)), 3),
                          floor_index_us=stats(ti), converged_round_us=stats(tr_), floor_finish_us=stats(tf),
                          rounds=st["rounds"], rounds_enqueued=enq, mean_round_us=round(float(per_round), 1),
                          floor_items=st["floor_items"], short_items=st["short_items"],
                          below_floor_plain=int(((need > 0) & (plain < need)).sum()), below_floor_served=int(((need > 0) & (hits < need)).sum()),
                          inserted=st["inserted"], rows_changed=st["rows_changed"], lowerings=st["lowerings"])), flush=True)


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
        measure("askubuntu", gen.engine, EvalData(tr, te, gen.engine.device), reps)
    else:
        eng, ev = s20k()
        measure("s20k", eng, ev, reps)


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
