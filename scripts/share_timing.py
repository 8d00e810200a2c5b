#!/usr/bin/env python3
"""Timing of the share-targeted lists (trainer.ShareTarget: two ltg_topk_groups lists per chunk, then ltg_topk_share once over the split),
on two workloads:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items; k = 100, the niche items of the
              data set promoted to ten points more of all slots than the plain lists give them
  s20k        20 000 users x 20 000 items, synthetic: a freshly initialised generator whose output bias is log Zipf popularity, as steep
              as the users' own spread of a logit, so that the plain lists pile onto a head as a trained model's do and the users still
              differ; k = 100, the items the plain lists recommend at most the median number of times promoted
              likewise

  arm plain   Recommender.run (k = 100) -- the walk this change leaves as it was, so it is also the parent commit's figure on the same
              box and inputs
  arm share   the same with share=ShareTarget(labels, 2, [1], plain share + 0.1)
  arm slots   the same with rule=MinSlots(labels, 2, [0, M]), M the smallest minimum whose lists hold at least as many promoted entries
              as the share arm's (found by bisection before the timing): the lever there was before

Device events around each arm (every arm ends in its own device-to-host copy of the table), 2 warm-up and --reps timed repetitions, the
arms alternated in one process; median / min / max in microseconds.  Beside them, on the lists the share arm gathered: ltg_topk_share
alone (19 launches, no read-back).  And what the rule buys: the total step cost (the score given up, summed exactly over the swaps) of
the share lists and of the MinSlots lists at M.  One JSON line per workload.  Without --workload every workload runs in a fresh child
process under its own `timeout`, and the first child that does not end clean ends the run."""
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
GAIN = 0.1                                           # the target: this much more of all slots than the plain lists give


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


def lost_score(plain_sc, sc):
    """the score a table gives up against the plain one: sum of the plain scores minus sum of its own, in float64 (both tables hold the
    same number of entries per row, so this is the total step cost up to fp32 rounding of the single steps)"""
    a, b = np.asarray(plain_sc, np.float64), np.asarray(sc, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(a[ok].sum() - b[ok].sum())


def measure(name, eng, ev, labels, reps):
    from ltgan.trainer import MinSlots, Recommender, ShareTarget
    step, k = 2 * 10 ** 9, 100
    promoted = np.nonzero(labels == 1)[0]
    count = lambda ids: int(np.isin(ids, promoted).sum())
    r0 = Recommender(eng, ev, k=k)
    zero = ShareTarget(labels, 2, [1], 0.0)
    Recommender(eng, ev, k=k, share=zero).run(rng_step=step)
    target = min(1.0, round(zero.stats()["plain_share"] + GAIN, 3))
    tgt = ShareTarget(labels, 2, [1], target)
    r1 = Recommender(eng, ev, k=k, share=tgt)
    plain_ids, plain_sc = r0.run(rng_step=step)
    ids, sc = r1.run(rng_step=step)
    st = tgt.stats()
    total = count(ids)
    lo, hi = 0, k                                        # the smallest M whose MinSlots lists hold at least `total` promoted entries
    while lo < hi:
        mid = (lo + hi) // 2
        got = count(Recommender(eng, ev, k=k, rule=MinSlots(labels, 2, [0, mid])).run(rng_step=step)[0])
        lo, hi = (lo, mid) if got >= total else (mid + 1, hi)
    M = lo
    r2 = Recommender(eng, ev, k=k, rule=MinSlots(labels, 2, [0, M]))
    ids2, sc2 = r2.run(rng_step=step)
    t0, t1, t2 = timed([lambda: r0.run(rng_step=step), lambda: r1.run(rng_step=step), lambda: r2.run(rng_step=step)], reps)
    so, io = torch.empty_like(r1.scores), torch.empty_like(r1.ids)
    (tm,) = timed([lambda: eng.topk_share(tgt.pro_s, tgt.pro_i, tgt.rest_s, tgt.rest_i, k, tgt.want, so, io, tgt.state, tgt.ws)], reps)
    assert torch.equal(io, r1.ids)
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=r0.chunk, k=k, target=target, reps=reps, warmup=WARMUP,
                          run_plain_us=stats(t0), run_share_us=stats(t1), run_min_slots_us=stats(t2),
                          share_over_plain_median=round(float(np.median(t1) / np.median(t0)), 3),
                          min_slots_over_plain_median=round(float(np.median(t2) / np.median(t0)), 3),
                          share_over_min_slots_median=round(float(np.median(t1) / np.median(t2)), 3),
                          ltg_topk_share_us=stats(tm), ltg_topk_share_over_plain_run=round(float(np.median(tm) / np.median(t0)), 4),
                          plain_share=round(st["plain_share"], 6), reached_share=round(st["share"], 6), reached=st["reached"],
                          steps_taken=st["taken"], steps_available=st["available"], rows_changed=st["rows_changed"], price=st["price"],
                          promoted_share_lists=total, min_slots_M=M, promoted_min_slots_lists=count(ids2),
                          score_given_up_share=round(lost_score(plain_sc, sc), 3), score_given_up_min_slots=round(lost_score(plain_sc, sc2), 3))),
          flush=True)


def s20k():
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Recommender
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
    ids, _ = Recommender(eng, ev, k=100).run(rng_step=2 * 10 ** 9)
    hits = np.bincount(ids[ids >= 0], minlength=I)
    return eng, ev, (hits <= np.median(hits)).astype(np.uint8)


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
            labels, _ = lt.build_groups(ds, "niche", 2, n_items)
            gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
        measure("askubuntu", gen.engine, EvalData(tr, te, gen.engine.device), labels, reps)
    else:
        eng, ev, labels = s20k()
        measure("s20k", eng, ev, labels, reps)


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
