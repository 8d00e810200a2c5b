#!/usr/bin/env python3
"""Timing of the minimum-slots rule (trainer.MinSlots: ltg_topk_groups + ltg_topk_quota), on the two workloads of longtail_timing.py:

  askubuntu   Askubuntu_Sample's test split (tests/golden/askubuntu_raw.npz): 10 000 users, 1 000 items, pop:4 groups
  c200k       one evaluation chunk at 200 000 items: eval_chunk_rows(200 000) = 2 684 users, pop:4 groups

  arm 0  Recommender.run (k = 100) without a rule
  arm 1  the same with one reserved group   (pop3: 30)
  arm 4  the same with four reserved groups (pop0 .. pop3: 10 / 20 / 30 / 40)

Device events around each arm (every arm ends in its own device-to-host copy of the table), 3 warm-up and 20 timed repetitions, the
arms alternated in one process; median / min / max in microseconds.  Beside them single launches on the first chunk's logits: ltg_topk,
ltg_topk_groups (one bit; k = 100 and k = 30) and ltg_topk_quota (one and four lists).  One JSON line per workload.  The per-kernel
lines come from a separate `rocprofv3 --kernel-trace --stats` run of this script (`--reps 3` keeps it short).

--plain-topk    times ltg_topk alone on the c200k chunk (topk_timing.py's workload) with whatever library _cabi binds, one JSON line.
--ab PARENT_SO  the plain path against an older build: fresh children of --plain-topk, alternated parent / new / parent / new (one
                process binds one library; the parent is loaded with LTG_HIP_LIB + LTG_AB_COMPAT=1, it lacks the two new exports),
                every child under its own `timeout`, the first failing child ends the run.  The margin is the spread of the
                parent's own arms."""
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
    from ltgan.trainer import MinSlots, Recommender
    step, k = 2 * 10 ** 9, 100
    r0 = Recommender(eng, ev, k=k)
    rule1, rule4 = MinSlots(labels, 4, [0, 0, 0, 30]), MinSlots(labels, 4, [10, 20, 30, 40])
    r1 = Recommender(eng, ev, k=k, rule=rule1)
    r4 = Recommender(eng, ev, k=k, rule=rule4)
    t0, t1, t4 = timed([lambda: r0.run(rng_step=step), lambda: r1.run(rng_step=step), lambda: r4.run(rng_step=step)], reps)
    ok1 = bool(((labels[r1.ids.cpu().numpy()] == 3).sum(1) >= 30).all())
    # single launches on the first chunk: its logits are rebuilt by one forward, the lists are the arms'
    n = r0.chunk
    tr, _ = ev.rows(0, n)
    eng.forward(tr, r0.acts, keep_prob=0.75, is_training=0.0, rng_step=step)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    s100, i100, s30, i30, so, io = new(n, k), new(n, k, dt=torch.int32), new(n, 30), new(n, 30, dt=torch.int32), new(n, k), new(n, k, dt=torch.int32)
    a_s, a_i = rule4.plain(n, k)
    g4s, g4i = rule4.reserved(n)
    g1s, g1i = rule1.reserved(n)
    tt, tg, tg30, tq1, tq4 = timed([lambda: eng.topk(r0.acts, tr, k, s100, i100),
                                    lambda: eng.topk_groups(r0.acts, tr, k, rule1.labels, 1 << 3, s100, i100),
                                    lambda: eng.topk_groups(r0.acts, tr, 30, rule1.labels, 1 << 3, s30, i30),
                                    lambda: eng.topk_quota(a_s, a_i, g1s, g1i, rule1.quota, so, io),
                                    lambda: eng.topk_quota(a_s, a_i, g4s, g4i, rule4.quota, so, io)], reps)
    tf, = timed([lambda: eng.forward(tr, r0.acts, keep_prob=0.75, is_training=0.0, rng_step=step)], reps)
    print(json.dumps(dict(workload=name, users=ev.n, items=eng.I, chunk_rows=n, k=k, reps=reps, warmup=WARMUP,
                          run_no_rule_us=stats(t0), run_one_group_us=stats(t1), run_four_groups_us=stats(t4),
                          one_group_over_none_median=round(float(np.median(t1) / np.median(t0)), 3),
                          four_groups_over_none_median=round(float(np.median(t4) / np.median(t0)), 3),
                          forward_us=stats(tf), k_topk_us=stats(tt), k_topk_groups_k100_us=stats(tg), k_topk_groups_k30_us=stats(tg30),
                          k_topk_quota_one_list_us=stats(tq1), k_topk_quota_four_lists_us=stats(tq4), every_user_has_30_of_pop3=ok1)), flush=True)


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


def plain_topk(reps):
    from ltgan import _cabi as cabi
    eng, ev, _ = c200k()
    n, k = ev.n, 100
    tr, _ = ev.rows(0, n)
    acts = eng.new_acts(n)
    eng.forward(tr, acts, keep_prob=0.75, is_training=0.0, rng_step=2 * 10 ** 9)
    s = torch.empty(n, k, dtype=torch.float32, device=eng.device)
    i = torch.empty(n, k, dtype=torch.int32, device=eng.device)
    t, = timed([lambda: eng.topk(acts, tr, k, s, i)], reps)
    print(json.dumps(dict(lib=os.path.relpath(cabi.LIB_PATH, ROOT), rows=n, items=eng.I, k=k, reps=reps, k_topk_us=stats(t),
                          id_checksum=int(i.to(torch.int64).sum().item()))), flush=True)


def ab(parent_so, reps, rounds):
    res = {"parent": [], "new": []}
    for _ in range(rounds):
        for arm in ("parent", "new"):
            env = dict(os.environ)
            env.pop("LTG_HIP_LIB", None)
            if arm == "parent":
                env.update(LTG_HIP_LIB=os.path.abspath(parent_so), LTG_AB_COMPAT="1")
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--plain-topk", "--reps", str(reps)],
                               env=env, capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("the %s arm failed (%d): %s" % (arm, r.returncode, r.stderr[-2000:]))
            line = r.stdout.strip().splitlines()[-1]
            print(arm, line, flush=True)
            res[arm].append(json.loads(line))
    med = {a: [x["k_topk_us"]["median"] for x in res[a]] for a in res}
    assert len({x["id_checksum"] for a in res for x in res[a]}) == 1, "the two builds disagree on the lists"
    print(json.dumps(dict(parent_medians_us=med["parent"], new_medians_us=med["new"], parent_spread_us=round(max(med["parent"]) - min(med["parent"]), 1),
                          new_minus_parent_us=round(float(np.mean(med["new"]) - np.mean(med["parent"])), 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", default="askubuntu,c200k")
    ap.add_argument("--plain-topk", action="store_true")
    ap.add_argument("--ab", default=None, metavar="PARENT_SO")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if a.ab:
        return ab(a.ab, a.reps, a.rounds)
    assert torch.cuda.is_available(), "a timing needs the GPU"
    if a.plain_topk:
        return plain_topk(a.reps)
    from ltgan import data_processing as dp
    from ltgan import longtail as lt
    from ltgan.dataset import EvalData, count_items, materialize_askubuntu
    from ltgan.generator import generator_VAECF
    if "askubuntu" in a.workloads:
        with tempfile.TemporaryDirectory() as tmp:
            ds = materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), os.path.join(tmp, "Askubuntu_Sample"))
            n_items = count_items(ds)
            tr, te, _ = dp.load_tr_te_data(os.path.join(ds, "test_tr.csv"), os.path.join(ds, "test_te.csv"), n_items)
            labels, _ = lt.build_groups(ds, "pop", 4, n_items)
            gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
        measure("askubuntu", gen.engine, EvalData(tr, te, gen.engine.device), labels, a.reps)
        del gen
    if "c200k" in a.workloads:
        eng, ev, X = c200k()
        labels, _ = lt.pop_groups_from_counts(np.asarray(X.sum(axis=0)).ravel().astype(np.int64), 4)
        measure("c200k", eng, ev, labels, a.reps)


if __name__ == "__main__":
    main()
