#!/usr/bin/env python3
"""Timing of the posterior-aware scores (serving.Posterior: ltg_posterior_h2 + ltg_posterior_scores per row block) against the composition
they replace, on one chunk of 2 048 users with S = 16 samples, beta = 1:

  i20000    20 000 items
  i200000   200 000 items (the bf16 shadow of W_p1t is present at both sizes)

fused        ltg_posterior_h2 + ltg_posterior_scores: the image is written once (rows * S * 608 * 2 bytes), the scores once (rows * I * 4)
composition  S times Engine.forward(is_training = 1, eps = eps[:, s]) with keep_prob = 1, each followed by two in-place torch updates
             (sum += l, sumsq += l * l), then mean / std / score in torch -- the cheapest accumulation torch offers; it writes and
             re-reads the [rows, I] logits S times.  (The encoder runs S times in it as well; its share is reported by the
             `forward_once_us` figure against `composition_us / S`.)

Device events around each arm, 3 warm-up and `--reps` timed repetitions, the arms alternated in one process; median / min / max in
microseconds.  The product's operations are 2 * rows * S * I * 608 (the padded K); `scores_tflops` is that over the median kernel time of
ltg_posterior_scores alone, `share_of_bf16_peak` that over 2 500 TFLOP/s.  The largest difference between the two arms' scores is
printed as well (different kernels and K orders, E[x^2] - E[x]^2 on the torch side).  One JSON line per workload; every workload runs in
a fresh child process under its own `timeout`, and the first child that does not end clean ends the run."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP = 3
ITEMS = {"i20000": 20000, "i200000": 200000}
LIMIT_S = {"i20000": 300, "i200000": 420}
BF16_PEAK_TFLOPS = 2500.0


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


def one(workload, reps, rows=2048, S=16, beta=1.0):
    assert torch.cuda.is_available(), "a timing needs the GPU"
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    I = ITEMS[workload]
    X = Hh.random_history(np.random.default_rng(0), rows, I, mean_nnz=40)
    eng = Engine(I, precision="bf16", seed=1)
    dev = eng.device
    ev = EvalData(X, X, dev)
    tr, _ = ev.rows(0, rows)
    acts = eng.new_acts(rows)
    eps = torch.randn(S, rows, eng.Z, device=dev)                       # [S][rows][Z]: one contiguous block per forward
    eps_rsz = eps.permute(1, 0, 2).contiguous()                         # [rows][S][Z]: what ltg_posterior_h2 takes
    acc, sq = torch.empty(rows, I, device=dev), torch.empty(rows, I, device=dev)

    def composition():
        acc.zero_()
        sq.zero_()
        for s in range(S):
            eng.forward(tr, acts, keep_prob=1.0, is_training=1.0, rng_step=1, eps=eps[s])
            acc.add_(acts.logits)
            sq.addcmul_(acts.logits, acts.logits)
        acc.div_(S)                                                      # mean
        sq.div_(S).addcmul_(acc, acc, value=-1.0).clamp_(min=0.0).sqrt_()   # std
        acc.add_(sq, alpha=beta)                                         # score, in place of the mean

    image = eng.posterior_image(rows, S)
    score = torch.empty(rows, I, device=dev)
    eng.forward(tr, acts, keep_prob=1.0, is_training=0.0, rng_step=1)
    mulv = acts.mulv.clone()

    def fused():
        eng.posterior_h2(mulv, rows, 0, S, 0, image, eps=eps_rsz)
        eng.posterior_scores(image, rows, S, beta, score)

    t_comp, t_fused = timed([composition, fused], reps)
    diff = float((acc - score).abs().max())
    t_h2, t_sc, t_fwd = timed([lambda: eng.posterior_h2(mulv, rows, 0, S, 0, image, eps=eps_rsz),
                               lambda: eng.posterior_scores(image, rows, S, beta, score),
                               lambda: eng.forward(tr, acts, keep_prob=1.0, is_training=1.0, rng_step=1, eps=eps[0])], reps)
    flop = 2.0 * rows * S * I * 608
    tf = flop / (float(np.median(t_sc)) * 1e-6) / 1e12
    print(json.dumps(dict(workload=workload, rows=rows, items=I, samples=S, beta=beta, reps=reps, warmup=WARMUP,
                          composition_us=stats(t_comp), fused_us=stats(t_fused),
                          composition_over_fused_median=round(float(np.median(t_comp) / np.median(t_fused)), 2),
                          k_post_h2_us=stats(t_h2), k_post_scores_us=stats(t_sc), forward_once_us=stats(t_fwd),
                          scores_tflops=round(tf, 1), share_of_bf16_peak=round(tf / BF16_PEAK_TFLOPS, 4),
                          bytes_written_fused=int(rows * S * 608 * 2 + rows * I * 4), bytes_logits_composition=int(S * rows * I * 4),
                          largest_score_difference=diff)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workloads", default="i20000,i200000")
    ap.add_argument("--workload", default=None, choices=sorted(ITEMS))
    a = ap.parse_args()
    if a.workload:
        return one(a.workload, a.reps)
    for w in a.workloads.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S[w]), sys.executable, os.path.abspath(__file__), "--workload", w, "--reps", str(a.reps)])
        if r.returncode != 0:
            sys.exit("the %s workload did not end clean (%d): nothing more is started" % (w, r.returncode))


if __name__ == "__main__":
    main()
