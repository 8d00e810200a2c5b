#!/usr/bin/env python3
"""Standalone timing of ltg_topk against the forward that produces its logits: I = 200 000 items, k = 100, one evaluation chunk of
eval_chunk_rows(200 000) = 2 684 users, device events around each launch after a warm-up.  Prints the top-K time, the forward time of
the same chunk, and the logits bytes over the top-K time as a fraction of 8 TB/s.  The kernel time proper comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import eval_chunk_rows
    I, k, reps = 200000, 100, 20
    rows = eval_chunk_rows(I)
    X = Hh.random_history(np.random.default_rng(0), rows, I, mean_nnz=40)
    eng = Engine(I, precision="bf16", seed=1)
    ev = EvalData(X, X, eng.device)
    tr, _ = ev.rows(0, rows)
    acts = eng.new_acts(rows)
    s = torch.empty(rows, k, dtype=torch.float32, device=eng.device)
    i = torch.empty(rows, k, dtype=torch.int32, device=eng.device)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = []
        for _ in range(reps):
            ev0.record()
            fn()
            ev1.record()
            ev1.synchronize()
            t.append(ev0.elapsed_time(ev1) * 1e3)
        return float(np.median(t)), float(min(t)), float(max(t))

    fwd = timed(lambda: eng.forward(tr, acts, keep_prob=0.75, is_training=0.0, rng_step=2 * 10 ** 9))
    top = timed(lambda: eng.topk(acts, tr, k, s, i))
    nbytes = rows * I * 4
    print(json.dumps(dict(I=I, k=k, rows=rows, topk_us_median=round(top[0], 1), topk_us_min=round(top[1], 1), topk_us_max=round(top[2], 1),
                          forward_us_median=round(fwd[0], 1), forward_us_min=round(fwd[1], 1), logits_bytes=nbytes,
                          topk_fraction_of_8TBps=round(nbytes / (top[0] * 1e-6) / 8e12, 3), reps=reps)))


if __name__ == "__main__":
    main()
