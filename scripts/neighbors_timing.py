#!/usr/bin/env python3
"""Standalone timing of ltg_item_neighbors against the composition a user would write without it, on the same packed operands: chunked
torch.matmul (bf16 operands, fp32 result) + torch.topk.  25 024 and 200 000 items, 4 096 queries, k = 20, cosine images of Gaussian rows.
The two arms are INTERLEAVED on one device (A B A B ...), device events around each, after a warm-up; prints one JSON line per size with
both medians, min / max (the baseline's own spread), the fused call's workspace and the bytes of scores the composition writes.
The GEMM of the composition writes fp32 directly (torch.mm(..., out_dtype=torch.float32)); a torch without that overload falls back to a
bf16 result cast to fp32, which the output line then names (gemm = "bf16+cast").
A third arm attributes the fused call's time: the same call with labels that admit no item (every accumulator is masked to "no entry":
no append, no compaction, empty lists) is the stream + MFMA + per-step barriers alone; fused - that = the selection epilogue.
The kernel times proper come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n_q, k = 4096, 20
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    dev = "cuda:0"
    st = lambda: torch.cuda.current_stream().cuda_stream
    for I in (25024, 200000):
        cfg = cabi.ltg_config(I, 600, 200, I, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
        g = torch.Generator(device=dev).manual_seed(1)
        W = torch.randn(I, 600, device=dev, generator=g)
        gen = cabi.ltg_gen_state()
        gen.p[3] = W.data_ptr()
        img = torch.empty(I, 608, dtype=torch.int16, device=dev)
        cabi.check(lib.ltg_item_pack(C.byref(cfg), C.byref(gen), 0, 0, img.data_ptr(), st()), "ltg_item_pack")
        q = torch.randperm(I, device=dev, generator=g)[:n_q].to(torch.int32)
        q_img = img[q.long()].contiguous()
        need = lib.ltg_item_neighbors_ws_bytes(C.byref(cfg), n_q, k)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        s = torch.empty(n_q, k, dtype=torch.float32, device=dev)
        i = torch.empty(n_q, k, dtype=torch.int32, device=dev)

        def fused():
            cabi.check(lib.ltg_item_neighbors(C.byref(cfg), img.data_ptr(), q_img.data_ptr(), q.data_ptr(), n_q, None, 0x1FF, k, s.data_ptr(),
                                              i.data_ptr(), ws.data_ptr(), need, st()), "ltg_item_neighbors")

        # the composition: the same bf16 operands, scores of a chunk of queries written as fp32, self masked, torch.topk
        tb, qb = img.view(torch.bfloat16), q_img.view(torch.bfloat16)
        chunk = 1024
        bs = torch.empty(n_q, k, dtype=torch.float32, device=dev)
        bi = torch.empty(n_q, k, dtype=torch.int64, device=dev)
        rows = torch.arange(chunk, device=dev)

        lab = torch.full((I,), 5, dtype=torch.uint8, device=dev)

        def no_select():                           # group_mask admits label 0 only: nothing is eligible
            cabi.check(lib.ltg_item_neighbors(C.byref(cfg), img.data_ptr(), q_img.data_ptr(), q.data_ptr(), n_q, lab.data_ptr(), 1, k,
                                              s2.data_ptr(), i2.data_ptr(), ws.data_ptr(), need, st()), "ltg_item_neighbors")

        s2, i2 = torch.empty_like(s), torch.empty_like(i)
        tbt = tb.t()
        try:
            torch.mm(qb[:16], tbt, out_dtype=torch.float32)
            gemm, mm = "fp32-out", (lambda a: torch.mm(a, tbt, out_dtype=torch.float32))
        except (TypeError, RuntimeError):
            gemm, mm = "bf16+cast", (lambda a: torch.mm(a, tbt).float())

        def composed():
            for lo in range(0, n_q, chunk):
                sc = mm(qb[lo:lo + chunk])
                sc[rows, q[lo:lo + chunk].long()] = -float("inf")
                v, ix = torch.topk(sc, k, dim=1)
                bs[lo:lo + chunk] = v
                bi[lo:lo + chunk] = ix

        for _ in range(3):
            fused()
            composed()
            no_select()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = {"fused": [], "composed": [], "no_select": []}
        for _ in range(reps):                      # interleaved: both arms see the same clocks and the same neighbours on the device
            for name, fn in (("fused", fused), ("composed", composed), ("no_select", no_select)):
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1e3)
        same = float((i.long() == bi).all(1).float().mean())      # (the composition accumulates in another order: near-ties may swap)
        out = dict(I=I, n_q=n_q, k=k, reps=reps, workspace_bytes=int(need), composed_score_bytes_per_chunk=chunk * I * 4,
                   score_matrix_bytes=n_q * I * 4, rows_identical=round(same, 4), gemm=gemm)
        for name, v in t.items():
            out[name + "_us_median"] = round(float(np.median(v)), 1)
            out[name + "_us_min"] = round(float(min(v)), 1)
            out[name + "_us_max"] = round(float(max(v)), 1)
        out["selection_us"] = round(out["fused_us_median"] - out["no_select_us_median"], 1)
        out["fused_over_composed"] = round(out["fused_us_median"] / out["composed_us_median"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
