#!/usr/bin/env python3
"""Standalone timing of ltg_topk_diversify against the composition a user would write without it, on the same packed image and the same
candidate lists: per chunk of users index_select of the candidates' image rows, torch.bmm (bf16 operands, fp32 result), then k rounds of
argmax / maximum.  20 000 user rows, candidates = 200, k = 100, lambda = 0.5, cosine images of 25 024 and 200 000 Gaussian rows; the
candidates are distinct random ids with sorted Gaussian scores (no locality in the gather: the unfavourable case for both arms).
The two arms are INTERLEAVED on one device (A B A B ...), device events around each, after a warm-up; prints one JSON line per size with
both medians, min / max, the bytes the composition holds per chunk (gathered rows + similarity matrices; the fused call holds none) and
the share of rows on which the two agree (the bmm accumulates in another order: near-ties may take another path).
The bmm writes fp32 directly (out_dtype=torch.float32); a torch without that overload falls back to a bf16 result cast to fp32, which the
output line then names (gemm = "bf16+cast").
Also timed, because the longer candidate list is part of what the option costs: ltg_topk over the same 20 000 rows of Gaussian logits at
k = candidates against k = 100, in the Recommender's chunks (logits of at most 2 GiB)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from ltgan import _cabi as cabi
    from ltgan.trainer import eval_chunk_rows
    lib = cabi.load()
    n, c, k, lam = 20000, 200, 100, 0.5
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    uc = int(sys.argv[2]) if len(sys.argv) > 2 else 2000            # users per chunk of the composition
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
        del W
        sc = torch.randn(n, c, device=dev, generator=g).sort(dim=1, descending=True).values.contiguous()
        ids = torch.cat([torch.rand(min(2000, n - lo), I, device=dev, generator=g).topk(c, dim=1).indices for lo in range(0, n, 2000)])
        ids = ids.to(torch.int32).contiguous()                       # distinct random ids per row
        so = torch.empty(n, k, dtype=torch.float32, device=dev)
        io = torch.empty(n, k, dtype=torch.int32, device=dev)
        stat = torch.empty(n, 2, dtype=torch.float32, device=dev)

        def fused():
            cabi.check(lib.ltg_topk_diversify(img.data_ptr(), 0, I, n, c, sc.data_ptr(), ids.data_ptr(), lam, k, so.data_ptr(), io.data_ptr(),
                                              stat.data_ptr(), st()), "ltg_topk_diversify")

        def fused_nostat():
            cabi.check(lib.ltg_topk_diversify(img.data_ptr(), 0, I, n, c, sc.data_ptr(), ids.data_ptr(), lam, k, so.data_ptr(), io.data_ptr(),
                                              None, st()), "ltg_topk_diversify")

        tb = img.view(torch.bfloat16)
        try:
            torch.bmm(tb[:2, :8].reshape(1, 2, 8), tb[:2, :8].reshape(1, 2, 8).transpose(1, 2), out_dtype=torch.float32)
            gemm, bmm = "fp32-out", (lambda a: torch.bmm(a, a.transpose(1, 2), out_dtype=torch.float32))
        except (TypeError, RuntimeError):
            gemm, bmm = "bf16+cast", (lambda a: torch.bmm(a, a.transpose(1, 2)).float())
        bi = torch.empty(n, k, dtype=torch.int32, device=dev)
        ar = torch.arange(uc, device=dev)

        def composed():
            for lo in range(0, n, uc):
                hi = min(n, lo + uc)
                m_ = hi - lo
                rows = tb.index_select(0, ids[lo:hi].reshape(-1).long()).view(m_, c, 608)
                S = bmm(rows)                                        # [m_, c, c] fp32
                s = sc[lo:hi]
                rel = (s - s[:, -1:]) / (s[:, :1] - s[:, -1:])
                lrel = lam * rel
                taken = torch.zeros(m_, c, dtype=torch.bool, device=dev)
                p = torch.zeros(m_, dtype=torch.long, device=dev)
                picks = torch.empty(m_, k, dtype=torch.long, device=dev)
                mx = None
                for r in range(k):
                    if r > 0:
                        obj = lrel - (1.0 - lam) * mx
                        p = obj.masked_fill(taken, -float("inf")).argmax(dim=1)
                    picks[:, r] = p
                    taken[ar[:m_], p] = True
                    col = S[ar[:m_], :, p]
                    mx = col if r == 0 else torch.maximum(mx, col)
                bi[lo:hi] = ids[lo:hi].gather(1, picks).to(torch.int32)

        # ltg_topk at k = candidates against k = 100, over the same rows in the Recommender's chunks
        chunk = min(n, eval_chunk_rows(I))
        logits = torch.randn(chunk, I, device=dev, generator=g)
        ts, ti = torch.empty(chunk, c, dtype=torch.float32, device=dev), torch.empty(chunk, c, dtype=torch.int32, device=dev)

        def topk_at(kk):
            def run():
                for lo in range(0, n, chunk):
                    m_ = min(n, lo + chunk) - lo
                    cabi.check(lib.ltg_topk(C.byref(cfg), logits.data_ptr(), None, m_, kk, ts.data_ptr(), ti.data_ptr(), st()), "ltg_topk")
            return run

        arms = (("fused", fused), ("composed", composed), ("fused_nostat", fused_nostat), ("topk_c", topk_at(c)), ("topk_k", topk_at(k)))
        for _ in range(2):
            for _, fn in arms:
                fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = {name: [] for name, _ in arms}
        for _ in range(reps):                      # interleaved: the arms see the same clocks and the same neighbours on the device
            for name, fn in arms:
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1e3)
        same = float((io == bi).all(1).float().mean())
        out = dict(I=I, rows=n, candidates=c, k=k, lam=lam, reps=reps, gemm=gemm, composed_chunk_users=uc,
                   composed_bytes_per_chunk=uc * c * 608 * 2 + uc * c * c * 4, fused_workspace_bytes=0, rows_identical=round(same, 4),
                   ils_before=round(float(stat[:, 0].mean()), 6), ils_after=round(float(stat[:, 1].mean()), 6), topk_chunk_rows=chunk)
        for name, v in t.items():
            out[name + "_us_median"] = round(float(np.median(v)), 1)
            out[name + "_us_min"] = round(float(min(v)), 1)
            out[name + "_us_max"] = round(float(max(v)), 1)
        out["fused_over_composed"] = round(out["fused_us_median"] / out["composed_us_median"], 3)
        print(json.dumps(out), flush=True)
        del logits, img, tb


if __name__ == "__main__":
    main()
