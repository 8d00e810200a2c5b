#!/usr/bin/env python3
"""Standalone timing of ltg_topk_explain against the expression a user would write without it, on the same packed image, lists and
histories: per sub-chunk of users index_select of the list rows and of the (padded) history rows, torch.bmm (bf16 operands, fp32
result), a mask for the padding and for the entry itself, torch.topk.  One chunk of 20 000 users at 20 000 items, top = 100, r = 3,
cosine image of Gaussian decoder rows, histories as tests/helpers.random_history gives them at mean_nnz = 30, lists of distinct random
ids (no locality in the gather).  The arms are INTERLEAVED on one device (A B C A B C ...), device events around each, after a warm-up;
the third arm is a device copy of 1 GiB, the box's copy rate.  Prints one JSON line: the medians, min / max, the bytes the fused call
gathers (list rows once per history block + history rows; csrc/ltg_explain.h) and their rate as a share of the copy rate, the bytes the
composition holds per sub-chunk, and the share of entries on which the two agree (the bmm accumulates in another order)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HB = 64                                  # EX_HB of csrc/ltg_explain.h


def main():
    import helpers as Hh
    from ltgan import _cabi as cabi
    from ltgan.engine import CsrRows
    lib = cabi.load()
    n, I, top, r = 20000, 20000, 100, 3
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    uc = int(sys.argv[2]) if len(sys.argv) > 2 else 1000            # users per sub-chunk of the composition
    dev = "cuda:0"
    st = lambda: torch.cuda.current_stream().cuda_stream
    cfg = cabi.ltg_config(I, 600, 200, I, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    g = torch.Generator(device=dev).manual_seed(1)
    W = torch.randn(I, 600, device=dev, generator=g)
    gen = cabi.ltg_gen_state()
    gen.p[3] = W.data_ptr()
    img = torch.empty(I, 608, dtype=torch.int16, device=dev)
    cabi.check(lib.ltg_item_pack(C.byref(cfg), C.byref(gen), 0, 0, img.data_ptr(), st()), "ltg_item_pack")
    torch.cuda.synchronize()
    del W
    X = Hh.random_history(np.random.default_rng(7), n, I, mean_nnz=30).tocsr()
    X.sort_indices()
    lens = np.diff(X.indptr).astype(np.int64)
    indptr = torch.from_numpy(X.indptr.astype(np.int32)).to(dev)
    indices = torch.from_numpy(X.indices.astype(np.int32)).to(dev)
    tr = CsrRows(indptr, indices, 0, n)
    ids = torch.cat([torch.rand(min(2000, n - lo), I, device=dev, generator=g).topk(top, dim=1).indices for lo in range(0, n, 2000)])
    ids = ids.to(torch.int32).contiguous()                           # distinct random ids per row
    so = torch.empty(n, top, r, dtype=torch.float32, device=dev)
    io = torch.empty(n, top, r, dtype=torch.int32, device=dev)

    def fused():
        cabi.check(lib.ltg_topk_explain(img.data_ptr(), 0, I, C.byref(tr.c), 0, n, top, ids.data_ptr(), top, r, so.data_ptr(), io.data_ptr(),
                                        st()), "ltg_topk_explain")

    tb = img.view(torch.bfloat16)
    try:
        torch.bmm(tb[:2, :8].reshape(1, 2, 8), tb[:2, :8].reshape(1, 2, 8).transpose(1, 2), out_dtype=torch.float32)
        gemm, bmm = "fp32-out", (lambda a, b: torch.bmm(a, b.transpose(1, 2), out_dtype=torch.float32))
    except (TypeError, RuntimeError):
        gemm, bmm = "bf16+cast", (lambda a, b: torch.bmm(a, b.transpose(1, 2)).float())
    # the padded histories of every sub-chunk, built once outside the timed region (the composition is given its index tensors for free)
    pads = []
    for lo in range(0, n, uc):
        hi = min(n, lo + uc)
        hmax = max(1, int(lens[lo:hi].max()))
        pad = np.full((hi - lo, hmax), -1, np.int64)
        for u in range(lo, hi):
            pad[u - lo, :lens[u]] = X.indices[X.indptr[u]:X.indptr[u + 1]]
        pads.append(torch.from_numpy(pad).to(dev))
    bi = torch.empty(n, top, r, dtype=torch.int32, device=dev)
    held = 0

    def composed():
        nonlocal held
        for c, lo in enumerate(range(0, n, uc)):
            hi = min(n, lo + uc)
            m_, pad = hi - lo, pads[c]
            hmax = pad.shape[1]
            q = tb.index_select(0, ids[lo:hi].reshape(-1).long()).view(m_, top, 608)
            h = tb.index_select(0, pad.clamp(min=0).reshape(-1)).view(m_, hmax, 608)
            S = bmm(q, h)                                            # [m_, top, hmax] fp32
            bad = (pad < 0)[:, None, :] | (pad[:, None, :] == ids[lo:hi, :, None])
            S = S.masked_fill(bad, -float("inf"))
            kk = min(r, hmax)
            v, p = S.topk(kk, dim=2)
            got = pad[:, None, :].expand(m_, top, hmax).gather(2, p)
            bi[lo:hi, :, :kk] = torch.where(torch.isinf(v), torch.full_like(got, -1), got).to(torch.int32)
            bi[lo:hi, :, kk:] = -1
            held = max(held, m_ * (top + hmax) * 608 * 2 + m_ * top * hmax * 4)

    big = torch.empty(1 << 28, dtype=torch.float32, device=dev)      # 1 GiB
    big2 = torch.empty_like(big)

    def copy():
        big2.copy_(big)

    arms = (("fused", fused), ("composed", composed), ("copy", copy))
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
    same = float((io == bi).all(2).float().mean())
    blocks = (lens + HB - 1) // HB
    gathered = int((blocks * top + lens).sum()) * 1216
    out = dict(I=I, rows=n, top=top, r=r, reps=reps, gemm=gemm, history_mean=round(float(lens.mean()), 2), history_max=int(lens.max()),
               users_over_one_block=int((blocks > 1).sum()), composed_chunk_users=uc, composed_bytes_per_chunk=held,
               fused_workspace_bytes=0, fused_gathered_bytes=gathered, entries_identical=round(same, 4))
    for name, v in t.items():
        out[name + "_us_median"] = round(float(np.median(v)), 1)
        out[name + "_us_min"] = round(float(min(v)), 1)
        out[name + "_us_max"] = round(float(max(v)), 1)
    copy_rate = 2.0 * big.numel() * 4 / (out["copy_us_median"] * 1e-6)            # bytes moved (read + written) per second
    out["copy_TBps"] = round(copy_rate / 1e12, 3)
    out["fused_gather_TBps"] = round(gathered / (out["fused_us_median"] * 1e-6) / 1e12, 3)
    out["fused_share_of_copy_rate"] = round(gathered / (out["fused_us_median"] * 1e-6) / copy_rate, 3)
    out["fused_over_composed"] = round(out["fused_us_median"] / out["composed_us_median"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
