"""The numpy reference of ltg_topk (per row lexsort((ids, -scores)) over the eligible items), the injected rows built to break a radix
select, and ltg_topk called through the C ABI -- shared by tests/test_gpu_topk.py, tests/test_gpu_quota.py and tests/test_quota_cpu.py."""
import ctypes as C

import numpy as np


def _topk_dev(logits, indptr, indices, k, item_lo=0):
    """ltg_topk on a [rows, I] device tensor; indptr / indices: device int32 CSR of LOCAL fold-in ids, or None"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, I = logits.shape
    cfg = cabi.ltg_config(I, 600, 200, I, 100, 150, 250, 300, 0, 0, item_lo, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    tr = None
    if indptr is not None:
        tr = cabi.ltg_batch(n, 0, indptr.data_ptr(), indices.data_ptr() if indices.numel() else indptr.data_ptr())
    s = torch.empty(n, k, dtype=torch.float32, device=logits.device)
    i = torch.empty(n, k, dtype=torch.int32, device=logits.device)
    rc = lib.ltg_topk(C.byref(cfg), logits.data_ptr(), C.byref(tr) if tr is not None else None, n, k, s.data_ptr(), i.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _reference(L, folds, k, item_lo=0):
    """numpy: per row lexsort((ids, -scores)) over the eligible items, padded with -1 / -inf"""
    n, I = L.shape
    S = np.full((n, k), -np.inf, np.float32)
    ID = np.full((n, k), -1, np.int32)
    for r in range(n):
        ok = np.ones(I, bool)
        if folds is not None:
            ok[folds[r]] = False
        loc = np.nonzero(ok)[0]
        sc = L[r, loc]
        o = np.lexsort((loc + item_lo, -sc))[:k]
        S[r, :len(o)] = sc[o]
        ID[r, :len(o)] = loc[o] + item_lo
    return S, ID


def _rows(rng, I, kmax):
    """injected rows and their fold-in lists (LOCAL ids, ascending)"""
    rows, folds = [], []
    rows.append(rng.standard_normal(I).astype(np.float32)); folds.append(np.sort(rng.choice(I, I // 20, replace=False)))
    rows.append(np.full(I, 1.5, np.float32)); folds.append(np.sort(rng.choice(I, 7, replace=False)))             # all equal
    rows.append(rng.integers(0, 4, I).astype(np.float32) * 0.5); folds.append(np.sort(rng.choice(I, 13, replace=False)))   # ties everywhere
    z = rng.choice(np.array([0.0, -0.0, -np.inf, 2.0], np.float32), I, p=[0.4, 0.4, 0.19, 0.01])                # signed zeros, -inf
    rows.append(z.astype(np.float32)); folds.append(np.sort(rng.choice(I, 5, replace=False)))
    rows.append(rng.standard_normal(I).astype(np.float32)); folds.append(np.zeros(0, np.int64))                 # empty fold-in
    keep = max(0, kmax // 2)                                                                                    # fewer than k eligible
    rows.append(rng.standard_normal(I).astype(np.float32)); folds.append(np.sort(rng.choice(I, I - min(I, keep), replace=False)))
    x = np.round(rng.standard_normal(I) * 20).astype(np.float32) / 4                                          # duplicates at every level
    rows.append(x); folds.append(np.sort(rng.choice(I, I // 3, replace=False)))
    rows.append(np.full(I, -np.inf, np.float32)); folds.append(np.sort(rng.choice(I, 3, replace=False)))      # nothing but -inf
    rows.append(rng.standard_normal(I).astype(np.float32)); folds.append(np.arange(I))                          # no eligible item at all
    return np.stack(rows), folds


def _csr(folds, dev):
    import torch
    ptr = np.zeros(len(folds) + 1, np.int32)
    ptr[1:] = np.cumsum([len(f) for f in folds])
    idx = np.concatenate([np.asarray(f, np.int32) for f in folds]) if ptr[-1] else np.zeros(1, np.int32)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _eq(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
