"""Top-K recommendations on the GPU: ltg_topk against numpy's lexsort bit for bit (injected rows built to break a radix select, and
logits of a real forward), ltg_topk_merge over ragged slabs against ltg_topk on the whole row, agreement of Recommender's ids with
ltg_rank_metrics' Recall@20/50, recommend.py against test.py, and the item-sharded recommender (tests/dist_topk_worker.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIG = """[Long-Tail-GAN]
h0_size = 100
h1_size = 150
h2_size = 250
h3_size = 300
NUM_EPOCH = 8
BATCH_SIZE = 100
DISPLAY_ITER = 50
LEARNING_RATE = 0.0001
to_restore = 0
model_name = LT_GAN
GANLAMBDA = 1.0
"""


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


@pytest.mark.parametrize("I", [1000, 1001, 20000, 25024, 200000])
def test_topk_matches_lexsort_bit_for_bit(I):
    import torch
    dev = "cuda:0"
    rng = np.random.default_rng(I)
    L, folds = _rows(rng, I, 1024)
    Ld = torch.from_numpy(L).to(dev)
    ptr, idx = _csr(folds, dev)
    for k in (1, 20, 100, 1000, 1024):
        S, ID = _topk_dev(Ld, ptr, idx, k)
        wS, wID = _reference(L, folds, k)
        assert np.array_equal(ID, wID), (I, k, np.nonzero((ID != wID).any(1))[0])
        assert _eq(S, wS), (I, k)
        S2, ID2 = _topk_dev(Ld, ptr, idx, k)                         # run to run: the same bits
        assert np.array_equal(ID2, ID) and _eq(S2, S)
        Sn, IDn = _topk_dev(Ld, None, None, k)                       # tr = None: nothing excluded
        wS, wID = _reference(L, None, k)
        assert np.array_equal(IDn, wID) and _eq(Sn, wS), (I, k, "tr=None")


@pytest.mark.parametrize("I", [1000, 25024])
def test_topk_on_forward_logits(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Recommender
    rng = np.random.default_rng(2)
    X = Hh.random_history(rng, 300, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    for kp, k in ((0.75, 100), (1.0, 1000)):
        rec = Recommender(eng, ev, k=k, chunk=128)
        ids, sc = rec.run(rng_step=77, keep_prob=kp)
        L = rec.acts.logits[: ev.n - 256].cpu().numpy()             # the last chunk's logits: rows 256 .. 299
        folds = [X.indices[X.indptr[r]:X.indptr[r + 1]] for r in range(256, ev.n)]
        wS, wID = _reference(L, folds, k)
        assert np.array_equal(ids[256:], wID) and _eq(sc[256:], wS)
        ids2, _ = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=kp)
        assert np.array_equal(ids2, ids)
        if kp == 1.0:                                               # dropout off: the counter does not matter
            assert np.array_equal(Recommender(eng, ev, k=k, chunk=128).run(rng_step=5, keep_prob=1.0)[0], ids)
    torch.cuda.synchronize()


@pytest.mark.parametrize("R", [2, 4, 8])
def test_merge_of_ragged_slabs_equals_the_whole_row(R):
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    dev = "cuda:0"
    I = 25024
    rng = np.random.default_rng(R)
    L, folds = _rows(rng, I, 100)
    cuts = np.sort(rng.choice(np.arange(61, I), R - 1, replace=False))
    cuts[0] = 60                                                    # one slab smaller than k: padded inside the merge
    edges = [0] + cuts.tolist() + [I]
    Ld = torch.from_numpy(L).to(dev)
    ptr, idx = _csr(folds, dev)
    for k in (1, 100, 1024):
        want_s, want_i = _topk_dev(Ld, ptr, idx, k)
        ps, pi = [], []
        for a, b in zip(edges[:-1], edges[1:]):
            sf = [f[(f >= a) & (f < b)] - a for f in folds]
            sp_, si_ = _csr(sf, dev)
            s, i = _topk_dev(Ld[:, a:b].contiguous(), sp_, si_, k, item_lo=a)
            ps.append(s)
            pi.append(i)
        ps = torch.from_numpy(np.stack(ps)).to(dev)
        pi = torch.from_numpy(np.stack(pi)).to(dev)
        n = L.shape[0]
        so = torch.empty(n, k, dtype=torch.float32, device=dev)
        io = torch.empty(n, k, dtype=torch.int32, device=dev)
        rc = lib.ltg_topk_merge(R, n, k, ps.data_ptr(), pi.data_ptr(), k, so.data_ptr(), io.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(io.cpu().numpy(), want_i) and _eq(so.cpu().numpy(), want_s), (R, k)


def _askubuntu(tmp_path):
    from ltgan.dataset import materialize_askubuntu
    ds = str(tmp_path / "Askubuntu_Sample")
    materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), ds)
    cwd = str(tmp_path / "run")
    os.makedirs(cwd)
    open(os.path.join(cwd, "config.ini"), "w").write(CONFIG)
    return ds, cwd


def test_recommender_recall_equals_rank_metrics_and_cli_equals_test_py(tmp_path):
    import torch
    from ltgan import data_processing as dp
    from ltgan.dataset import EvalData, count_items
    from ltgan.generator import generator_VAECF
    from ltgan.test import _Counters
    from ltgan.train import save_checkpoint
    from ltgan.trainer import Evaluator, Recommender
    ds, cwd = _askubuntu(tmp_path)
    n_items = count_items(ds)
    gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
    eng = gen.engine
    ck = os.path.join(cwd, "model_0.pt")
    save_checkpoint(ck, eng, _Counters(), 0)
    tr, te, uid0 = dp.load_tr_te_data(os.path.join(ds, "test_tr.csv"), os.path.join(ds, "test_te.csv"), n_items)
    ev = EvalData(tr, te, eng.device)
    step = 2 * 10 ** 9
    out = Evaluator(eng, ev)
    out.run(rng_step=step)
    o = out.out.cpu().numpy()
    ids, _ = Recommender(eng, ev, k=50).run(rng_step=step)
    eligible = n_items - np.diff(ev.tr_host.indptr)
    assert eligible.min() >= 50
    te_c = ev.te_host
    n_ok = 0
    for r in range(ev.n):
        held = te_c.indices[te_c.indptr[r]:te_c.indptr[r + 1]]
        if held.size == 0:
            assert o[r, 3] == 0
            continue
        n_ok += 1
        r20 = np.isin(ids[r, :20], held).sum() / min(20, held.size)
        r50 = np.isin(ids[r, :50], held).sum() / min(50, held.size)
        assert abs(r20 - o[r, 1]) <= 1e-6 and abs(r50 - o[r, 2]) <= 1e-6, (r, r20, o[r, 1], r50, o[r, 2])
        assert len(set(ids[r].tolist())) == 50
    assert n_ok > 100
    torch.cuda.synchronize()
    # the CLIs, fresh processes: recommend.py's Recall@20 == test.py's on the same checkpoint
    tscript = os.path.join(ROOT, "long-tail-gan_amd", "test.py")
    rscript = os.path.join(ROOT, "long-tail-gan_amd", "recommend.py")
    t = subprocess.run(["timeout", "-k", "10", "600", sys.executable, tscript, ds, ck], cwd=cwd, capture_output=True, text=True, timeout=700)
    assert t.returncode == 0, t.stdout[-2000:] + t.stderr[-4000:]
    r20_test = float(t.stdout.strip().splitlines()[-1].split("\t")[1])
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, rscript, ds, ck, "--out", "recs.tsv", "--npz", "recs.npz"], cwd=cwd,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    f = dict(x.split(": ") for x in last.split("\t"))
    assert abs(float(f["Recall@20"]) - r20_test) <= 1e-6, (last, r20_test)
    assert int(f["users"]) == tr.shape[0] and 0.0 <= float(f["niche_share@100"]) <= 1.0 and 0.0 < float(f["coverage@100"]) <= 1.0
    lines = open(os.path.join(cwd, "recs.tsv")).read().splitlines()
    assert len(lines) == tr.shape[0]
    for n, line in enumerate(lines):
        u, items = line.split("\t")
        items = [int(x) for x in items.split(",")]
        assert int(u) == uid0 + n and len(items) == 100 and len(set(items)) == 100 and min(items) >= 0 and max(items) < n_items
    z = np.load(os.path.join(cwd, "recs.npz"))
    assert z["ids"].shape == (tr.shape[0], 100) and z["scores"].dtype == np.float32
    # two ranks (gloo, one GPU), items sharded: the same table up to near-ties of the all-reduce order
    env = dict(os.environ, LTGAN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "900", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29641", rscript, ds, ck, "--out", "recs2.tsv", "--npz", "recs2.npz"]
    r2 = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=env, timeout=1000)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    f2 = dict(x.split(": ") for x in [l for l in r2.stdout.strip().splitlines() if l.startswith("users: ")][-1].split("\t"))
    assert int(f2["users"]) == tr.shape[0] and abs(float(f2["Recall@20"]) - r20_test) < 3e-3
    z2 = np.load(os.path.join(cwd, "recs2.npz"))
    assert (z2["ids"] == z["ids"]).all(1).mean() > 0.97
    assert len(open(os.path.join(cwd, "recs2.tsv")).read().splitlines()) == tr.shape[0]


@pytest.mark.parametrize("world,workload", [(2, "ml20m"), (4, "ml20m"), (2, "custom:1001")])
def test_sharded_recommender(world, workload):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = ["timeout", "-k", "10", "900", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", "29643", os.path.join(ROOT, "tests", "dist_topk_worker.py"), workload, "230"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1000)      # fresh children only
    assert out.returncode == 0 and ("TOPK_SHARDED_OK world=%d" % world) in out.stdout, out.stdout[-3000:] + out.stderr[-6000:]
