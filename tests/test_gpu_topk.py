"""Top-K recommendations on the GPU: ltg_topk against numpy's lexsort bit for bit (injected rows built to break a radix select, and
logits of a real forward), ltg_topk_merge over ragged slabs against ltg_topk on the whole row, agreement of Recommender's ids with
ltg_rank_metrics' Recall@20/50, recommend.py against test.py, and the item-sharded recommender (tests/dist_topk_worker.py)."""
import os

import numpy as np
import pytest

from serving_harness import askubuntu_run, run_cli, run_ranks
from topk_ref import _csr, _eq, _reference, _rows, _topk_dev

pytestmark = pytest.mark.gpu


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


def test_recommender_recall_equals_rank_metrics_and_cli_equals_test_py(tmp_path):
    import torch
    from ltgan.dataset import EvalData
    from ltgan.trainer import Evaluator, Recommender
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)
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
    r20_test = float(run_cli("test.py", [ds, ck], cwd)[-1].split("\t")[1])
    last = run_cli("recommend.py", [ds, ck, "--out", "recs.tsv", "--npz", "recs.npz"], cwd)[-1]
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
    out2 = run_cli("recommend.py", [ds, ck, "--out", "recs2.tsv", "--npz", "recs2.npz"], cwd, world=2, limit=900)
    f2 = dict(x.split(": ") for x in [l for l in out2 if l.startswith("users: ")][-1].split("\t"))
    assert int(f2["users"]) == tr.shape[0] and abs(float(f2["Recall@20"]) - r20_test) < 3e-3
    z2 = np.load(os.path.join(cwd, "recs2.npz"))
    assert (z2["ids"] == z["ids"]).all(1).mean() > 0.97
    assert len(open(os.path.join(cwd, "recs2.tsv")).read().splitlines()) == tr.shape[0]


@pytest.mark.parametrize("world,workload", [(2, "ml20m"), (4, "ml20m"), (2, "custom:1001")])
def test_sharded_recommender(world, workload):
    run_ranks("dist_topk_worker.py", [workload, "230"], world, "TOPK_SHARDED_OK world=%d" % world)
