"""The long-tail report on the GPU: ltg_topk_metrics on injected lists against numpy (valid flags and item_hits exactly, the metrics
against the oracle's NDCG / Recall on the group-filtered held-out matrix), bit equality with ltg_rank_metrics on tied logits and on the
logits of a real forward, accumulation of item_hits, the item-sharded report (tests/dist_longtail_worker.py) and longtail.py against
test.py in fresh child processes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import ltg_oracle as O
from serving_harness import DEV, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu

# users with at least one held-out item of the group, Askubuntu_Sample's test split (tests/test_longtail_cpu.py derives them)
USERS_NICHE = {"popular": 9081, "niche": 7835, "all": 10000}
USERS_POP4 = {"pop0": 9737, "pop1": 4172, "pop2": 2563, "pop3": 1823, "all": 10000}


def _csr_dev(rows):
    """list of ascending id arrays -> (ltg_batch, tensors to keep alive)"""
    from ltgan import _cabi as cabi
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows]) if ptr[-1] else np.zeros(1, np.int32)
    p, i = _t(ptr), _t(idx)
    return cabi.ltg_batch(len(rows), 0, p.data_ptr(), i.data_ptr()), (p, i)


def _metrics_dev(ids, held_rows, labels, n_groups, cut, hits=None, with_hits=True):
    """ltg_topk_metrics through the C ABI -> (out [n, n_groups + 1, 4], item_hits or None) host arrays"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, k_in = ids.shape
    idt = ids if isinstance(ids, torch.Tensor) else _t(ids.astype(np.int32))
    te, keep = _csr_dev(held_rows)
    lab = _t(labels.astype(np.uint8))
    out = torch.full((n, n_groups + 1, 4), -7.0, dtype=torch.float32, device=DEV)
    h = None
    if with_hits:
        h = _t(hits.astype(np.int32)) if hits is not None else torch.zeros(len(labels), dtype=torch.int32, device=DEV)
    rc = lib.ltg_topk_metrics(idt.data_ptr(), n, k_in, C.byref(te), lab.data_ptr(), len(labels), n_groups, cut[0], cut[1], cut[2], cut[3],
                              out.data_ptr(), h.data_ptr() if h is not None else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), (h.cpu().numpy() if h is not None else None)


def _numpy_report(ids, held_rows, labels, n_groups, cut):
    """the contract restated directly: rank(h) = position of h in the list; float64"""
    n, k_in = ids.shape
    k_ndcg, k_r1, k_r2, k_exp = cut
    out = np.zeros((n, n_groups + 1, 4))
    hits = np.zeros(len(labels), np.int64)
    for u in range(n):
        pos = {int(i): j for j, i in enumerate(ids[u]) if i >= 0}
        for i in ids[u, :k_exp]:
            if 0 <= i < len(labels):
                hits[i] += 1
        for s in range(n_groups + 1):
            H = [int(h) for h in held_rows[u] if s == n_groups or labels[h] == s]
            if not H:
                continue
            ranks = [pos.get(h, 1 << 30) for h in H]
            dcg = sum(1.0 / np.log2(r + 2.0) for r in ranks if r < k_ndcg)
            idcg = sum(1.0 / np.log2(r + 2.0) for r in range(min(len(H), k_ndcg)))
            out[u, s] = [dcg / idcg, sum(r < k_r1 for r in ranks) / min(k_r1, len(H)), sum(r < k_r2 for r in ranks) / min(k_r2, len(H)), 1.0]
    return out, hits


def _injected(rng, I, k_in, n_groups):
    """lists, held-out rows, labels and the masked score matrix whose ranking the lists are (for the oracle).
    A row with padding stands for a user with fewer than k_in eligible items: every item outside its list is a fold-in item, so its
    held-out items (disjoint from the fold-in) all come from the list."""
    n = 14
    labels = rng.integers(0, n_groups, I).astype(np.uint8)
    stray = rng.random(I) < 0.15
    labels[stray] = rng.choice(np.array([n_groups, 9, 255], np.uint8), int(stray.sum()))      # labels >= n_groups: in no group
    ids = np.full((n, k_in), -1, np.int32)
    pred = np.full((n, I), -np.inf, np.float32)
    held = []
    for u in range(n):
        n_list = k_in
        if u in (2, 9):
            n_list = max(0, k_in // 3)                                                          # padded rows (u = 2 at k_in = 1: empty)
        lst = rng.choice(I, n_list, replace=False).astype(np.int32)
        ids[u, :n_list] = lst
        pred[u, lst] = np.arange(n_list, 0, -1, dtype=np.float32) + 5.0
        rest = np.setdiff1d(np.arange(I), lst)
        if n_list == k_in:
            pred[u, rest] = rng.random(len(rest)).astype(np.float32)                            # everything else ranks behind the list
        if u == 3:
            h = np.zeros(0, np.int64)                                                           # no held-out items
        elif n_list < k_in:
            h = rng.choice(lst, min(len(lst), 4), replace=False) if n_list else np.zeros(0, np.int64)
        elif u == 5:
            h = rng.choice(I, k_in + 37, replace=False)                                        # more held-out items than k_in
            h[: k_in // 2 + 1] = lst[: k_in // 2 + 1]
        elif u == 6:
            h = rng.choice(rest, 9, replace=False)                                              # nothing of it is in the list
        elif u == 7 and n_groups > 1:                                                           # group 0 empty for this user, others not
            cand = np.nonzero(labels != 0)[0]
            h = np.concatenate([np.intersect1d(cand, lst)[:3], rng.choice(np.setdiff1d(cand, lst), 4, replace=False)])
        else:
            h = np.concatenate([rng.choice(lst, min(k_in, int(rng.integers(1, 6))), replace=False), rng.choice(rest, int(rng.integers(0, 5)), replace=False)])
        held.append(np.unique(h).astype(np.int64))
    return ids, held, labels, pred


@pytest.mark.parametrize("n_groups", [1, 2, 8])
@pytest.mark.parametrize("k_in", [1, 20, 100, 1024])
def test_injected_lists_match_numpy_and_the_oracle(k_in, n_groups):
    I = 3000
    rng = np.random.default_rng(1000 * k_in + n_groups)
    ids, held, labels, pred = _injected(rng, I, k_in, n_groups)
    cut = (min(100, k_in), min(20, k_in), min(50, k_in), max(1, (2 * k_in) // 3))
    out, hits = _metrics_dev(ids, held, labels, n_groups, cut)
    want, want_hits = _numpy_report(ids, held, labels, n_groups, cut)
    assert np.array_equal(hits, want_hits)                                                      # exactly
    assert np.array_equal(out[:, :, 3], want[:, :, 3])                                          # exactly
    assert out[3, :, 3].sum() == 0 and np.all(out[3] == 0)
    if n_groups > 1:
        assert want[7, 0, 3] == 0 and want[7, 1:, 3].sum() > 0
    np.testing.assert_allclose(out[:, :, :3], want[:, :, :3], rtol=2e-6, atol=1e-7)
    # the oracle on the held-out matrix with the columns outside the group zeroed
    H = np.zeros((len(held), I), bool)
    for u, h in enumerate(held):
        H[u, h] = True
    for s in range(n_groups + 1):
        Hs = H if s == n_groups else H & (labels == s)[None, :]
        ok = out[:, s, 3] > 0
        nd = O.ndcg_binary_at_k(pred, Hs, cut[0])
        assert ok.sum() == len(nd) == int((Hs.sum(1) > 0).sum())
        print("k_in=%d n_groups=%d slot=%d users=%d max|ndcg - oracle|=%.3g" % (k_in, n_groups, s, len(nd),
              np.abs(out[ok, s, 0] - nd).max() if len(nd) else 0.0))
        np.testing.assert_allclose(out[ok, s, 0], nd, rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(out[ok, s, 1], O.recall_at_k(pred, Hs, cut[1]), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(out[ok, s, 2], O.recall_at_k(pred, Hs, cut[2]), rtol=2e-6, atol=1e-7)


def test_out_of_range_ids_are_not_indices():
    """a list id or a held-out id outside [0, n_items_global) other than the padding is never used as an index"""
    I, k_in = 500, 20
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 2, I).astype(np.uint8)
    ids = np.stack([rng.choice(I, k_in, replace=False) for _ in range(3)]).astype(np.int32)
    ids[0, 4], ids[1, 0], ids[2, 7] = I, 2 ** 31 - 1, -5
    held = [np.array([int(ids[0, 1]), I + 3]), np.array([int(ids[1, 2])]), np.array([int(ids[2, 3])])]
    cut = (20, 20, 20, 20)
    out, hits = _metrics_dev(ids, [np.sort(h) for h in held], labels, 2, cut)
    ok = (ids >= 0) & (ids < I)
    assert np.array_equal(hits, np.bincount(ids[ok], minlength=I))
    assert out[0, 2, 3] == 1 and out[0, 2, 1] == 0.5                                            # the stray held-out id counts in "all", in no group
    assert out[0, :2, 3].sum() == 1


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _rank_metrics_dev(eng, logits, tr_rows, te_rows, cut):
    import torch
    from ltgan import _cabi as cabi
    n = logits.shape[0]
    tr, k1 = _csr_dev(tr_rows)
    te, k2 = _csr_dev(te_rows)
    out = torch.zeros(n, 4, dtype=torch.float32, device=DEV)
    rc = eng.lib.ltg_rank_metrics(C.byref(eng.cfg), logits.data_ptr(), C.byref(tr), C.byref(te), cut[0], cut[1], cut[2], out.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_bit_equal(eng, logits, tr_rows, te_rows, labels, n_groups, k, cut):
    """ltg_topk -> ltg_topk_metrics == ltg_rank_metrics (all) and == ltg_rank_metrics on the filtered held-out CSR (slot g), raw words"""
    import torch
    n = logits.shape[0]
    tr, keep = _csr_dev(tr_rows)
    s = torch.empty(n, k, dtype=torch.float32, device=DEV)
    i = torch.empty(n, k, dtype=torch.int32, device=DEV)
    rc = eng.lib.ltg_topk(C.byref(eng.cfg), logits.data_ptr(), C.byref(tr), n, k, s.data_ptr(), i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    out, _ = _metrics_dev(i, te_rows, labels, n_groups, cut)
    want = _rank_metrics_dev(eng, logits, tr_rows, te_rows, cut)
    assert np.array_equal(_bits(out[:, n_groups]), _bits(want)), "all slot"
    n_valid = [int((want[:, 3] > 0).sum())]
    for g in range(n_groups):
        want_g = _rank_metrics_dev(eng, logits, tr_rows, [h[labels[h] == g] for h in te_rows], cut)
        assert np.array_equal(_bits(out[:, g]), _bits(want_g)), "slot %d" % g
        n_valid.append(int((want_g[:, 3] > 0).sum()))
    return out, n_valid


def test_bit_equal_to_rank_metrics_on_tied_logits():
    import torch
    from ltgan.engine import Engine
    n, I = 64, 1000
    rng = np.random.default_rng(n + I)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="fp32", seed=3)
    pred = rng.random((n, I)).astype(np.float32)
    for c in range(0, I - 1, 17):
        pred[:, c] = pred[:, c + 1]                                    # exact ties (test_rank_metrics_match_oracle's construction)
    held = rng.random((n, I)) < 0.01
    held[3] = False
    tr = rng.random((n, I)) < 0.05
    tr[held] = False
    tr[1, :] = True; tr[1, :40] = False; held[1] = False; held[1, :5] = True   # fewer than 100 eligible items
    held[7, ::3] = ~tr[7, ::3]                                         # more than 100 held-out items
    rows = lambda m: [np.nonzero(r)[0] for r in m]
    labels = rng.integers(0, 3, I).astype(np.uint8)
    labels[::11] = 200
    out, n_valid = _assert_bit_equal(eng, _t(pred), rows(tr), rows(held), labels, 3, 100, (100, 20, 50, 100))
    assert min(n_valid) > 10 and not out[3, :, 3].any() and held[7].sum() > 100
    out8, _ = _assert_bit_equal(eng, _t(pred), rows(tr), rows(held), rng.integers(0, 8, I).astype(np.uint8), 8, 128, (100, 20, 50, 128))
    assert np.array_equal(_bits(out8[:, 8]), _bits(out[:, 3]))         # a longer list changes nothing below the cutoffs
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,I", [(64, 1000), (8, 20000), (4, 200000)])
def test_bit_equal_to_rank_metrics_on_forward_logits(n, I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    rng = np.random.default_rng(I)
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    eng.g_p[7].copy_(_t(rng.uniform(1.0, 3.0, I).astype(np.float32)))           # item biases of a trained model's size
    ev = EvalData(X, X, eng.device)
    tr, _ = ev.rows(0, n)
    acts = eng.new_acts(n)
    eng.forward(tr, acts, keep_prob=0.75, is_training=0.0, rng_step=31)
    torch.cuda.synchronize()
    logits = acts.logits[:n]
    assert bool(torch.isfinite(logits).all())
    tr_rows = [X.indices[X.indptr[r]:X.indptr[r + 1]] for r in range(n)]
    top = torch.topk(logits, 60, dim=1).indices.cpu().numpy()                    # held-out items the list will hold, and some it will not
    te_rows = []
    for r in range(n):
        h = np.concatenate([top[r, rng.choice(60, 12, replace=False)], rng.choice(I, 10, replace=False)])
        te_rows.append(np.setdiff1d(np.unique(h), tr_rows[r]))                   # disjoint from the fold-in
    te_rows[n - 1] = np.zeros(0, np.int64)
    labels = rng.integers(0, 4, I).astype(np.uint8)
    out, n_valid = _assert_bit_equal(eng, logits, tr_rows, te_rows, labels, 4, 100, (100, 20, 50, 100))
    assert min(n_valid) >= 1 and out[:, 4, 0].max() > 0 and out[n - 1, 4, 3] == 0


def test_item_hits_accumulate_and_null_hits_leave_out_unchanged():
    I, k_in = 3000, 100
    rng = np.random.default_rng(77)
    ids, held, labels, _ = _injected(rng, I, k_in, 2)
    cut = (100, 20, 50, 30)
    out1, h1 = _metrics_dev(ids, held, labels, 2, cut)
    out2, h2 = _metrics_dev(ids[::-1].copy(), held[::-1], labels, 2, cut, hits=h1)
    assert np.array_equal(h2, 2 * h1) and h1.sum() == (ids[:, :30] >= 0).sum()
    assert np.array_equal(_bits(out2), _bits(out1[::-1]))
    out3, h3 = _metrics_dev(ids, held, labels, 2, cut, with_hits=False)
    assert h3 is None and np.array_equal(_bits(out3), _bits(out1))


def test_recommender_with_report_is_evaluator_plus_recommender():
    """the optional report changes nothing the classes did before, and its all slot is Evaluator's table bit for bit"""
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Evaluator, LongTailReport, Recommender
    I, n = 1000, 300
    rng = np.random.default_rng(4)
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    T = Hh.random_history(rng, n, I, mean_nnz=6)
    T = T - T.multiply(X)
    T.eliminate_zeros()
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, T, eng.device)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    e = Evaluator(eng, ev, chunk=128)
    m = e.run(rng_step=77)
    ids0, sc0 = Recommender(eng, ev, k=100, chunk=128).run(rng_step=77)
    rep = LongTailReport(labels, 3, k_exp=40)
    ids1, sc1 = Recommender(eng, ev, k=100, chunk=128, report=rep).run(rng_step=77)
    assert np.array_equal(ids0, ids1) and np.array_equal(_bits(sc0), _bits(sc1))
    out, hits = rep.table()
    assert np.array_equal(_bits(out[:, 3]), _bits(e.out.cpu().numpy()))
    assert np.array_equal(hits, np.bincount(ids1[:, :40].ravel(), minlength=I))
    from ltgan import longtail as lt
    r = lt.aggregate(out, hits, labels, ["a", "b", "c"], 40)
    assert (r["all"]["ndcg"], r["all"]["recall20"], r["all"]["recall50"], r["all"]["users"]) == (m["ndcg"], m["recall20"], m["recall50"], m["n_users"])
    ids2, _ = Recommender(eng, ev, k=100, chunk=128, report=rep).run(rng_step=77)     # a second run starts item_hits from zero
    assert np.array_equal(rep.table()[1], hits)
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=30, chunk=128, report=LongTailReport(labels, 3))
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_report(world):
    # differences seen between the sharded and the unsharded report (one MI355X, gloo, custom:1001, 230 users; the worker prints them
    # as SEEN ...): 0 in every column at 2 and at 3 ranks.  A record; the bound is the 3e-3 of test_gpu_cli.py.
    run_ranks("dist_longtail_worker.py", ["custom:1001", "230"], world, "LONGTAIL_SHARDED_OK world=%d" % world)


def _parse(lines):
    """longtail.py's stdout lines -> (first line, {name: fields}) ; the report lines are the ones after the NDCG line"""
    at = max(i for i, l in enumerate(lines) if len(l.split("\t")) == 3)
    rows = {}
    for l in lines[at + 1:]:
        f = l.split("\t")
        rows[f[0]] = f
    return lines[at], rows


def _check_report(lines, json_path, users, k):
    first, rows = _parse(lines)
    assert list(rows) == list(users), rows.keys()
    rep = json.load(open(json_path))
    assert rep["k"] == k
    share = 0.0
    for name, f in rows.items():
        assert len(f) == (9 if name == "all" else 8)
        assert int(f[2]) == users[name], (name, f[2], users[name])
        for x in f[3:6]:
            assert 0.0 <= float(x) <= 1.0
        assert 0.0 < float(f[7]) <= 1.0, (name, f[7])                                    # coverage
        j = rep["all"] if name == "all" else [g for g in rep["groups"] if g["name"] == name][0]
        assert (int(f[1]), int(f[2])) == (j["items"], j["users"])
        got = [float(x) for x in f[3:]]
        want = [j["ndcg"], j["recall20"], j["recall50"], j["share"], j["coverage"]] + ([j["gini"]] if name == "all" else [])
        assert np.allclose(got, want, rtol=0, atol=1e-6), (name, got, want)
        if name != "all":
            share += j["share"]
    assert abs(share - 1.0) < 1e-9 and float(rows["all"][6]) == 1.0 and 0.0 <= float(rows["all"][8]) < 1.0
    assert sum(int(f[1]) for n_, f in rows.items() if n_ != "all") == int(rows["all"][1]) == 1000
    a = rep["all"]
    assert first == str(a["ndcg"]) + "\t" + str(a["recall20"]) + "\t" + str(a["recall50"])
    return first, rows, rep


def test_cli_against_test_py(tmp_path):
    ds, cwd, n_items, _, ck, _, _, _ = askubuntu_run(tmp_path, split=None)
    t_last = run_cli("test.py", [ds, ck], cwd)[-1]
    first, rows, rep = _check_report(run_cli("longtail.py", [ds, ck, "--json", "niche.json"], cwd), os.path.join(cwd, "niche.json"), USERS_NICHE, 100)
    print("test.py    : %r\nlongtail.py: %r" % (t_last, first))
    assert first == t_last                                                # string-equal: one forward, the same bits, from process to process (held on an MI355X)
    assert (int(rows["popular"][1]), int(rows["niche"][1])) == (103, 897)
    first4, rows4, rep4 = _check_report(run_cli("longtail.py", [ds, ck, "--groups", "pop:4", "--k", "20", "--json", "pop4.json"], cwd),
                                        os.path.join(cwd, "pop4.json"), USERS_POP4, 20)
    assert first4 == t_last and [int(rows4["pop%d" % g][1]) for g in range(4)] == [250] * 4
    # two ranks (gloo, one GPU), items sharded: users exact, the means within what test_gpu_cli.py allows between sharded and unsharded.
    # Seen on one MI355X (a record, not a bound): NDCG@100 differs by 2.1e-7 (popular), 5.7e-8 (niche), 8.5e-8 (all); both recalls by 0.
    _, rows2, rep2 = _check_report(run_cli("longtail.py", [ds, ck, "--json", "niche2.json"], cwd, world=2), os.path.join(cwd, "niche2.json"),
                                   USERS_NICHE, 100)
    for name in rows:
        d = [abs(float(a) - float(b)) for a, b in zip(rows[name][3:6], rows2[name][3:6])]
        print("sharded - unsharded, %s: %s" % (name, d))
        assert rows[name][1:3] == rows2[name][1:3] and max(d) < 3e-3, (name, d)
