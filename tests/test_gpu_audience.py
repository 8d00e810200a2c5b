"""Item audiences on the GPU: ltg_item_audience against numpy's lexsort bit for bit (injected columns built to break a selection, every
combination of lse / fold-in / query order, one and several row segments), accumulation over ragged chunks through ltg_topk_merge,
Recommender(..., audience=...) on a real forward, audience.py on the Askubuntu fixture, and the item-sharded walk
(tests/dist_audience_worker.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import audience_ref as AR
from serving_harness import askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu

N_SPECIAL = 9          # the injected columns sit at 3, 3 + step, ... so that they fall into different column blocks


def _eq(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _csr(folds, dev):
    import torch
    ptr = np.zeros(len(folds) + 1, np.int32)
    ptr[1:] = np.cumsum([len(f) for f in folds])
    idx = np.concatenate([np.asarray(f, np.int32) for f in folds]) if ptr[-1] else np.zeros(1, np.int32)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _audience_dev(Ld, lse_d, csr, n_rows, row_lo, q_d, k):
    """ltg_item_audience on the first n_rows rows of a [rows, I] device tensor; csr: (indptr, indices) device int32 of LOCAL ids, or None"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    I = Ld.shape[1]
    n_q = int(q_d.numel())
    cfg = cabi.ltg_config(I, 600, 200, I, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    tr = cabi.ltg_batch(n_rows, 0, csr[0].data_ptr(), csr[1].data_ptr()) if csr is not None else None
    need = lib.ltg_item_audience_ws_bytes(C.byref(cfg), n_rows, n_q, k)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=Ld.device)
    s = torch.empty(n_q, k, dtype=torch.float32, device=Ld.device)
    i = torch.empty(n_q, k, dtype=torch.int32, device=Ld.device)
    rc = lib.ltg_item_audience(C.byref(cfg), Ld.data_ptr(), lse_d.data_ptr() if lse_d is not None else None,
                               C.byref(tr) if tr is not None else None, n_rows, row_lo, q_d.data_ptr(), n_q, k, s.data_ptr(), i.data_ptr(),
                               ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), need


def _chunk(rng, n, I):
    """[n, I] logits with the injected columns, lse [n], and per row the ascending LOCAL columns it holds; -> L, lse, folds, special"""
    L = rng.standard_normal((n, I)).astype(np.float32)
    special = 3 + (I // N_SPECIAL) * np.arange(N_SPECIAL)
    L[:, special[1]] = 1.5                                                                  # all equal: row order decides
    L[:, special[2]] = rng.integers(0, 4, n).astype(np.float32) * 0.5                       # four values: ties everywhere
    L[:, special[3]] = rng.choice(np.array([0.0, -0.0, -np.inf, 2.0], np.float32), n, p=[0.4, 0.4, 0.19, 0.01])
    L[:, special[4]] = -np.inf                                                              # nothing but -inf
    L[:, special[5]] = np.round(rng.standard_normal(n) * 20).astype(np.float32) / 4         # duplicates at every level
    lse = (rng.standard_normal(n) * 0.5 + 7.0).astype(np.float32)
    lse[::5] = 0.0                                                                          # (-0.0 - 0.0 = -0.0, 0.0 - 0.0 = +0.0)
    held = rng.random((n, I)) < 0.02
    held[:, special[:6]] |= rng.random((n, 6)) < 0.3                                        # the injected columns lose rows too
    held[:, special[6]] = True                                                              # every row holds it: an all-padding list
    for c, free in ((special[7], 10), (special[8], 128)):                                   # held by all rows but k // 2 (k = 20, 256)
        held[:, c] = True
        held[rng.choice(n, min(n, free), replace=False), c] = False
    folds = [np.nonzero(held[r])[0] for r in range(n)]
    return L, lse, folds, held, special


@pytest.mark.parametrize("I,n_rows", [(I, n) for I in (1000, 1001) for n in (1, 63, 257, 1000)] + [(1001, 2500)])
def test_audience_matches_lexsort_bit_for_bit(I, n_rows):
    import torch
    dev = "cuda:0"
    rng = np.random.default_rng(1000 * I + n_rows)
    L, lse, folds, held, special = _chunk(rng, n_rows, I)
    Ld, lse_d, csr = torch.from_numpy(L).to(dev), torch.from_numpy(lse).to(dev), _csr(folds, dev)
    sub = rng.permutation(np.concatenate([special, rng.choice(I, 40, replace=False)]))
    sub = np.concatenate([sub, sub[:3]]).astype(np.int32)                                  # shuffled, with repeated columns
    few = np.array([special[3], special[0], special[8], special[3], special[5]], np.int32)  # one column block: the rows are cut into segments
    queries = [np.arange(I, dtype=np.int32), sub] + ([few] if n_rows > 1024 else [])
    q_dev = [torch.from_numpy(q).to(dev) for q in queries]
    segmented = False
    for use_lse in (True, False):
        for use_tr in (True, False):
            # one reference per (lse, tr): every column at the longest k; a shorter list is its prefix, a query is its row
            wS, wID = AR.audience_lists(L, lse if use_lse else None, folds if use_tr else None, np.arange(I), 256, held=held if use_tr else None)
            for q, qd in zip(queries, q_dev):
                for k in (1, 20, 256):
                    for row_lo in (0, 5000):
                        S, ID, need = _audience_dev(Ld, lse_d if use_lse else None, csr if use_tr else None, n_rows, row_lo, qd, k)
                        segmented = segmented or need > 0
                        want_id = np.where(wID[q, :k] >= 0, wID[q, :k] + row_lo, -1)
                        what = (I, n_rows, use_lse, use_tr, len(q), k, row_lo)
                        assert np.array_equal(ID, want_id), (what, np.nonzero((ID != want_id).any(1))[0][:8])
                        assert _eq(S, wS[q, :k]), what
                    S2, ID2, _ = _audience_dev(Ld, lse_d if use_lse else None, csr if use_tr else None, n_rows, 5000, qd, k)
                    assert np.array_equal(ID2, ID) and _eq(S2, S), "a second call gives other bits"
    assert segmented == (n_rows > 1024)               # the case with several row segments and their merge is among these
    if n_rows >= 63:
        assert (wID[special[1], :20] == np.arange(20)).all()          # (use_tr False, all equal: the first rows, in order)


def test_audience_accumulates_over_ragged_chunks():
    """three chunks (400, 15, 285 rows: the second shorter than k) through ltg_item_audience + ltg_topk_merge == the reference on all 700"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    dev = "cuda:0"
    I, n = 1001, 700
    rng = np.random.default_rng(7)
    L, lse, folds, held, special = _chunk(rng, n, I)
    Ld, lse_d = torch.from_numpy(L).to(dev), torch.from_numpy(lse).to(dev)
    q = np.arange(I, dtype=np.int32)
    qd = torch.from_numpy(q).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for k in (20, 256):
        pair_s = torch.full((2, I, k), float("-inf"), dtype=torch.float32, device=dev)
        pair_i = torch.full((2, I, k), -1, dtype=torch.int32, device=dev)
        out_s, out_i = torch.empty(I, k, dtype=torch.float32, device=dev), torch.empty(I, k, dtype=torch.int32, device=dev)
        for a, b in ((0, 400), (400, 415), (415, 700)):
            S, ID, _ = _audience_dev(Ld[a:b].contiguous(), lse_d[a:b].contiguous(), _csr(folds[a:b], dev), b - a, a, qd, k)
            pair_s[1].copy_(torch.from_numpy(S))
            pair_i[1].copy_(torch.from_numpy(ID))
            assert lib.ltg_topk_merge(2, I, k, pair_s.data_ptr(), pair_i.data_ptr(), k, out_s.data_ptr(), out_i.data_ptr(), st) == 0
            pair_s[0].copy_(out_s)
            pair_i[0].copy_(out_i)
        torch.cuda.synchronize()
        wS, wID = AR.audience_lists(L, lse, folds, q, k, held=held)
        assert np.array_equal(pair_i[0].cpu().numpy(), wID), k
        assert _eq(pair_s[0].cpu().numpy(), wS), k


def test_audience_on_a_real_forward():
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Audience, Recommender
    I, users, k, chunk, step = 1000, 300, 50, 128, 77
    rng = np.random.default_rng(2)
    X = Hh.random_history(rng, users, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    folds = [X.indices[X.indptr[r]:X.indptr[r + 1]] for r in range(users)]
    items = np.concatenate([rng.permutation(I)[:200], [5, 5]]).astype(np.int32)
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=0, chunk=chunk, audience=Audience([I], k=k))
    acts = eng.new_acts(chunk)
    for kp in (0.75, 1.0):
        L, lse = np.empty((users, I), np.float32), np.empty(users, np.float32)
        for lo in range(0, users, chunk):
            hi = min(users, lo + chunk)
            tr, _ = ev.rows(lo, hi)
            eng.forward(tr, acts, keep_prob=kp, is_training=0.0, rng_step=step + lo)
            torch.cuda.synchronize()
            L[lo:hi] = acts.logits[: hi - lo].cpu().numpy()
            lse[lo:hi] = acts.lse[: hi - lo].cpu().numpy()
        tables = {}
        for score in ("logprob", "logit"):
            aud = Audience(items, k=k, score=score)
            rec = Recommender(eng, ev, k=0, chunk=chunk, audience=aud)
            ids0, sc0 = rec.run(rng_step=step, keep_prob=kp)
            assert ids0.shape == (users, 0) and sc0.shape == (users, 0) and ids0.dtype == np.int32 and sc0.dtype == np.float32
            ids, sc = aud.table()
            wS, wID = AR.audience_lists(L, lse if score == "logprob" else None, folds, items, k)
            assert np.array_equal(ids, wID), (kp, score, np.nonzero((ids != wID).any(1))[0][:8])
            assert _eq(sc, wS), (kp, score)
            rec.run(rng_step=step, keep_prob=kp)                      # a second run starts from empty lists and ends with the same ones
            ids2, sc2 = aud.table()
            assert np.array_equal(ids2, ids) and _eq(sc2, sc)
            tables[score] = (ids, sc)
        # user lists and audiences from one walk: neither changes the other
        aud = Audience(items, k=k)
        u_ids, u_sc = Recommender(eng, ev, k=100, chunk=chunk, audience=aud).run(rng_step=step, keep_prob=kp)
        p_ids, p_sc = Recommender(eng, ev, k=100, chunk=chunk).run(rng_step=step, keep_prob=kp)
        assert np.array_equal(u_ids, p_ids) and _eq(u_sc, p_sc)
        a_ids, a_sc = aud.table()
        assert np.array_equal(a_ids, tables["logprob"][0]) and _eq(a_sc, tables["logprob"][1])
    torch.cuda.synchronize()


def test_audience_cli_on_the_askubuntu_fixture(tmp_path):
    import torch
    from ltgan import data_processing as dp
    ds, cwd, n_items, _, ck, tr, _, uid0 = askubuntu_run(tmp_path)
    torch.cuda.synchronize()
    tr = tr.tocsr()
    _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(ds, "item2id.txt"), os.path.join(ds, "item_list.txt"),
                                               os.path.join(ds, "niche_items.txt"), n_items)
    niche = sorted(int(x) for x in niche)
    users = tr.shape[0]
    out = run_cli("audience.py", [ds, ck, "--items", "niche", "--k", "20", "--npz", "aud.npz"], cwd)
    lines = open(os.path.join(cwd, "audience.tsv")).read().splitlines()
    assert len(lines) == len(niche) > 0
    held = tr.tocsc()
    n_listed = 0
    for sid, line in zip(niche, lines):
        s, _, rest = line.partition("\t")
        uids = [int(x) for x in rest.split(",")] if rest else []
        assert int(s) == sid and len(uids) <= 20 and len(set(uids)) == len(uids)
        assert all(uid0 <= u < uid0 + users for u in uids)
        have = set(held.indices[held.indptr[sid]:held.indptr[sid + 1]].tolist())
        assert not have & {u - uid0 for u in uids}, sid
        assert len(uids) == min(20, users - len(have))
        n_listed += len(uids)
    assert n_listed > 0
    z = np.load(os.path.join(cwd, "aud.npz"))
    assert z["items"].tolist() == niche and z["uids"].shape == (len(niche), 20) and z["scores"].shape == (len(niche), 20)
    assert z["scores"].dtype == np.float32
    f = dict(x.split(": ") for x in out[-1].split("\t"))
    assert int(f["items"]) == len(niche) and int(f["users"]) == users and 0.0 < float(f["user_coverage@20"]) <= 1.0


@pytest.mark.parametrize("world,workload", [(2, "ml20m"), (4, "ml20m"), (2, "custom:1001"), (4, "custom:1001")])
def test_sharded_audience(world, workload):
    """tests/dist_audience_worker.py: bit for bit against the numpy reference on the gathered logits with bf16 and with fp32 decoder operands;
    against the unsharded walk within 1e-5 relative at every position with fp32 operands, where the all-reduce order is the only source of
    difference the bound was derived for (with bf16 operands a rounding of an operand flips here and there: 1.3e-05 at custom:1001, printed
    by the worker, which says where that comes from)"""
    run_ranks("dist_audience_worker.py", [workload, "230"], world, "AUDIENCE_SHARDED_OK world=%d" % world)
