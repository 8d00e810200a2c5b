"""List explanations on the GPU (ltg_topk_explain): ids and score bits exactly against numpy on an image whose row products are exact in
fp32 (heavy ties), over histories whose lengths straddle the kernel's block; on a trained engine's cosine image the same ids and score
bits as ltg_item_neighbors over the user's history rows, and every score within the derived accumulation bound of the fp64 products;
Recommender(explain=) against ltg_topk + the entry point called by hand, with and without diversify=; the item-sharded recommender
(tests/dist_explain_worker.py) and recommend.py on Askubuntu_Sample in fresh child processes.  The reference is tests/explain_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest

import explain_ref as E
import neighbors_ref as NR
from serving_harness import DEV, _nbr_dev, _small_engine, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu


def _eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _why_dev(img_d, image_lo, ids, indptr, indices, hist_lo, top, r):
    """ltg_topk_explain through the C ABI: img_d a device int16 image, ids / indptr / indices host arrays -> host (scores, ids)"""
    import torch
    from ltgan import _cabi as cabi
    from ltgan.engine import CsrRows
    lib = cabi.load()
    n, k_in = ids.shape
    i_d = _t(np.asarray(ids, np.int32))
    tr = CsrRows(_t(np.asarray(indptr, np.int32)), _t(np.asarray(indices, np.int32)), 0, n)
    so = torch.full((n, top, r), 7.0, dtype=torch.float32, device=DEV)
    io = torch.full((n, top, r), -7, dtype=torch.int32, device=DEV)
    rc = lib.ltg_topk_explain(img_d.data_ptr(), image_lo, int(img_d.shape[0]), C.byref(tr.c), hist_lo, n, k_in, i_d.data_ptr(), top, r,
                              so.data_ptr(), io.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), io.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. exact parity
@pytest.fixture(scope="module")
def exact():
    img = E.exact_image()
    return img, _t(img.view(np.int16))


@pytest.mark.parametrize("image_lo", [0, 13])
@pytest.mark.parametrize("case", range(len(E.EXACT_CASES)))
def test_exact_parity_with_numpy(exact, case, image_lo):
    """every product and partial sum is exact in fp32: ids and score bits equal numpy's, twice in a row, wherever the history's base is"""
    img, img_d = exact
    k_in, top, r = E.EXACT_CASES[case]
    ids, indptr, indices = E.exact_inputs(k_in, top, r, img.shape[0], image_lo)
    assert ids.shape[0] == 37 and set(E.history_lengths(r)) <= set(np.diff(indptr).tolist())
    wS, wI = E.explain_lists(img, image_lo, ids, indptr, indices, 0, top, r)
    gS, gI = _why_dev(img_d, image_lo, ids, indptr, indices, 0, top, r)
    bad = np.nonzero((gI != wI).any((1, 2)))[0]
    assert bad.size == 0, (k_in, top, r, bad[:5], gI[bad[:1]], wI[bad[:1]])
    assert _eq(gS, wS), (k_in, top, r)
    assert (gI[E.ROW_EMPTY] == -1).all() and (gI[E.ROW_MINUS1, top // 2] == -1).all() and (gI[E.ROW_STRAY, min(1, top - 1)] == -1).all()
    if top > 2:
        assert (gI[E.ROW_MINUS1, top // 2 + 1:, 0] >= 0).all()           # the entries behind a padding are still explained
    gS2, gI2 = _why_dev(img_d, image_lo, ids, indptr, indices, 0, top, r)
    assert np.array_equal(gI2, gI) and _eq(gS2, gS)
    gS7, gI7 = _why_dev(img_d, image_lo, ids, indptr, indices - 7, 7, top, r)
    assert np.array_equal(gI7, gI) and _eq(gS7, gS)


# ---------------------------------------------------------------------------------------------- 2. ltg_item_neighbors' scores
@pytest.fixture(scope="module")
def real_lists():
    """the cosine image of an engine at I = 1 001 after a few G steps, 48 users' histories and their ltg_topk lists of forward logits"""
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    rng = np.random.default_rng(21)
    eng = _small_engine(I=1001, steps=3)
    img_d = eng.item_pack("decoder", "cosine")
    X = Hh.random_history(rng, 48, 1001, mean_nnz=12).tocsr()
    X.sort_indices()
    ev = EvalData(X, X, eng.device)
    tr, _ = ev.rows(0, 48)
    acts = eng.new_acts(48)
    eng.forward(tr, acts, keep_prob=1.0, is_training=0.0, rng_step=5)
    s_d = torch.empty(48, 100, dtype=torch.float32, device=eng.device)
    i_d = torch.empty(48, 100, dtype=torch.int32, device=eng.device)
    eng.topk(acts, tr, 100, s_d, i_d)
    torch.cuda.synchronize()
    return img_d.cpu().numpy().view(np.uint16), img_d, i_d.cpu().numpy(), X.indptr.astype(np.int32), X.indices.astype(np.int32)


def test_same_scores_as_item_neighbors(real_lists):
    img, img_d, ids, indptr, indices = real_lists
    top, r = 100, 3
    gS, gI = _why_dev(img_d, 0, ids, indptr, indices, 0, top, r)
    lens = np.diff(indptr)
    users = [int(u) for u in np.argsort(-lens, kind="stable")[[0, 5, 20, 40]] if lens[u] > 0]
    assert len(users) == 4
    for u in users:
        h = indices[indptr[u]:indptr[u + 1]].astype(np.int64)
        nS, nP = _nbr_dev(img_d[_t(h)].contiguous(), img_d[_t(ids[u, :top].astype(np.int64))].contiguous(), np.full(top, -1, np.int32), r)
        nI = np.where(nP >= 0, h[np.maximum(nP, 0)], -1)
        assert np.array_equal(gI[u], nI), u                              # (a list never holds a fold-in item: nothing to exclude)
        assert _eq(gS[u], nS), u
    worst = 0.0
    for u in range(ids.shape[0]):
        h = indices[indptr[u]:indptr[u + 1]].astype(np.int64)
        if h.size == 0:
            assert (gI[u] == -1).all() and np.isneginf(gS[u]).all()
            continue
        q = img[ids[u, :top].astype(np.int64)]
        S64, bound = NR.scores64(q, img[h]), NR.score_bound(q, img[h])
        pos = np.searchsorted(h, gI[u])                                  # [top, r] positions in h (padding: clipped below)
        valid = gI[u] >= 0
        assert (valid.sum(1) == min(r, h.size)).all() and (h[np.minimum(pos, h.size - 1)][valid] == gI[u][valid]).all()
        pos = np.minimum(pos, h.size - 1)
        err = np.abs(gS[u].astype(np.float64) - np.take_along_axis(S64, pos, 1))
        assert (err[valid] <= np.take_along_axis(bound, pos, 1)[valid]).all(), u
        worst = max(worst, float(err[valid].max()))
        if h.size > r:
            kept = np.zeros(S64.shape, bool)
            np.put_along_axis(kept, pos, True, 1)
            last = np.take_along_axis(S64, pos, 1).min(1)
            left = np.where(kept, -np.inf, S64).max(1)
            assert (last >= left - 2.0 * bound.max(1)).all(), u
    print("largest |score - fp64 product| %.3e" % worst)


# ---------------------------------------------------------------------------------------------- 3. the host layer
@pytest.mark.parametrize("I", [1001, 1537])
def test_recommender_with_explain(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Diversify, Explain, Recommender
    rng = np.random.default_rng(I)
    n, k, top, r = 300, 100, 20, 3
    X = Hh.random_history(rng, n, I, mean_nnz=15).tocsr()
    X.sort_indices()
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=1.0)
    why = Explain(r, top=top)
    rec = Recommender(eng, ev, k=k, chunk=128, explain=why)
    ids, sc = rec.run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids, plain_ids) and _eq(sc, plain_sc)          # explaining changes no list
    wI, wS = why.table()
    assert wI.shape == wS.shape == (n, top, r) and wI.dtype == np.int32 and wS.dtype == np.float32
    # by hand on the short last chunk, whose logits are still in the activations: ltg_topk, then the entry point
    tr, _ = ev.rows(256, n)
    m = n - 256
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    l_s, l_i, h_s, h_i = new(m, k), new(m, k, dt=torch.int32), new(m, top, r), new(m, top, r, dt=torch.int32)
    image = eng.item_pack("decoder", "cosine")
    eng.topk(rec.acts, tr, k, l_s, l_i)
    eng.topk_explain(image, 0, tr, l_i, top, r, h_s, h_i)
    torch.cuda.synchronize()
    assert np.array_equal(wI[256:], h_i.cpu().numpy()) and _eq(wS[256:], h_s.cpu().numpy())

    def check_reasons(lists, tab):
        for u in range(n):
            h = X.indices[X.indptr[u]:X.indptr[u + 1]]
            got = tab[u]
            assert np.isin(got[got >= 0], h).all(), u                    # every reason is a fold-in item of the user
            assert (got != lists[u, :top, None]).all(), u                # ... and never the entry itself
            assert ((got >= 0).sum(1) == min(r, h.size)).all(), u        # (a list holds no fold-in item: every history item is a candidate)
    check_reasons(ids, wI)
    assert (np.diff(wS, axis=2)[wI[:, :, 1:] >= 0] <= 0).all()           # best first
    # with diversify= at the same space / metric: the explanations are those of the diversified lists, the image is packed once
    calls = []
    pack = eng.item_pack
    eng.item_pack = lambda *a, **kw: (calls.append(a), pack(*a, **kw))[1]
    why_d = Explain(r, top=top)
    rec_d = Recommender(eng, ev, k=k, chunk=128, diversify=Diversify(0.3, candidates=200), explain=why_d)
    ids_d, _ = rec_d.run(rng_step=77, keep_prob=1.0)
    assert len(calls) == 1, calls
    other = Explain(r, top=top, metric="dot")                            # another image: packed on its own
    Recommender(eng, ev, k=k, chunk=128, diversify=Diversify(0.3, candidates=200), explain=other).run(rng_step=77, keep_prob=1.0)
    assert len(calls) == 3 and other.image is not why_d.image
    eng.item_pack = pack
    dI, dS = why_d.table()
    assert not np.array_equal(ids_d, ids)
    check_reasons(ids_d, dI)
    ids_dev = _t(ids_d)
    for lo in range(0, n, 128):
        hi = min(n, lo + 128)
        a_s, a_i = new(hi - lo, top, r), new(hi - lo, top, r, dt=torch.int32)
        eng.topk_explain(image, 0, ev.rows(lo, hi)[0], ids_dev[lo:hi], top, r, a_s, a_i)
        assert np.array_equal(dI[lo:hi], a_i.cpu().numpy()) and _eq(dS[lo:hi], a_s.cpu().numpy())
    why2 = Explain(r, top=top)
    Recommender(eng, ev, k=k, chunk=128, explain=why2).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(why2.table()[0], wI) and _eq(why2.table()[1], wS)          # run to run
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. over item shards
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recommender_with_explain(world):
    run_ranks("dist_explain_worker.py", ["1001", "230"], world, "EXPLAIN_SHARDED_OK world=%d" % world)


# ---------------------------------------------------------------------------------------------- 5. the CLI
def test_cli_on_askubuntu(tmp_path):
    import torch
    from ltgan import data_processing as dp
    from ltgan import recommend as rc
    from ltgan.dataset import EvalData
    from ltgan.trainer import Recommender
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    tr = tr.tocsr()

    out = run_cli("recommend.py", [ds, ck, "--explain", "3", "--explain-top", "10", "--why", "why.tsv", "--out", "recs.tsv", "--npz", "recs.npz"], cwd)
    assert out[-2].startswith("users: %d\tniche_share@100: " % tr.shape[0]) and out[-1].startswith("why@10: %d entries, " % (10 * tr.shape[0]))
    recs = [line.split("\t")[1].split(",") for line in open(os.path.join(cwd, "recs.tsv")).read().splitlines()]
    lines = open(os.path.join(cwd, "why.tsv")).read().splitlines()
    assert len(lines) == 10 * tr.shape[0]
    z = np.load(os.path.join(cwd, "recs.npz"))
    assert z["why_ids"].shape == z["why_scores"].shape == (tr.shape[0], 10, 3)
    n_reasons = 0
    for j, line in enumerate(lines):
        u, e = divmod(j, 10)
        uid, sid, why = line.split("\t")
        assert int(uid) == uid0 + u and sid == recs[u][e]
        hist = set(tr.indices[tr.indptr[u]:tr.indptr[u + 1]].tolist())
        pairs = [p.split(":") for p in why.split(",")] if why else []
        assert len(pairs) == min(3, len(hist)), (line, len(hist))
        scores = [float(s) for _, s in pairs]
        assert all(int(h) in hist and int(h) != int(sid) for h, _ in pairs) and scores == sorted(scores, reverse=True), line
        assert [int(h) for h, _ in pairs] == z["why_ids"][u, e][z["why_ids"][u, e] >= 0].tolist()
        n_reasons += len(pairs)
    assert out[-1] == "why@10: %d entries, %d reasons" % (len(lines), n_reasons)
    # without the option: the summary of the plain Recommender as the last line, the same lists, and no why-file
    os.remove(os.path.join(cwd, "why.tsv"))
    plain = run_cli("recommend.py", [ds, ck, "--out", "plain.tsv"], cwd)
    ids, _ = Recommender(eng, EvalData(tr, te, eng.device), k=100).run(rng_step=rc.RNG_STEP)
    _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(ds, "item2id.txt"), os.path.join(ds, "item_list.txt"),
                                               os.path.join(ds, "niche_items.txt"), n_items)
    assert plain[-1] == rc.summary_line(rc.long_tail_summary(ids, niche, n_items, te), 100)
    assert not any(l.startswith("why@") for l in plain) and not os.path.exists(os.path.join(cwd, "why.tsv"))
    assert open(os.path.join(cwd, "plain.tsv")).read() == open(os.path.join(cwd, "recs.tsv")).read()
    torch.cuda.synchronize()
