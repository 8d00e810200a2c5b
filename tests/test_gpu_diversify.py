"""Diversified top-K lists on the GPU (ltg_topk_diversify): ids, score bits and both statistics exactly against numpy on an image whose
row products are exact in fp32 (heavy ties); on real-valued tables every pick against the fp64 optimum GIVEN the device's own prefix,
within the derived accumulation bound; Recommender(diversify=) against ltg_topk + the entry point called by hand with a LongTailReport
reading the diversified lists; the item-sharded recommender (tests/dist_diversify_worker.py) and both CLIs on Askubuntu_Sample in fresh
child processes.  The reference is tests/diversify_ref.py.

The second test prints its largest pick shortfall and statistic error per case (pytest -s); DESIGN 5.12 records them."""
import os

import numpy as np
import pytest

import diversify_ref as D
import neighbors_ref as NR
from serving_harness import DEV, _pack_dev, _small_engine, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu


def _eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _div_dev(img_d, image_lo, sc, ids, lam, k, stat=True):
    """ltg_topk_diversify through the C ABI: img_d a device int16 image, sc / ids host lists -> host (scores, ids, stats)"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, c_in = ids.shape
    s_d, i_d = _t(np.asarray(sc, np.float32)), _t(np.asarray(ids, np.int32))
    so = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
    io = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    st = torch.full((n, 2), 7.0, dtype=torch.float32, device=DEV) if stat else None
    rc = lib.ltg_topk_diversify(img_d.data_ptr(), image_lo, int(img_d.shape[0]), n, c_in, s_d.data_ptr(), i_d.data_ptr(), lam, k,
                                so.data_ptr(), io.data_ptr(), st.data_ptr() if stat else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), io.cpu().numpy(), st.cpu().numpy() if stat else None


# ---------------------------------------------------------------------------------------------- 1. exact parity
@pytest.fixture(scope="module")
def exact():
    img = D.exact_image()
    return img, _t(img.view(np.int16))


@pytest.mark.parametrize("case", range(len(D.EXACT_CASES)))
def test_exact_parity_with_numpy(exact, case):
    """every product, partial sum, relevance and objective is exact in fp32: ids, score bits and both statistics equal numpy's"""
    img, img_d = exact
    c_in, k = D.EXACT_CASES[case]
    lo = 13 if case % 2 else 0                                           # (image_lo > 0: row 3's stray id 12 is then a non-negative one)
    sc, ids = D.exact_lists(c_in, k, img.shape[0], image_lo=lo)
    n = D.valid_counts(ids, lo, img.shape[0])
    S = D.exact_similarities(img, ids, lo, n)
    for lam in D.EXACT_LAMBDAS:
        wS, wID, picks = D.mmr_lists(sc, ids, S, k, lam, np.float64, n=n)
        gS, gID, gst = _div_dev(img_d, lo, sc, ids, lam, k)
        bad = np.nonzero((gID != wID).any(1))[0]
        assert bad.size == 0, (c_in, k, lam, bad[:5], gID[bad[:1]], wID[bad[:1]])
        assert _eq(gS, wS), (c_in, k, lam)
        want = np.zeros((len(n), 2), np.float32)
        for r in range(len(n)):
            for col, pos in enumerate((np.arange(min(k, n[r])), picks[r])):
                t, pairs = D.pair_sum(S[r], pos)
                assert t == np.float32(t)                                # (the sum is exact in fp32: one rounding, the division)
                want[r, col] = np.float32(t) / np.float32(pairs) if pairs else 0.0
        assert _eq(gst, want + np.float32(0.0)), (c_in, k, lam, np.nonzero((gst != want).any(1))[0][:5])
        if lam == 1.0:
            assert np.array_equal(gID, np.where(np.arange(k)[None, :] < n[:, None], ids[:, :k], -1))
        gS2, gID2, _ = _div_dev(img_d, lo, sc, ids, lam, k, stat=False)   # stat_out NULL, and twice in a row: the same bits
        assert np.array_equal(gID2, gID) and _eq(gS2, gS)


# ---------------------------------------------------------------------------------------------- 2. near-optimal picks on real tables
def _check_prefix_optimal(img, image_lo, sc, ids, lam, k, got):
    """-> (largest shortfall, largest stat error); asserts the structure exactly and every pick within the tolerance"""
    gS, gID, gst = got
    n = D.valid_counts(ids, image_lo, img.shape[0])
    worst = worst_stat = 0.0
    u = 2.0 ** -24
    for r in range(ids.shape[0]):
        nr, kk = int(n[r]), int(min(k, n[r]))
        assert (gID[r, kk:] == -1).all() and np.isneginf(gS[r, kk:]).all()
        if kk == 0:
            assert (gst[r] == 0).all()
            continue
        pos_of = {int(g): p for p, g in enumerate(ids[r, :nr])}
        assert len(set(gID[r, :kk].tolist())) == kk and all(int(g) in pos_of for g in gID[r, :kk])      # no duplicate, no stranger
        picks = np.array([pos_of[int(g)] for g in gID[r, :kk]])
        assert picks[0] == 0 and _eq(gS[r, :kk], sc[r, picks])
        rows = img[ids[r, :nr].astype(np.int64) - image_lo]
        S64, bound = NR.scores64(rows, rows), NR.score_bound(rows, rows)
        tol = 2.0 * (1.0 - lam) * bound.max() + 4.0 * u * (lam + (1.0 - lam) * np.abs(S64).max())
        short = D.pick_shortfall(sc[r, :nr], S64, picks, lam)
        if short.size:
            worst = max(worst, float(short.max()))
            assert short.max() <= tol, (r, lam, int(short.argmax()) + 1, short.max(), tol)
        for col, pos in enumerate((np.arange(kk), picks)):
            t, pairs = D.pair_sum(S64, pos)
            if pairs == 0:
                assert gst[r, col] == 0
                continue
            gam = pairs * u / (1.0 - pairs * u)
            mean_abs = D.pair_sum(np.abs(S64), pos)[0] / pairs
            err = abs(float(gst[r, col]) - t / pairs)
            worst_stat = max(worst_stat, err)
            assert err <= bound.max() + gam * mean_abs, (r, col, err)
    return worst, worst_stat


@pytest.fixture(scope="module")
def real_tables():
    """(host image uint16, device image, scores, ids, k) per table: the cosine image of an engine at I = 1 001 after a few G steps with
    ltg_topk lists of forward logits (c_in = 200, k = 100), and 2 003 Gaussian rows with Gaussian scores (c_in = 256, k = 256)"""
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    rng = np.random.default_rng(21)
    eng = _small_engine(I=1001, steps=3)
    img_d = eng.item_pack("decoder", "cosine")
    X = Hh.random_history(rng, 48, 1001, mean_nnz=12)
    ev = EvalData(X, X, eng.device)
    tr, _ = ev.rows(0, 48)
    acts = eng.new_acts(48)
    eng.forward(tr, acts, keep_prob=1.0, is_training=0.0, rng_step=5)
    s_d = torch.empty(48, 200, dtype=torch.float32, device=eng.device)
    i_d = torch.empty(48, 200, dtype=torch.int32, device=eng.device)
    eng.topk(acts, tr, 200, s_d, i_d)
    torch.cuda.synchronize()
    out = [(img_d.cpu().numpy().view(np.uint16), img_d, 0, s_d.cpu().numpy(), i_d.cpu().numpy(), 100)]
    W = rng.standard_normal((2003, 600)).astype(np.float32)
    g_d = _pack_dev(W, "cosine")
    sc = -np.sort(-rng.standard_normal((24, 256)).astype(np.float32), axis=1)
    ids = np.stack([7 + rng.choice(2003, 256, replace=False) for _ in range(24)]).astype(np.int32)
    sc[1, 100:], ids[1, 100:] = -np.inf, -1                             # a short row, and an empty one
    sc[2, :], ids[2, :] = -np.inf, -1
    out.append((g_d.cpu().numpy().view(np.uint16), g_d, 7, sc, ids, 256))
    return out


@pytest.mark.parametrize("table", [0, 1])
@pytest.mark.parametrize("lam", [0.3, 0.7])
def test_every_pick_is_near_optimal_given_the_devices_prefix(real_tables, table, lam):
    img, img_d, lo, sc, ids, k = real_tables[table]
    got = _div_dev(img_d, lo, sc, ids, lam, k)
    worst, worst_stat = _check_prefix_optimal(img, lo, sc, ids, lam, k, got)
    print("table %d lambda %.1f: largest pick shortfall %.3e, largest stat error %.3e" % (table, lam, worst, worst_stat))
    assert not np.array_equal(got[1][:, :k], ids[:, :k])                 # the re-ranking moved something
    one = _div_dev(img_d, lo, sc, ids, 1.0, k)                           # lambda = 1: the first k candidates bit for bit
    n = D.valid_counts(ids, lo, img.shape[0])
    keep = np.arange(k)[None, :] < n[:, None]
    assert np.array_equal(one[1], np.where(keep, ids[:, :k], -1)) and _eq(one[0], np.where(keep, sc[:, :k], -np.inf).astype(np.float32))


# ---------------------------------------------------------------------------------------------- 3. the host layer
@pytest.mark.parametrize("I", [1001, 1537])
def test_recommender_with_diversify(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Diversify, LongTailReport, MinSlots, Recommender
    rng = np.random.default_rng(I)
    n, k, c = 300, 100, 200
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    plain_ids, _ = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=1.0)
    div = Diversify(0.3, candidates=c)
    rep = LongTailReport(labels, 2)
    rec = Recommender(eng, ev, k=k, chunk=128, diversify=div, report=rep)
    ids, sc = rec.run(rng_step=77, keep_prob=1.0)
    st = div.stats()
    # by hand on the short last chunk, whose logits are still in the activations: ltg_topk at `candidates`, then the entry point
    tr, _ = ev.rows(256, n)
    m = n - 256
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    c_s, c_i, w_s, w_i, w_st = new(m, c), new(m, c, dt=torch.int32), new(m, k), new(m, k, dt=torch.int32), new(m, 2)
    eng.topk(rec.acts, tr, c, c_s, c_i)
    eng.topk_diversify(eng.item_pack("decoder", "cosine"), 0, c_s, c_i, 0.3, k, w_s, w_i, w_st)
    torch.cuda.synchronize()
    assert np.array_equal(ids[256:], w_i.cpu().numpy()) and _eq(sc[256:], w_s.cpu().numpy()) and _eq(st[256:], w_st.cpu().numpy())
    assert np.array_equal(np.sort(ids[:, :k], 1)[:, 1:] != np.sort(ids[:, :k], 1)[:, :-1], np.ones((n, k - 1), bool))       # k distinct ids
    assert not np.array_equal(ids, plain_ids) and np.array_equal(ids[:, 0], plain_ids[:, 0])
    # the report read the diversified lists: ltg_topk_metrics over them, chunk by chunk
    rep2 = LongTailReport(labels, 2)
    rep2.bind(eng, n, k)
    ids_d = _t(ids)
    for lo in range(0, n, 128):
        hi = min(n, lo + 128)
        rep2.add(eng, ids_d[lo:hi], ev.rows(lo, hi)[1], lo)
    (o1, h1), (o2, h2) = rep.table(), rep2.table()
    assert _eq(o1, o2) and np.array_equal(h1, h2) and np.array_equal(h1, np.bincount(ids.ravel(), minlength=I))
    assert st[:, 1].mean() <= st[:, 0].mean()                            # a sanity check, not a bound
    print("I %d: mean pair similarity %.6f -> %.6f" % (I, st[:, 0].mean(), st[:, 1].mean()))
    ids2, sc2 = Recommender(eng, ev, k=k, chunk=128, diversify=Diversify(0.3, candidates=c)).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids2, ids) and _eq(sc2, sc)                    # run to run, and the report changes nothing
    ids1, _ = Recommender(eng, ev, k=k, chunk=128, diversify=Diversify(1.0)).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids1, plain_ids)                               # lam = 1: the plain list
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=k, chunk=128, diversify=Diversify(0.3), rule=MinSlots(labels, 3, [0, 5, 5]))
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recommender_with_diversify(world):
    run_ranks("dist_diversify_worker.py", ["1001", "230"], world, "DIVERSIFY_SHARDED_OK world=%d" % world)


def test_clis_on_askubuntu(tmp_path):
    import torch
    from ltgan import data_processing as dp
    from ltgan import recommend as rc
    from ltgan.dataset import EvalData
    from ltgan.trainer import Recommender
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)

    out = run_cli("recommend.py", [ds, ck, "--diversify", "0.5", "--out", "div.tsv"], cwd)
    assert out[-2].startswith("users: %d\tniche_share@100: " % tr.shape[0]) and out[-1].startswith("ils@100: ") and " -> " in out[-1]
    before, after = (float(x) for x in out[-1][len("ils@100: "):].split(" -> "))
    print(out[-1])
    assert np.isfinite(before) and np.isfinite(after) and after <= before
    lines = open(os.path.join(cwd, "div.tsv")).read().splitlines()
    assert len(lines) == tr.shape[0]
    for n, line in enumerate(lines):
        u, items = line.split("\t")
        items = [int(x) for x in items.split(",")]
        assert int(u) == uid0 + n and len(items) == 100 == len(set(items)) and min(items) >= 0 and max(items) < n_items
    out = run_cli("longtail.py", [ds, ck, "--diversify", "0.5", "--candidates", "150", "--div-space", "encoder"], cwd)
    assert out[-1].startswith("ils@100: ") and out[-2].startswith("all\t") and len(out[-2].split("\t")) == 9
    # without the option: the summary of the plain Recommender as the last line, and no other
    plain = run_cli("recommend.py", [ds, ck, "--out", "plain.tsv"], cwd)
    ids, _ = Recommender(eng, EvalData(tr, te, eng.device), k=100).run(rng_step=rc.RNG_STEP)
    _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(ds, "item2id.txt"), os.path.join(ds, "item_list.txt"),
                                               os.path.join(ds, "niche_items.txt"), n_items)
    assert plain[-1] == rc.summary_line(rc.long_tail_summary(ids, niche, n_items, te), 100)
    assert not any(l.startswith("ils@") for l in plain)
    torch.cuda.synchronize()
