"""Calibrated top-K lists on the GPU: ltg_hist_groups exactly against numpy; ltg_topk_calibrate's ids, score bits and statistic bits
against the reference of tests/calibrate_ref.py (nothing in the definition is a transcendental or an MFMA sum, so real-valued Gaussian
scores are held bit for bit) at a single class, a wave boundary (64 / 65), lists that run out, 1 024-entry lists (heads read from global
memory) and k = 1; Recommender(calibrate=) against the entry points called by hand, with a LongTailReport reading the calibrated lists;
the item-sharded recommender (tests/dist_calibrate_worker.py) and both CLIs on Askubuntu_Sample in fresh child processes."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import calibrate_ref as R
from serving_harness import DEV, _bits, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu
LAMBDAS = (0.0, 0.25, 0.5, 0.99, 1.0)


def _cal_dev(S, I, list_class, n_groups, hist, lam, k, stat=True):
    """ltg_topk_calibrate through the C ABI on host arrays -> host (scores, ids, stats)"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    L, n, m_in = I.shape
    s_d, i_d, h_d = _t(np.asarray(S, np.float32)), _t(np.asarray(I, np.int32)), _t(np.asarray(hist, np.int32))
    so = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
    io = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    st = torch.full((n, 2), 7.0, dtype=torch.float32, device=DEV) if stat else None
    lc = (C.c_int32 * L)(*list_class)
    rc = lib.ltg_topk_calibrate(n, L, m_in, s_d.data_ptr(), i_d.data_ptr(), lc, n_groups, h_d.data_ptr(), lam, k, so.data_ptr(), io.data_ptr(),
                                st.data_ptr() if stat else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), io.cpu().numpy(), st.cpu().numpy() if stat else None


# ---------------------------------------------------------------------------------------------- 1. the histogram
@pytest.mark.parametrize("n_groups", [1, 3, 8])
@pytest.mark.parametrize("hist_lo", [0, 13])
def test_hist_groups_equals_numpy(n_groups, hist_lo):
    import torch
    from ltgan import _cabi as cabi
    from ltgan.engine import CsrRows
    lib = cabi.load()
    rng = np.random.default_rng(10 * n_groups + hist_lo)
    n_items = 6007
    labels = rng.integers(0, 256, n_items).astype(np.uint8)
    labels[rng.integers(0, n_items, 3000)] = rng.integers(0, n_groups + 1, 3000).astype(np.uint8)       # (most labels above 8 otherwise)
    lens = [0, 1, 63, 64, 65, 257, 5000, 0, 130]
    rows = [np.sort(rng.choice(n_items, m, replace=False)) for m in lens]
    rows[2][-1] = rows[5][-1] = n_items - 1                             # with hist_lo = 13 these lie outside the catalogue
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32)
    want = R.hist_groups(indptr, indices, hist_lo, labels, n_groups)
    assert want.sum(1).tolist() != lens if hist_lo else want.sum(1).tolist() == lens
    tr = CsrRows(_t(indptr), _t(indices), 0, len(lens))
    out = torch.full((len(lens), n_groups + 1), -77, dtype=torch.int32, device=DEV)      # a sentinel: the counts are written, not added to
    rc = lib.ltg_hist_groups(C.byref(tr.c), hist_lo, len(lens), _t(labels).data_ptr(), n_items, n_groups, out.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    # a range of rows of a longer CSR: indptr stays absolute
    sub = CsrRows(_t(indptr), _t(indices), 3, 7)
    out2 = torch.full((4, n_groups + 1), -77, dtype=torch.int32, device=DEV)
    assert lib.ltg_hist_groups(C.byref(sub.c), hist_lo, 4, _t(labels).data_ptr(), n_items, n_groups, out2.data_ptr(),
                               torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), want[3:7])


# ---------------------------------------------------------------------------------------------- 2. parity with the reference
#        (n_groups, m_in, k), the classes that have a list, rows, the kinds of the rows
CASES = [((1, 8, 8), (0, 1), 23, R.KINDS),
         ((2, 65, 64), (0, 2), 23, R.KINDS),                             # class 1 has no list: its history share still counts
         ((2, 100, 100), (0, 1, 2), 23, R.KINDS),
         ((3, 130, 100), (0, 2, 3), 23, R.KINDS),
         ((8, 1024, 1024), tuple(range(9)), 6, ("regular", "ties", "short", "bigH", "usedup", "ragged")),
         ((3, 100, 1), (1, 3), 23, R.KINDS)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_calibrate_parity_with_the_reference(case):
    (n_groups, m_in, k), lc, n, kinds = CASES[case]
    S, I, hist, row_kind = R.build_case(500 + case, n, n_groups, lc, m_in, k, kinds=kinds)
    assert set(row_kind) == set(kinds) and (hist.sum(1) == 5000).any()
    moved = 0
    for lam in LAMBDAS:
        wS, wI, wst = R.calibrate_lists(S, I, lc, n_groups, hist, lam, k)
        gS, gI, gst = _cal_dev(S, I, lc, n_groups, hist, lam, k)
        bad = np.nonzero((gI != wI).any(1))[0]
        assert bad.size == 0, (CASES[case][0], lam, [row_kind[u] for u in bad[:5]], bad[:5], gI[bad[:1]], wI[bad[:1]])
        assert np.array_equal(_bits(gS), _bits(wS)), (CASES[case][0], lam)
        badst = np.nonzero((_bits(gst) != _bits(wst)).any(1))[0]
        assert badst.size == 0, (CASES[case][0], lam, [row_kind[u] for u in badst[:5]], gst[badst[:3]], wst[badst[:3]])
        gS2, gI2, _ = _cal_dev(S, I, lc, n_groups, hist, lam, k, stat=False)      # stat_out NULL, and twice in a row: the same bits
        assert np.array_equal(gI2, gI) and np.array_equal(_bits(gS2), _bits(gS))
        if lam == 0.0:
            pS, pI = R.plain_lists(S, I, k)
            assert np.array_equal(gI, pI) and np.array_equal(_bits(gS), _bits(pS))
        else:
            moved += int(not np.array_equal(gI, R.plain_lists(S, I, k)[1]))
    assert moved == len(LAMBDAS) - 1 or k == 1                           # the inputs discriminate: calibration moved something


@pytest.mark.parametrize("case", [1, 3])
def test_lambda_zero_equals_the_merge_of_the_lists(case):
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    (n_groups, m_in, k), lc, n, kinds = CASES[case]
    S, I, hist, _ = R.build_case(900 + case, n, n_groups, lc, m_in, k, kinds=kinds)
    s_d, i_d = _t(S), _t(I)
    so = torch.empty(n, k, dtype=torch.float32, device=DEV)
    io = torch.empty(n, k, dtype=torch.int32, device=DEV)
    assert lib.ltg_topk_merge(len(lc), n, m_in, s_d.data_ptr(), i_d.data_ptr(), k, so.data_ptr(), io.data_ptr(),
                              torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    gS, gI, gst = _cal_dev(S, I, lc, n_groups, hist, 0.0, k)
    assert np.array_equal(gI, io.cpu().numpy()) and np.array_equal(_bits(gS), _bits(so.cpu().numpy()))
    assert np.array_equal(_bits(gst[:, 0]), _bits(gst[:, 1]))


# ---------------------------------------------------------------------------------------------- 3. the host layer
@pytest.mark.parametrize("I", [1001, 1537])
def test_recommender_with_calibrate(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Calibrate, Diversify, LongTailReport, MinSlots, Recommender
    rng = np.random.default_rng(I)
    n, k, lam = 300, 100, 0.7
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    labels = rng.integers(0, 4, I).astype(np.uint8)                      # n_groups = 3 and a label 3: the class "in no group" occurs
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=1.0)
    cal = Calibrate(labels, 3, lam)
    rep = LongTailReport(labels, 3)
    rec = Recommender(eng, ev, k=k, chunk=128, calibrate=cal, report=rep)
    ids, sc = rec.run(rng_step=77, keep_prob=1.0)
    st = cal.stats()
    assert cal.classes == [0, 1, 2, 3]
    # by hand on the short last chunk, whose logits are still in the activations: one list per class, the histogram, the entry point
    tr, _ = ev.rows(256, n)
    m = n - 256
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    g_s, g_i, w_s, w_i, w_st = new(4, m, k), new(4, m, k, dt=torch.int32), new(m, k), new(m, k, dt=torch.int32), new(m, 2)
    lab_d = _t(labels)
    for j, mask in enumerate((1, 2, 4, 0x1F8)):
        eng.topk_groups(rec.acts, tr, k, lab_d, mask, g_s[j], g_i[j])
    h_d = torch.full((m, 4), -5, dtype=torch.int32, device=eng.device)
    eng.hist_groups(tr, lab_d, 3, h_d)
    eng.topk_calibrate(g_s, g_i, [0, 1, 2, 3], 3, h_d, lam, k, w_s, w_i, w_st)
    torch.cuda.synchronize()
    Xc = X.tocsr()
    assert np.array_equal(h_d.cpu().numpy(), R.hist_groups(Xc.indptr, Xc.indices, 0, labels, 3)[256:])
    assert np.array_equal(ids[256:], w_i.cpu().numpy()) and np.array_equal(_bits(sc[256:]), _bits(w_s.cpu().numpy()))
    assert np.array_equal(_bits(st[256:]), _bits(w_st.cpu().numpy()))
    srt = np.sort(ids, 1)
    assert (srt[:, 1:] != srt[:, :-1]).all() and ids.min() >= 0 and ids.max() < I                     # k distinct ids in range
    assert not np.array_equal(ids, plain_ids)
    # the report read the calibrated lists: ltg_topk_metrics over them, chunk by chunk
    rep2 = LongTailReport(labels, 3)
    rep2.bind(eng, n, k)
    ids_d = _t(ids)
    for lo in range(0, n, 128):
        hi = min(n, lo + 128)
        rep2.add(eng, ids_d[lo:hi], ev.rows(lo, hi)[1], lo)
    (o1, h1), (o2, h2) = rep.table(), rep2.table()
    assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(h1, h2) and np.array_equal(h1, np.bincount(ids.ravel(), minlength=I))
    assert st[:, 1].mean() <= st[:, 0].mean()                            # a sanity check, not a bound
    print("I %d: mean miscalibration %.6f -> %.6f" % (I, st[:, 0].mean(), st[:, 1].mean()))
    ids2, sc2 = Recommender(eng, ev, k=k, chunk=128, calibrate=Calibrate(labels, 3, lam)).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids2, ids) and np.array_equal(_bits(sc2), _bits(sc))                        # run to run, and the report changes nothing
    ids0, sc0 = Recommender(eng, ev, k=k, chunk=128, calibrate=Calibrate(labels, 3, 0.0)).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids0, plain_ids) and np.array_equal(_bits(sc0), _bits(plain_sc))            # lam = 0: the plain table
    # niche-style labels, two classes (no item is "in no group"), lam = 1: the list follows the rounded share of the history
    niche = (rng.random(I) < 0.4).astype(np.uint8)
    cal1 = Calibrate(niche, 2, 1.0)
    ids1, _ = Recommender(eng, ev, k=k, chunk=128, calibrate=cal1).run(rng_step=77, keep_prob=1.0)
    assert cal1.classes == [0, 1]
    h = R.hist_groups(Xc.indptr, Xc.indices, 0, niche, 2)
    checked = 0
    for u in range(n):
        H = int(h[u].sum())
        left = [(niche == c).sum() - h[u, c] for c in (0, 1)]            # the eligible items of each class
        if H == 0 or min(left) < k:
            continue
        n0 = int((niche[ids1[u]] == 0).sum())
        assert abs(Fraction(n0) - Fraction(k * int(h[u, 0]), H)) <= Fraction(1, 2), (u, n0, h[u])
        checked += 1
    assert checked > n // 2
    for kw in (dict(diversify=Diversify(0.3)), dict(rule=MinSlots(labels, 4, [0, 5, 5, 0]))):
        with pytest.raises(ValueError):
            Recommender(eng, ev, k=k, chunk=128, calibrate=Calibrate(labels, 3, lam), **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recommender_with_calibrate(world):
    run_ranks("dist_calibrate_worker.py", ["1001", "230"], world, "CALIBRATE_SHARDED_OK world=%d" % world)


def test_clis_on_askubuntu(tmp_path):
    import torch
    from ltgan import data_processing as dp
    from ltgan import recommend as rc
    from ltgan.dataset import EvalData
    from ltgan.trainer import Recommender
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)

    def miscal(line):
        assert line.startswith("miscal@100: ") and " -> " in line, line
        before, after = (float(x) for x in line[len("miscal@100: "):].split(" -> "))
        assert np.isfinite(before) and np.isfinite(after) and after <= before, line
        return before, after

    out = run_cli("recommend.py", [ds, ck, "--calibrate", "0.9", "--out", "cal.tsv"], cwd)
    assert out[-2].startswith("users: %d\tniche_share@100: " % tr.shape[0])
    print(out[-1])
    miscal(out[-1])
    lines = open(os.path.join(cwd, "cal.tsv")).read().splitlines()
    assert len(lines) == tr.shape[0]
    for n, line in enumerate(lines):
        u, items = line.split("\t")
        items = [int(x) for x in items.split(",")]
        assert int(u) == uid0 + n and len(items) == 100 == len(set(items)) and min(items) >= 0 and max(items) < n_items
    out = run_cli("longtail.py", [ds, ck, "--calibrate", "0.9", "--groups", "pop:3"], cwd)
    miscal(out[-1])
    assert out[-2].startswith("all\t") and len(out[-2].split("\t")) == 9
    # without the option: the summary of the plain Recommender as the last line, and no other
    plain = run_cli("recommend.py", [ds, ck, "--out", "plain.tsv"], cwd)
    ids, _ = Recommender(eng, EvalData(tr, te, eng.device), k=100).run(rng_step=rc.RNG_STEP)
    _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(ds, "item2id.txt"), os.path.join(ds, "item_list.txt"),
                                               os.path.join(ds, "niche_items.txt"), n_items)
    assert plain[-1] == rc.summary_line(rc.long_tail_summary(ids, niche, n_items, te), 100)
    assert not any(l.startswith("miscal@") for l in plain)
    torch.cuda.synchronize()
