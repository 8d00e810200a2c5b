"""CPU-side checks of the calibrated lists: ltg_hist_groups and ltg_topk_calibrate are exported and bound with the header's argument
types, every documented refusal returns LTG_EINVAL without a GPU, Calibrate and the Recommender validate, both CLIs handle --calibrate,
the extra summary line, and the numpy reference the GPU tests lean on (tests/calibrate_ref.py): equal to its plain-loop restatement on
random rows full of special cases, and with the four consequences of the definition that DESIGN 5.15 lists."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import calibrate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32 = C.c_void_p, C.c_int32
    hist_args = [C.POINTER(cabi.ltg_batch), i32, i32, vp, i32, i32, vp, vp]
    cal_args = [i32, i32, i32, vp, vp, C.POINTER(i32), i32, vp, C.c_float, i32, vp, vp, vp, vp]
    assert cabi.SYMBOLS["ltg_hist_groups"] == (C.c_int, hist_args) and cabi.SYMBOLS["ltg_topk_calibrate"] == (C.c_int, cal_args)
    assert lib.ltg_hist_groups.argtypes == hist_args and lib.ltg_hist_groups.restype == C.c_int
    assert lib.ltg_topk_calibrate.argtypes == cal_args and lib.ltg_topk_calibrate.restype == C.c_int
    assert cabi.LTG_CAL_MAX_CLASSES == 9
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_CAL_MAX_CLASSES 9" in header and "#define LTG_ABI_VERSION 14" in header
    assert "int ltg_hist_groups(const ltg_batch* tr, int32_t hist_lo, int32_t n_rows, const uint8_t* item_group," in header
    assert "int ltg_topk_calibrate(int32_t n_rows, int32_t n_lists, int32_t m_in, const float* score_grp, const int32_t* id_grp," in header
    kernel = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_calibrate.h")).read()
    assert "constexpr int CAL_C = 9;" in kernel


def test_calibrate_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    buf = (C.c_float * 4096)()
    ib = (C.c_int32 * 4096)()

    def cls(*v):
        return (C.c_int32 * len(v))(*v)

    def call(n=2, lists=2, m_in=8, sg=buf, ig=ib, lc=cls(0, 2), g=2, hist=ib, lam=0.5, k=4, so=buf, io=ib, st=None):
        return lib.ltg_topk_calibrate(n, lists, m_in, sg, ig, lc, g, hist, lam, k, so, io, st, None)

    assert call(n=0) == 0
    for name in ("sg", "ig", "lc", "hist", "so", "io"):
        assert call(**{name: None}) == -1, name
    for g in (0, -1, 9, 2 ** 31 - 1):
        assert call(g=g, lists=1, lc=cls(0)) == -1, g
    for lists in (0, -1, 4):
        assert call(lists=lists, lc=cls(0, 1, 2, 3)) == -1, lists
    for k in (0, -1, 9):
        assert call(k=k) == -1, k
    for m_in in (0, -1, 1025):
        assert call(m_in=m_in, k=1) == -1, m_in
    for lam in (-1e-6, 1.0 + 1e-6, float("nan"), float("inf"), -float("inf")):
        assert call(lam=lam) == -1, lam
    for bad in (cls(1, 1), cls(2, 0), cls(-1, 0), cls(0, 3), cls(2, 2)):
        assert call(lc=bad) == -1, list(bad)
    assert call(n=-1) == -1
    # zero rows: nothing to launch, but the arguments are still checked
    assert call(n=0, lam=0.0) == 0 and call(n=0, lam=1.0, st=buf, m_in=1024, k=1024) == 0
    assert call(n=0, g=8, lists=9, lc=cls(*range(9))) == 0 and call(n=0, lists=3, lc=cls(0, 1, 2)) == 0
    assert call(n=0, k=9) == -1 and call(n=0, lam=2.0) == -1 and call(n=0, lc=cls(1, 0)) == -1 and call(n=0, g=9) == -1


def test_hist_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    ptr = (C.c_int32 * 8)()
    lab = (C.c_uint8 * 16)()
    out = (C.c_int32 * 64)()

    def batch(n_rows=2, indptr=True, indices=True):
        return cabi.ltg_batch(n_rows, 0, C.addressof(ptr) if indptr else None, C.addressof(ptr) if indices else None, None, None, None, None,
                              None, None, None)

    def call(tr=batch(), lo=0, n=2, labels=lab, n_glob=16, g=2, co=out):
        return lib.ltg_hist_groups(C.byref(tr) if tr is not None else None, lo, n, labels, n_glob, g, co, None)

    assert call(tr=batch(0), n=0) == 0
    for name in ("tr", "labels", "co"):
        assert call(**{name: None}) == -1, name
    assert call(tr=batch(indptr=False)) == -1 and call(tr=batch(indices=False)) == -1
    assert call(tr=batch(3)) == -1 and call(n=3) == -1 and call(tr=batch(-1), n=-1) == -1
    assert call(lo=-1) == -1
    for n_glob in (0, -5):
        assert call(n_glob=n_glob) == -1
    for g in (0, -1, 9):
        assert call(g=g) == -1, g
    assert call(tr=batch(0), n=0, g=9) == -1 and call(tr=batch(0), n=0, lo=-1) == -1 and call(tr=batch(0), n=0, g=8, lo=2 ** 31 - 1) == 0


class _FakeEngine:
    I, I_global, device, item_lo = 50, 50, "cpu", 0


def test_calibrate_validation():
    from ltgan.sharded import Calibrate as ShardedCalibrate
    from ltgan.trainer import Calibrate, Diversify, Recommender
    assert ShardedCalibrate is Calibrate
    labels = np.array([0, 1, 7] * 16 + [0, 0], np.uint8)
    for lam in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            Calibrate(labels, 2, lam)
    for g in (0, 9, -1):
        with pytest.raises(ValueError):
            Calibrate(labels, g, 0.5)
    with pytest.raises(ValueError):
        Calibrate(labels[:49], 2, 0.5).bind(_FakeEngine(), 10, 20, 33)      # a label count that differs from the catalogue
    c = Calibrate(labels, 2, 0.5)
    c.bind(_FakeEngine(), 10, 20, 33)
    assert c.classes == [0, 1, 2] and c.masks == [1, 2, 0x1FC]               # label 7 is in no group: the last class, bits 2 .. 8
    assert tuple(c.stat.shape) == (33, 2) and tuple(c.class_lists(7, 20)[1].shape) == (3, 7, 20) and c.hist.numel() == 10 * 3
    c = Calibrate(labels, 8, 1.0)
    c.bind(_FakeEngine(), 4, 5, 6)
    assert c.classes == [0, 1, 7] and c.masks == [1, 2, 128]                 # only the classes that occur get a list
    c = Calibrate(np.minimum(labels, 1), 3, 0.0)
    c.bind(_FakeEngine(), 4, 5, 6)
    assert c.classes == [0, 1] and tuple(c.class_lists(4, 5)[0].shape) == (2, 4, 5) and c.hist.numel() == 4 * 4
    good = Calibrate(labels, 2, 0.5)
    for kw in (dict(rule=object()), dict(diversify=Diversify(0.5))):        # refused before anything of the engine is touched
        with pytest.raises(ValueError):
            Recommender(_FakeEngine(), None, k=10, calibrate=good, **kw)
    with pytest.raises(ValueError):
        Recommender(_FakeEngine(), None, k=0, calibrate=good)


def test_cli_arguments():
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    for mod in (rc, lt):
        a = mod.parse_args(["ds", "model.pt"])                           # nothing changes without the option
        assert a.calibrate is None and a.diversify is None and a.min_slots is None
        assert mod.parse_args(["ds", "m.pt", "--calibrate", "0.9"]).calibrate == 0.9
        assert mod.parse_args(["ds", "m.pt", "--calibrate", "0"]).calibrate == 0.0
        a = mod.parse_args(["ds", "m.pt", "--calibrate", "1", "--groups", "pop:4"])
        assert (a.calibrate, a.group_kind, a.n_groups) == (1.0, "pop", 4)
        for bad in (["--calibrate", "-0.1"], ["--calibrate", "1.5"], ["--calibrate", "nan"], ["--calibrate", "x"], ["--calibrate"],
                    ["--calibrate", "0.5", "--min-slots", "niche:5"], ["--calibrate", "0.5", "--diversify", "0.5"],
                    ["--calibrate", "0.5", "--groups", "pop:9"]):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(["ds", "m.pt"] + bad)
            assert e.value.code == 2, (mod.__name__, bad)
    assert rc.parse_args(["ds", "m.pt", "--calibrate", "0.5", "--explain", "3"]).explain == 3      # the explanations read the calibrated lists


def test_miscal_line_from_a_hand_made_table():
    import scipy.sparse as sp
    from ltgan import longtail as lt
    stats = np.array([[0.5, 0.25], [9.0, 9.0], [0.25, 0.125]], np.float32)
    tr = sp.csr_matrix(np.array([[1, 0, 1], [0, 0, 0], [0, 1, 0]], np.float32))          # user 1 has no history
    assert lt.miscal_line(stats, tr, 100) == "miscal@100: 0.375000 -> 0.187500"
    assert lt.miscal_line(stats[1:2], tr[1:2], 7) == "miscal@7: nan -> nan"


# ---------------------------------------------------------------------------------------------- the reference
CASES = [(1, (0, 1), 8, 8), (2, (0, 2), 9, 7), (3, (0, 1, 2, 3), 12, 12), (4, (1, 3, 4), 20, 5), (8, tuple(range(9)), 6, 6), (3, (2,), 10, 10)]


@pytest.fixture(scope="module")
def rows():
    """about 300 rows over six shapes, every kind of special row in each"""
    return [(g, lc, k) + R.build_case(100 + n, 50, g, lc, m_in, k) for n, (g, lc, m_in, k) in enumerate(CASES)]


def test_reference_equals_the_plain_loop(rows):
    seen, moved, total = set(), 0, 0
    for g, lc, k, S, I, hist, kinds in rows:
        for u in range(S.shape[1]):
            lam = (0.0, 0.25, 0.5, 0.99, 1.0)[u % 5]
            ws, wi, wst, _ = R.calibrate_row(S[:, u], I[:, u], lc, g, hist[u], lam, k)
            ids, sc, st = R.loop_row(S[:, u], I[:, u], lc, g, hist[u], lam, k)
            n = len(ids)
            assert n == min(k, sum(R.valid_len(I[j, u]) for j in range(len(lc)))), (g, u)
            assert wi[:n].tolist() == ids and (wi[n:] == -1).all() and np.isneginf(ws[n:]).all(), (g, u, kinds[u], lam)
            assert np.array_equal(ws[:n].view(np.uint32), np.array(sc, np.float32).view(np.uint32)), (g, u)
            assert np.array_equal(wst.view(np.uint32), np.array(st, np.float32).view(np.uint32)), (g, u, kinds[u], lam, wst, st)
            assert len(set(ids)) == n and ((wst >= 0) & (wst <= 1)).all()
            seen.add(kinds[u])
            total += 1
            moved += int(not np.array_equal(wi, R.plain_lists(S[:, u:u + 1], I[:, u:u + 1], k)[1][0]))
    assert seen == set(R.KINDS) and total == 300 and moved > 60, (seen, total, moved)


def test_lambda_zero_and_an_empty_history_give_the_plain_list(rows):
    for g, lc, k, S, I, hist, kinds in rows:
        ps, pi = R.plain_lists(S, I, k)
        ws, wi, st = R.calibrate_lists(S, I, lc, g, hist, 0.0, k)
        assert np.array_equal(wi, pi) and np.array_equal(ws.view(np.uint32), ps.view(np.uint32))
        assert np.array_equal(st[:, 0], st[:, 1])
        empty = np.nonzero(hist.sum(1) == 0)[0]
        assert empty.size >= 4
        for lam in (0.3, 1.0):
            for u in empty:
                ws, wi, st, _ = R.calibrate_row(S[:, u], I[:, u], lc, g, hist[u], lam, k)
                assert np.array_equal(wi, pi[u]) and np.array_equal(ws.view(np.uint32), ps[u].view(np.uint32)) and (st == 0).all()


def test_two_classes_at_lambda_one_follow_the_rounded_share():
    """both classes keep candidates (full lists of m_in >= k entries): the list holds n_0 entries of class 0 with |n_0 - k h_0 / H| <= 1/2"""
    k = 25
    S, I, hist, _ = R.build_case(7, 200, 1, (0, 1), k, k, kinds=("regular", "ties", "equal", "bigH"))
    cls_of = {}
    for u in range(200):
        _, wi, st, picks = R.calibrate_row(S[:, u], I[:, u], (0, 1), 1, hist[u], 1.0, k)
        n0, (h0, h1) = sum(1 for j, _ in picks if j == 0), (int(x) for x in hist[u])
        assert len(picks) == k and abs(Fraction(n0) - Fraction(k * h0, h0 + h1)) <= Fraction(1, 2), (u, n0, h0, h1)
        for m in range(1, k + 1):                                       # ... and so does every prefix of it
            n0m = sum(1 for j, _ in picks[:m] if j == 0)
            assert abs(Fraction(n0m) - Fraction(m * h0, h0 + h1)) <= Fraction(1, 2), (u, m)
        cls_of[u] = n0
    assert len(set(cls_of.values())) > 10


@pytest.mark.parametrize("n_groups", [1, 2, 4])
def test_mean_miscalibration_falls_below_a_hundredth_at_lambda_one(n_groups):
    """C = 2, 3 and 5 classes, 200 rows of full lists at k = 100: the plain lists are far from the histories' mix, the calibrated ones
    within rounding of it (a list of 100 entries can match C shares to about C / 400 at the worst)"""
    lc = tuple(range(n_groups + 1))
    S, I, hist, _ = R.build_case(11 + n_groups, 200, n_groups, lc, 100, 100, kinds=("regular",))
    _, _, st = R.calibrate_lists(S, I, lc, n_groups, hist, 1.0, 100)
    before, after = st.astype(np.float64).mean(0)
    print("C = %d: mean tv %.4f -> %.4f" % (n_groups + 1, before, after))
    assert before > 0.2 and after < 0.01 and (st[:, 1] <= st[:, 0]).all()
