"""CPU-side checks of the long-tail report: ltg_topk_metrics is exported and bound under ABI 14 and refuses bad arguments before any
launch; the item-group builders on the materialised Askubuntu_Sample (the numbers below were computed from the fixture); the host
aggregation, both output formats and the Gini coefficient on hand-made tables; longtail.py's argument errors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz")


def test_symbol_is_exported_and_abi_stays_14():
    from ltgan import _cabi as cabi
    assert "ltg_topk_metrics" in cabi.SYMBOLS
    lib = cabi.load()
    assert lib.ltg_topk_metrics is not None
    assert lib.ltg_abi_version() == cabi.LTG_ABI_VERSION == 14
    hdr = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "int ltg_topk_metrics(" in hdr and "#define LTG_ABI_VERSION 14" in hdr


def _call(lib, cabi, **kw):
    """ltg_topk_metrics with valid host-side arguments (nothing is dereferenced on the device before the checks), overridden by kw"""
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)
    a = dict(id_in=p, n_rows=2, k_in=100, te=cabi.ltg_batch(2, 0, p, p), item_group=p, n_items_global=1000, n_groups=2, k_ndcg=100,
             k_r1=20, k_r2=50, k_exp=100, out=p, item_hits=p)
    a.update(kw)
    te = a["te"]
    return lib.ltg_topk_metrics(a["id_in"], a["n_rows"], a["k_in"], C.byref(te) if te is not None else None, a["item_group"],
                                a["n_items_global"], a["n_groups"], a["k_ndcg"], a["k_r1"], a["k_r2"], a["k_exp"], a["out"],
                                a["item_hits"], None)


@pytest.mark.parametrize("bad", [dict(id_in=None), dict(te=None), dict(item_group=None), dict(out=None), dict(n_rows=-1), dict(k_in=0),
                                 dict(k_in=1025), dict(n_groups=0), dict(n_groups=9), dict(k_ndcg=0), dict(k_r1=0), dict(k_r2=0),
                                 dict(k_exp=0), dict(k_ndcg=101), dict(k_r1=101), dict(k_r2=101), dict(k_exp=101),
                                 dict(k_in=10), dict(n_items_global=0), dict(n_items_global=-5), dict(n_rows=3)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_bad_arguments_are_einval(bad):
    from ltgan import _cabi as cabi
    lib = cabi.load()
    assert _call(lib, cabi, **bad) == -1            # LTG_EINVAL (n_rows=3: te->n_rows != n_rows; k_in=10: every default cutoff > k_in)


def test_zero_rows_is_ok_without_a_launch():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    buf = (C.c_int32 * 4)()
    assert _call(lib, cabi, n_rows=0, te=cabi.ltg_batch(0, 0, C.addressof(buf), C.addressof(buf))) == 0
    assert _call(lib, cabi, n_rows=0, te=cabi.ltg_batch(0, 0, C.addressof(buf), C.addressof(buf)), item_hits=None) == 0


@pytest.fixture(scope="module")
def askubuntu(tmp_path_factory):
    from ltgan.dataset import materialize_askubuntu
    return materialize_askubuntu(RAW, str(tmp_path_factory.mktemp("lt") / "Askubuntu_Sample"))


def _users_per_group(ds, split, labels, n_groups):
    from ltgan import data_processing as dp
    from ltgan.dataset import count_items
    _, te, _ = dp.load_tr_te_data(os.path.join(ds, "%s_tr.csv" % split), os.path.join(ds, "%s_te.csv" % split), count_items(ds))
    te = te.tocsr()
    rows = np.repeat(np.arange(te.shape[0]), np.diff(te.indptr))
    lab = labels[te.indices]
    return te.shape[0], int(np.unique(rows).size), [int(np.unique(rows[lab == g]).size) for g in range(n_groups)]


def test_group_builders_on_askubuntu(askubuntu):
    from ltgan import longtail as lt
    from ltgan.dataset import count_items
    ds = askubuntu
    n_items = count_items(ds)
    assert n_items == 1000
    lab, names = lt.build_groups(ds, "niche", 2, n_items)
    assert names == ["popular", "niche"] and lab.dtype == np.uint8 and lab.shape == (1000,)
    assert int((lab == 1).sum()) == 897 and int((lab == 0).sum()) == 103
    n, n_all, per = _users_per_group(ds, "test", lab, 2)
    assert (n, n_all) == (10000, 10000) and per == [9081, 7835]
    assert _users_per_group(ds, "validation", lab, 2)[2] == [9116, 7766]
    lab4, names4 = lt.build_groups(ds, "pop", 4, n_items)
    assert names4 == ["pop0", "pop1", "pop2", "pop3"] and np.bincount(lab4).tolist() == [250, 250, 250, 250]
    assert _users_per_group(ds, "test", lab4, 4)[2] == [9737, 4172, 2563, 1823]
    assert _users_per_group(ds, "validation", lab4, 4)[2] == [9755, 4046, 2534, 1799]
    # the head bucket is the most popular quarter: every count in bucket g >= every count in bucket g + 1
    import pandas as pd
    cnt = np.bincount(pd.read_csv(os.path.join(ds, "train_GAN.csv"))["sid"].to_numpy(), minlength=n_items)
    for g in range(3):
        assert cnt[lab4 == g].min() >= cnt[lab4 == g + 1].max()


def test_pop_groups_tie_rule():
    from ltgan import longtail as lt
    #                 id: 0  1  2  3  4  5  6  7
    counts = np.array([5, 9, 5, 0, 9, 5, 1, 0])
    # order: 1, 4 (9; lower id first), 0, 2, 5 (5), 6 (1), 3, 7 (0)  -> position p gets p * N // 8
    lab, names = lt.pop_groups_from_counts(counts, 2)
    assert lab.tolist() == [0, 0, 0, 1, 0, 1, 1, 1] and names == ["pop0", "pop1"]
    lab, _ = lt.pop_groups_from_counts(counts, 4)
    assert lab.tolist() == [1, 0, 1, 3, 0, 2, 2, 3]
    lab, _ = lt.pop_groups_from_counts(np.zeros(5, int), 3)              # all equal: id order; 5 items over 3 buckets
    assert lab.tolist() == [0, 0, 1, 1, 2]


def _gini_direct(h):
    h = np.sort(np.asarray(h, np.float64))
    n = len(h)
    return sum((2 * (i + 1) - n - 1) * h[i] for i in range(n)) / (n * h.sum())


def test_gini():
    from ltgan import longtail as lt
    rng = np.random.default_rng(0)
    for h in ([1, 1, 1, 1], [0, 0, 0, 8], [3, 0, 1, 7, 7, 2], rng.integers(0, 50, 1000)):
        assert abs(lt.gini(h) - _gini_direct(h)) < 1e-12
    assert lt.gini([1, 1, 1, 1]) == 0.0 and abs(lt.gini([0, 0, 0, 8]) - 0.75) < 1e-15
    assert np.isnan(lt.gini(np.zeros(7, np.int32))) and np.isnan(lt.gini([]))


def _tables():
    # 4 users, 2 groups + all; columns ndcg, recall@20, recall@50, valid
    out = np.zeros((4, 3, 4), np.float32)
    out[0] = [[0.5, 1.0, 1.0, 1], [0.25, 0.5, 0.5, 1], [0.375, 0.75, 0.75, 1]]
    out[1] = [[0.0, 0.0, 0.0, 0], [1.0, 1.0, 1.0, 1], [1.0, 1.0, 1.0, 1]]
    out[2] = [[0.0, 0.0, 0.0, 0], [0.0, 0.0, 0.0, 0], [0.0, 0.0, 0.0, 0]]      # no held-out items: in no mean
    out[3] = [[0.125, 0.0, 1.0, 1], [0.0, 0.0, 0.0, 0], [0.125, 0.0, 1.0, 1]]
    labels = np.array([0, 0, 1, 1, 1, 7], np.uint8)                             # item 5: no group
    hits = np.array([4, 0, 2, 0, 1, 1], np.int32)
    return out, hits, labels


def test_aggregate_and_output_formats(tmp_path):
    from ltgan import longtail as lt
    out, hits, labels = _tables()
    rep = lt.aggregate(out, hits, labels, ["popular", "niche"], 10)
    g0, g1 = rep["groups"]
    a = rep["all"]
    assert (g0["name"], g0["items"], g0["users"]) == ("popular", 2, 2) and (g1["name"], g1["items"], g1["users"]) == ("niche", 3, 2)
    assert (a["name"], a["items"], a["users"]) == ("all", 6, 3) and rep["k"] == 10
    assert g0["ndcg"] == np.float64(np.float32(0.5) + np.float32(0.125)) / 2 and g0["recall20"] == 0.5 and g0["recall50"] == 1.0
    assert g1["ndcg"] == 0.625 and g1["recall20"] == 0.75 and g1["recall50"] == 0.75
    o64 = out.astype(np.float64)
    ok = o64[:, 2, 3] > 0
    assert a["ndcg"] == float(o64[ok, 2, 0].mean()) and a["recall20"] == float(o64[ok, 2, 1].mean())     # Evaluator.run's expression
    assert g0["share"] == 4 / 8 and g1["share"] == 3 / 8 and a["share"] == 1.0
    assert g0["coverage"] == 1 / 2 and g1["coverage"] == 2 / 3 and a["coverage"] == 4 / 6
    assert abs(a["gini"] - _gini_direct(hits)) < 1e-12
    lines = lt.report_lines(rep)
    assert len(lines) == 4
    assert lines[0] == str(a["ndcg"]) + "\t" + str(a["recall20"]) + "\t" + str(a["recall50"])          # test.py's print
    assert lines[1] == "popular\t2\t2\t0.312500000\t0.500000000\t1.000000000\t0.500000\t0.500000"
    assert lines[2] == "niche\t3\t2\t0.625000000\t0.750000000\t0.750000000\t0.375000\t0.666667"
    f = lines[3].split("\t")
    assert f[0] == "all" and len(f) == 9 and f[1:3] == ["6", "3"] and f[6] == "1.000000" and f[7] == "0.666667"
    assert abs(float(f[8]) - a["gini"]) < 1e-6
    path = str(tmp_path / "r.json")
    lt.write_json(rep, path)
    back = json.load(open(path))
    assert back["all"] == a and back["groups"] == rep["groups"] and back["k"] == 10
    # nothing recommended, nobody valid: nan, not a crash
    rep0 = lt.aggregate(np.zeros((3, 3, 4), np.float32), np.zeros(6, np.int32), labels, ["popular", "niche"], 5)
    assert rep0["all"]["users"] == 0 and np.isnan(rep0["all"]["ndcg"]) and np.isnan(rep0["all"]["gini"]) and np.isnan(rep0["groups"][0]["share"])
    assert rep0["all"]["coverage"] == 0.0
    assert len(lt.report_lines(rep0)) == 4


@pytest.mark.parametrize("argv", [["--groups", "pop:1"], ["--groups", "pop:9"], ["--groups", "pop:x"], ["--groups", "head"], ["--k", "0"],
                                  ["--k", "1025"], ["--keep-prob", "0"], ["--split", "train"]])
def test_cli_argument_errors(argv, capsys):
    from ltgan import longtail as lt
    with pytest.raises(SystemExit) as e:
        lt.parse_args(["ds", "ck"] + argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_arguments():
    from ltgan import longtail as lt
    a = lt.parse_args(["ds", "ck"])
    assert (a.split, a.group_kind, a.n_groups, a.k, a.keep_prob, a.json) == ("test", "niche", 2, 100, 0.75, None)
    a = lt.parse_args(["ds", "ck", "--groups", "pop:8", "--k", "1024", "--split", "validation", "--json", "r.json"])
    assert (a.split, a.group_kind, a.n_groups, a.k, a.json) == ("validation", "pop", 8, 1024, "r.json")


def test_report_option_checks_its_arguments():
    from ltgan.trainer import LongTailReport
    r = LongTailReport(np.zeros(10, np.uint8), 2, k_exp=300)
    assert r.k == 300 and r.cut == dict(k_ndcg=100, k_r1=20, k_r2=50, k_exp=300)
    assert LongTailReport(np.zeros(10, np.uint8), 1, k_exp=5).k == 100
    for kw in (dict(n_groups=0), dict(n_groups=9), dict(n_groups=2, k_exp=0), dict(n_groups=2, k_ndcg=1025)):
        with pytest.raises(ValueError):
            LongTailReport(np.zeros(10, np.uint8), **kw)
