"""CPU-side checks of the top-K recommendation path: the two entry points are exported and bound, their argument validation returns
LTG_EINVAL before any HIP call, and recommend.py's argument handling, writers and long-tail summary work on hand-made tables."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(cabi, n_items=1000, item_lo=0):
    return cabi.ltg_config(n_items, 600, 200, n_items, 100, 150, 250, 300, 0, 0, item_lo, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


def test_topk_entry_points_are_exported_and_bound():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    for name in ("ltg_topk", "ltg_topk_merge"):
        assert name in cabi.SYMBOLS
        assert getattr(lib, name).argtypes == cabi.SYMBOLS[name][1]
    assert lib.ltg_abi_version() == 14


def test_topk_argument_validation_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    cfg = _cfg(cabi)
    buf = (C.c_float * 16)()
    ib = (C.c_int32 * 16)()
    # k out of [1, 1024]
    for k in (0, -1, 1025):
        assert lib.ltg_topk(C.byref(cfg), buf, None, 2, k, buf, ib, None) == -1, k
        assert lib.ltg_topk_merge(2, 2, 4, buf, ib, k, buf, ib, None) == -1, k
    assert lib.ltg_topk_merge(2, 2, 0, buf, ib, 4, buf, ib, None) == -1            # k_in
    assert lib.ltg_topk_merge(2, 2, 1025, buf, ib, 4, buf, ib, None) == -1
    assert lib.ltg_topk_merge(0, 2, 4, buf, ib, 4, buf, ib, None) == -1            # n_parts
    # NULL pointers
    assert lib.ltg_topk(None, buf, None, 2, 4, buf, ib, None) == -1
    assert lib.ltg_topk(C.byref(cfg), None, None, 2, 4, buf, ib, None) == -1
    assert lib.ltg_topk(C.byref(cfg), buf, None, 2, 4, None, ib, None) == -1
    assert lib.ltg_topk(C.byref(cfg), buf, None, 2, 4, buf, None, None) == -1
    for args in ((None, ib, buf, ib), (buf, None, buf, ib), (buf, ib, None, ib), (buf, ib, buf, None)):
        assert lib.ltg_topk_merge(2, 2, 4, args[0], args[1], 4, args[2], args[3], None) == -1
    # a fold-in batch whose row count disagrees, or without its arrays
    tr = cabi.ltg_batch(3, 0, C.cast(ib, C.c_void_p), C.cast(ib, C.c_void_p))
    assert lib.ltg_topk(C.byref(cfg), buf, C.byref(tr), 2, 4, buf, ib, None) == -1
    tr = cabi.ltg_batch(2, 0, None, C.cast(ib, C.c_void_p))
    assert lib.ltg_topk(C.byref(cfg), buf, C.byref(tr), 2, 4, buf, ib, None) == -1
    assert lib.ltg_topk(C.byref(cfg), buf, None, -1, 4, buf, ib, None) == -1       # negative rows
    # a slab too large for the kernel's LDS (fold-in bitset + candidate buffer) is refused, not launched
    assert lib.ltg_topk(C.byref(_cfg(cabi, 600000)), buf, None, 2, 4, buf, ib, None) == -1
    # zero rows: nothing to launch
    assert lib.ltg_topk(C.byref(cfg), buf, None, 0, 4, buf, ib, None) == 0
    assert lib.ltg_topk_merge(2, 0, 4, buf, ib, 4, buf, ib, None) == 0


def _rec():
    from ltgan import recommend
    return recommend


def test_recommend_cli_arguments():
    rc = _rec()
    a = rc.parse_args(["ds", "model.pt"])
    assert (a.dataset_dir, a.checkpoint, a.k, a.split, a.keep_prob, a.out, a.npz) == ("ds", "model.pt", 100, "test", 0.75, "recs.tsv", None)
    a = rc.parse_args(["ds", "m.pt", "--k", "20", "--split", "validation", "--keep-prob", "1.0", "--out", "o.tsv", "--npz", "o.npz"])
    assert (a.k, a.split, a.keep_prob, a.out, a.npz) == (20, "validation", 1.0, "o.tsv", "o.npz")
    for bad in (["ds", "m.pt", "--k", "0"], ["ds", "m.pt", "--k", "1025"], ["ds", "m.pt", "--split", "train"],
                ["ds", "m.pt", "--keep-prob", "0"], ["ds"]):
        with pytest.raises(SystemExit):
            rc.parse_args(bad)
    # the script itself: usage errors before any GPU work
    out = subprocess.run([sys.executable, os.path.join(ROOT, "long-tail-gan_amd", "recommend.py"), "ds", "m.pt", "--k", "2000"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--k must be in [1, 1024]" in out.stderr


def test_recommend_writers_map_rows_to_uids_and_ids_to_sids(tmp_path):
    rc = _rec()
    ids = np.array([[7, 3, 5], [0, 1, -1], [9, 8, 2]], np.int32)
    scores = np.array([[3.0, 2.0, 1.0], [0.5, -0.0, -np.inf], [1.0, 1.0, -np.inf]], np.float32)
    uids = rc.write_recs(ids, scores, 40, str(tmp_path / "r.tsv"), str(tmp_path / "r.npz"))
    assert uids.tolist() == [40, 41, 42]
    lines = open(tmp_path / "r.tsv").read().splitlines()
    assert lines == ["40\t7,3,5", "41\t0,1", "42\t9,8,2"]            # padding (-1) is not an item
    z = np.load(tmp_path / "r.npz")
    assert z["uids"].tolist() == [40, 41, 42] and z["ids"].dtype == np.int32 and np.array_equal(z["ids"], ids)
    assert z["scores"].dtype == np.float32 and np.array_equal(z["scores"].view(np.uint32), scores.view(np.uint32))


def test_long_tail_summary_matches_numpy():
    rc = _rec()
    rng = np.random.default_rng(3)
    n_items, n_users, k = 500, 40, 25
    ids = np.stack([rng.choice(n_items, k, replace=False) for _ in range(n_users)]).astype(np.int32)
    ids[5, 20:] = -1                                                  # a padded row
    niche = set(rng.choice(n_items, 120, replace=False).tolist())
    te = sp.random(n_users, n_items, density=0.02, random_state=4, format="csr")
    te.data[:] = 1.0
    te = te.tolil()
    te[7] = 0                                                         # a user without held-out items: left out of the mean
    te = te.tocsr()
    te.eliminate_zeros()
    m = rc.long_tail_summary(ids, niche, n_items, te)
    flat = ids[ids >= 0]
    assert m["users"] == n_users
    assert m["niche_share"] == pytest.approx(np.mean([i in niche for i in flat.tolist()]), abs=1e-12)
    assert m["coverage"] == pytest.approx(len(set(flat.tolist())) / n_items, abs=1e-12)
    dense = te.toarray() > 0
    want = [dense[r, ids[r, :20][ids[r, :20] >= 0]].sum() / min(20, dense[r].sum()) for r in range(n_users) if dense[r].any()]
    assert m["recall20"] == pytest.approx(float(np.mean(want)), abs=1e-12)
    assert "niche_share@25: " in rc.summary_line(m, k) and rc.summary_line(m, k).startswith("users: 40\t")
