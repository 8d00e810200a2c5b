"""CPU-side checks of the item audiences: the two entry points are exported and bound, their argument validation answers before any HIP
call, the workspace is lists and never a block of the score matrix, audience.py's argument handling and writers work on a hand-made table,
and the numpy reference the GPU tests compare against (tests/audience_ref.py) agrees with a plain loop."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import audience_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _cfg(cabi, n_items=1000):
    return cabi.ltg_config(n_items, 600, 200, n_items, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


def test_audience_entry_points_are_exported_and_bound():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    for name in ("ltg_item_audience_ws_bytes", "ltg_item_audience"):
        assert name in cabi.SYMBOLS
        assert getattr(lib, name).argtypes == cabi.SYMBOLS[name][1]
    assert lib.ltg_abi_version() == 14 and cabi.LTG_AUD_MAX_K == 256
    hdr = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_AUD_MAX_K 256" in hdr


def test_item_audience_argument_validation_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    cfg = _cfg(cabi)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40

    def call(cfg=cfg, logits=p, lse=p, tr=None, n_rows=4, row_lo=0, q=p, n_q=3, k=8, s=p, i=p, ws=p, ws_bytes=big):
        return lib.ltg_item_audience(C.byref(cfg) if cfg is not None else None, logits, lse, C.byref(tr) if tr is not None else None, n_rows,
                                     row_lo, q, n_q, k, s, i, ws, ws_bytes, None)

    for name in ("cfg", "logits", "q", "s", "i"):
        assert call(**{name: None}) == EINVAL, name
    for k in (0, -1, 257):
        assert call(k=k) == EINVAL, k
    assert call(n_rows=-1) == EINVAL and call(n_q=-1) == EINVAL and call(row_lo=-1) == EINVAL
    assert call(n_rows=2, row_lo=2 ** 31 - 2) == EINVAL                # row_lo + n_rows > INT32_MAX
    assert call(n_rows=0, row_lo=2 ** 31 - 1) == 0                     # ... == INT32_MAX: accepted, and nothing to do
    assert call(cfg=_cfg(cabi, 0)) == EINVAL
    # a tr whose row count disagrees with the call's, or that lacks its arrays
    assert call(tr=cabi.ltg_batch(5, 0, p.value, p.value)) == EINVAL
    assert call(tr=cabi.ltg_batch(4, 0, None, p.value)) == EINVAL
    assert call(tr=cabi.ltg_batch(4, 0, p.value, None)) == EINVAL
    # the workspace: 20 000 rows of 4 queries are cut into row segments, whose lists need room; one byte short, or no buffer, is refused
    need = lib.ltg_item_audience_ws_bytes(C.byref(cfg), 20000, 4, 8)
    assert need >= 2 * 4 * 8 * 8
    assert call(n_rows=20000, n_q=4, ws_bytes=need - 1) == EINVAL
    assert call(n_rows=20000, n_q=4, ws=None, ws_bytes=big) == EINVAL
    # the zero-size calls launch nothing (no GPU here: a launch would fail) and need no workspace, lse or tr
    assert call(n_rows=0) == 0 and call(n_q=0) == 0
    assert call(n_rows=0, lse=None, ws=None, ws_bytes=0) == 0
    assert call(n_q=0, tr=cabi.ltg_batch(4, 0, p.value, p.value), ws=None, ws_bytes=0) == 0
    # arguments the call refuses need no workspace
    ws = lib.ltg_item_audience_ws_bytes
    assert ws(C.byref(cfg), 20000, 4, 257) == 0 and ws(C.byref(cfg), 20000, 4, 0) == 0
    assert ws(C.byref(cfg), -1, 4, 8) == 0 and ws(C.byref(cfg), 20000, -1, 8) == 0
    assert ws(None, 20000, 4, 8) == 0 and ws(C.byref(_cfg(cabi, 0)), 20000, 4, 8) == 0


def test_audience_workspace_is_lists_not_scores():
    """at 20 000 rows x 20 000 queries, k = 100, the workspace is a whole number of (n_q x k) lists -- at most 32 row segments -- and far
    below the 1.6 GB of the scores; a walk in chunks sizes it for every chunk length that occurs (the need is not monotone in the rows)"""
    from ltgan import _cabi as cabi
    from ltgan.trainer import neighbors_ws_bytes
    lib = cabi.load()
    cfg = _cfg(cabi, 20000)
    ws = lambda n, n_q, k: lib.ltg_item_audience_ws_bytes(C.byref(cfg), n, n_q, k)
    assert ws(20000, 20000, 100) < 20000 * 20000 * 4 // 8
    for n, n_q, k in ((20000, 20000, 100), (20000, 7, 256), (3000, 300, 20), (20000, 1, 1), (100, 5, 100)):
        w, per_list = ws(n, n_q, k), n_q * k * 8
        seg = -(-w // per_list)
        assert seg <= 32 and w <= seg * per_list + 256, (n, n_q, k, w)
        assert seg == 0 or seg >= 2                  # one segment writes the outputs itself
    for n_users, chunk, n_q, k in ((50000, 20000, 40, 100), (20001, 20000, 3, 256), (6040, 4096, 1000, 20)):
        have = neighbors_ws_bytes(lambda n, kk: ws(n, n_q, kk), n_users, chunk, k)
        for lo in range(0, n_users, chunk):
            assert ws(min(chunk, n_users - lo), n_q, k) <= have


def _aud():
    from ltgan import audience
    return audience


def test_audience_cli_arguments():
    au = _aud()
    a = au.parse_args(["ds", "model.pt"])
    assert (a.dataset_dir, a.checkpoint, a.k, a.items, a.split, a.keep_prob, a.score, a.out, a.npz) == \
        ("ds", "model.pt", 100, "all", "test", 0.75, "logprob", "audience.tsv", None)
    a = au.parse_args(["ds", "m.pt", "--k", "256", "--items", "niche", "--split", "validation", "--keep-prob", "1.0", "--score", "logit",
                       "--out", "o.tsv", "--npz", "o.npz"])
    assert (a.k, a.items, a.split, a.keep_prob, a.score, a.out, a.npz) == (256, "niche", "validation", 1.0, "logit", "o.tsv", "o.npz")
    assert au.parse_args(["ds", "m.pt", "--k", "1"]).k == 1
    for bad in (["ds", "m.pt", "--k", "0"], ["ds", "m.pt", "--k", "257"], ["ds", "m.pt", "--score", "prob"], ["ds", "m.pt", "--split", "train"],
                ["ds", "m.pt", "--keep-prob", "0"], ["ds"]):
        with pytest.raises(SystemExit):
            au.parse_args(bad)
    script = os.path.join(ROOT, "long-tail-gan_amd", "audience.py")
    for k in ("0", "257"):
        out = subprocess.run([sys.executable, script, "ds", "m.pt", "--k", k], capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and "--k must be in [1, 256]" in out.stderr, (k, out.stderr[-500:])


def test_audience_writers_and_summary(tmp_path):
    au = _aud()
    rows = np.array([[7, 3, 1], [0, 2, -1], [-1, -1, -1]], np.int32)
    scores = np.array([[-0.5, -0.75, -9.25], [-0.0, -3.5, -np.inf], [-np.inf] * 3], np.float32)
    uids = au.write_audience([5, 3, 11], rows, scores, 1000, str(tmp_path / "a.tsv"), str(tmp_path / "a.npz"))
    assert open(tmp_path / "a.tsv").read().splitlines() == ["5\t1007,1003,1001", "3\t1000,1002", "11\t"]      # padding is not a user
    assert uids.tolist() == [[1007, 1003, 1001], [1000, 1002, -1], [-1, -1, -1]]
    z = np.load(tmp_path / "a.npz")
    assert z["items"].tolist() == [5, 3, 11] and z["items"].dtype == np.int32 and np.array_equal(z["uids"], uids)
    assert z["scores"].dtype == np.float32 and np.array_equal(z["scores"].view(np.uint32), scores.view(np.uint32))
    m = au.audience_summary(rows, 10)
    assert m == dict(items=3, users=10, coverage=pytest.approx(0.5))
    assert au.summary_line(m, 3) == "items: 3\tusers: 10\tuser_coverage@3: 0.500000"
    assert au.audience_summary(rows[2:], 10)["coverage"] == 0.0


def test_audience_validates_its_arguments():
    from ltgan.trainer import Audience
    for k in (0, 257):
        with pytest.raises(ValueError):
            Audience([1, 2], k=k)
    with pytest.raises(ValueError):
        Audience([1, 2], score="prob")
    a = Audience([5, 3, 3], k=2, score="logit")
    assert a.items.dtype == np.int32 and a.items.tolist() == [5, 3, 3] and not a.needs_lse and Audience([1]).needs_lse


@pytest.mark.parametrize("k", [1, 3, 9])
def test_reference_lists_equal_a_brute_force_loop(k):
    """7 rows x 5 columns: ties, signed zeros, -inf, a column every row holds, a column held by all rows but one, a repeated query column,
    scores with and without lse, a row offset"""
    rng = np.random.default_rng(k)
    L = (rng.integers(-3, 4, (7, 5)) * 0.25).astype(np.float32)
    L[::2, 1] = -0.0
    L[1, 1] = 0.0
    L[3, 2] = -np.inf
    L[:, 4] = 1.5
    lse = (rng.integers(0, 3, 7) * 0.5).astype(np.float32)
    folds = [np.array(sorted({3} | ({0} if r != 4 else set()) | ({2} if r % 3 == 0 else set()))) for r in range(7)]
    q_col = [4, 0, 3, 1, 2, 1]
    for ls in (lse, None):
        for f in (folds, None):
            for row_lo in (0, 40):
                got = AR.audience_lists(L, ls, f, q_col, k, row_lo)
                want = AR.brute_force(L, ls, f, q_col, k, row_lo)
                assert np.array_equal(got[1], want[1]), (k, ls is None, f is None)
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
                assert np.array_equal(got[1][3], got[1][5]) and np.array_equal(got[0][3].view(np.uint32), got[0][5].view(np.uint32))
                if f is not None:
                    assert (got[1][2] == -1).all() and np.isneginf(got[0][2]).all()           # column 3: every row holds it
                    assert got[1][1].tolist() == [4 + row_lo] + [-1] * (k - 1)                # column 0: all rows but row 4
