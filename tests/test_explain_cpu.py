"""CPU-side checks of the list explanations: ltg_topk_explain is exported and bound with the header's argument types, every documented
refusal returns LTG_EINVAL without a GPU, Explain and the Recommender validate, recommend.py handles --explain / --explain-top /
--explain-space / --explain-metric / --why, the TSV / npz writers on a hand-made table, and the numpy reference the GPU tests lean on
against a plain loop on ragged histories."""
import ctypes as C
import os

import numpy as np
import pytest

import explain_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32 = C.c_void_p, C.c_int32
    args = [vp, i32, i32, C.POINTER(cabi.ltg_batch), i32, i32, i32, vp, i32, i32, vp, vp, vp]
    assert cabi.SYMBOLS["ltg_topk_explain"] == (C.c_int, args)
    assert lib.ltg_topk_explain.argtypes == args and lib.ltg_topk_explain.restype == C.c_int
    assert (cabi.LTG_WHY_MAX_TOP, cabi.LTG_WHY_MAX_R) == (256, 8) == (E.MAX_TOP, E.MAX_R)
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_WHY_MAX_TOP 256" in header and "#define LTG_WHY_MAX_R 8" in header and "#define LTG_ABI_VERSION 14" in header
    assert ("int ltg_topk_explain(const uint16_t* image, int32_t image_lo, int32_t image_rows, const ltg_batch* tr, int32_t hist_lo, "
            "int32_t n_rows,") in header
    kernel = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_explain.h")).read()
    assert "constexpr int EX_HB = %d;" % E.HB in kernel                  # the block the GPU tests' histories straddle


def test_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    img = (C.c_uint16 * (608 * 4 + 8))()
    base = C.addressof(img)
    base += (-base) % 16                                                # the image is read by 16-byte loads
    buf = (C.c_float * 1024)()
    ib = (C.c_int32 * 1024)()
    ptr = (C.c_int32 * 8)()

    def batch(n_rows=2, indptr=True, indices=True):
        return cabi.ltg_batch(n_rows, 0, C.addressof(ptr) if indptr else None, C.addressof(ptr) if indices else None, None, None, None, None,
                              None, None, None)

    def call(image=base, lo=0, rows=4, tr=batch(), hist_lo=0, n=2, k_in=8, ii=ib, top=4, r=3, so=buf, io=ib):
        return lib.ltg_topk_explain(image, lo, rows, C.byref(tr) if tr is not None else None, hist_lo, n, k_in, ii, top, r, so, io, None)

    for name in ("image", "tr", "ii", "so", "io"):
        assert call(**{name: None}) == -1, name
    assert call(tr=batch(indptr=False)) == -1 and call(tr=batch(indices=False)) == -1
    assert call(tr=batch(n_rows=3)) == -1 and call(n=3) == -1           # tr->n_rows != n_rows
    assert call(n=-1, tr=batch(n_rows=-1)) == -1
    for k_in in (0, -1, 1025):
        assert call(k_in=k_in, top=1) == -1, k_in
    for top in (0, -1, 9):
        assert call(top=top) == -1, top
    assert call(k_in=1024, top=257) == -1 and call(k_in=300, top=256, n=0, tr=batch(n_rows=0)) == 0
    for r in (0, -1, 9):
        assert call(r=r) == -1, r
    assert call(rows=0) == -1 and call(rows=-3) == -1
    assert call(lo=-1) == -1 and call(hist_lo=-1) == -1
    assert call(image=base + 2) == -1                                   # not 16-byte aligned
    assert call(n=0, tr=batch(n_rows=0)) == 0                           # zero rows: nothing to launch
    assert call(n=0, tr=batch(n_rows=0), r=9) == -1 and call(n=0, tr=batch(n_rows=0), top=9) == -1     # ... the arguments are still checked


class _FakeEngine:
    I, I_global, device = 50, 50, "cpu"


def test_explain_validation():
    from ltgan.serving import SlabLists
    from ltgan.sharded import Explain as ShardedExplain
    from ltgan.trainer import Explain, Recommender
    assert ShardedExplain is Explain
    for r in (0, -1, 9):
        with pytest.raises(ValueError):
            Explain(r)
    for top in (0, -2, 257):
        with pytest.raises(ValueError):
            Explain(3, top=top)
    with pytest.raises(ValueError):
        Explain(3, space="items")
    with pytest.raises(ValueError):
        Explain(3, metric="l2")
    x = Explain()
    assert (x.r, x.space, x.metric) == (3, "decoder", "cosine")
    x.bind(_FakeEngine(), 20, 33)
    assert x.top == 20 and tuple(x.why_s.shape) == tuple(x.why_i.shape) == (33, 20, 3)
    x.bind(_FakeEngine(), 1000, 5)
    assert x.top == 256                                                 # min(k, 256)
    x = Explain(8, top=10, space="encoder", metric="dot")
    x.bind(_FakeEngine(), 10, 5)
    assert (x.top, x.r) == (10, 8) and x.why_i.dtype.is_floating_point is False
    with pytest.raises(ValueError):
        Explain(3, top=21).bind(_FakeEngine(), 20, 5)                   # top > k
    x = Explain(3)
    x.r = 9
    with pytest.raises(ValueError):
        x.bind(_FakeEngine(), 20, 5)
    with pytest.raises(ValueError):                                     # refused before anything of the engine is touched
        Recommender(_FakeEngine(), None, k=0, explain=Explain())
    lists = SlabLists(_FakeEngine(), rows=10, longest=20 * 3, parts=2)  # top * r floats per row serve the [rows * top, r] lists
    ls, li = lists.local(7 * 20, 3, None, None)
    assert tuple(ls.shape) == tuple(li.shape) == (140, 3) and ls.is_contiguous()


def test_cli_arguments():
    from ltgan import recommend as rc
    a = rc.parse_args(["ds", "model.pt"])                                # nothing changes without the option
    assert (a.explain, a.explain_top, a.explain_space, a.explain_metric, a.why) == (None, None, None, None, None)
    a = rc.parse_args(["ds", "m.pt", "--explain", "3"])
    assert (a.explain, a.explain_top, a.why) == (3, None, "why.tsv")
    a = rc.parse_args(["ds", "m.pt", "--k", "20", "--explain", "8", "--explain-top", "20", "--explain-space", "encoder", "--explain-metric",
                       "dot", "--why", "w.tsv", "--diversify", "0.5"])
    assert (a.explain, a.explain_top, a.explain_space, a.explain_metric, a.why, a.diversify) == (8, 20, "encoder", "dot", "w.tsv", 0.5)
    for bad in (["--explain", "0"], ["--explain", "9"], ["--explain", "x"], ["--explain-top", "5"], ["--why", "w.tsv"],
                ["--explain-space", "encoder"], ["--explain-metric", "dot"], ["--explain", "3", "--explain-top", "0"],
                ["--explain", "3", "--explain-top", "101"], ["--k", "300", "--explain", "3", "--explain-top", "257"],
                ["--explain", "3", "--explain-space", "items"], ["--explain", "3", "--explain-metric", "l2"]):
        with pytest.raises(SystemExit) as e:
            rc.parse_args(["ds", "m.pt"] + bad)
        assert e.value.code == 2, bad
    assert rc.parse_args(["ds", "m.pt", "--k", "300", "--explain", "3", "--explain-top", "256"]).explain_top == 256


def test_writers_on_a_hand_made_table(tmp_path):
    from ltgan import recommend as rc
    ids = np.array([[5, 9, 4], [7, -1, 2]], np.int32)
    sc = np.array([[3.0, 2.0, 1.0], [1.5, -np.inf, 0.5]], np.float32)
    inf = -np.inf
    why_i = np.array([[[1, 2], [3, -1]], [[-1, -1], [8, 6]]], np.int32)           # top = 2, r = 2; user 1's second entry is padding
    why_s = np.array([[[0.75, -0.5], [1.0 / 3.0, inf]], [[inf, inf], [9.0, 9.0]]], np.float32)
    path = str(tmp_path / "why.tsv")
    assert rc.write_why(why_i, why_s, ids, 40, path) == (3, 3)
    assert open(path).read() == "40\t5\t1:0.75,2:-0.5\n40\t9\t3:0.333333\n41\t7\t\n"
    npz = str(tmp_path / "recs.npz")
    rc.write_recs(ids, sc, 40, str(tmp_path / "recs.tsv"), npz, why=(why_i, why_s))
    z = np.load(npz)
    assert sorted(z.files) == ["ids", "scores", "uids", "why_ids", "why_scores"]
    assert np.array_equal(z["why_ids"], why_i) and z["why_ids"].dtype == np.int32
    assert np.array_equal(z["why_scores"], why_s) and z["why_scores"].dtype == np.float32
    rc.write_recs(ids, sc, 40, None, npz)                                # without an explanation the npz is what it was
    assert sorted(np.load(npz).files) == ["ids", "scores", "uids"]
    assert open(str(tmp_path / "recs.tsv")).read() == "40\t5,9,4\n41\t7,2\n"


@pytest.mark.parametrize("image_lo", [0, 13])
def test_reference_equals_the_plain_loop_on_ragged_histories(image_lo):
    img = E.exact_image()
    hit_self = outside = ties = 0
    for k_in, top, r in [(20, 16, 3), (100, 17, 8), (30, 30, 1)]:
        ids, indptr, indices = E.exact_inputs(k_in, top, r, img.shape[0], image_lo, rows=12)
        got_s, got_i = E.explain_lists(img, image_lo, ids, indptr, indices, 0, top, r)
        want_s, want_i = E.explain_loop(img, image_lo, ids, indptr, indices, 0, top, r)
        assert np.array_equal(got_i, want_i), (k_in, top, r)
        assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
        s7, i7 = E.explain_lists(img, image_lo, ids, indptr, indices - 7, 7, top, r)      # the history's base moves nothing
        assert np.array_equal(i7, got_i) and np.array_equal(s7.view(np.uint32), got_s.view(np.uint32))
        # the inputs discriminate: a history holds entries of its own list, ids outside the image occur, and the tie rule decides
        h = indices[indptr[E.ROW_SELF]:indptr[E.ROW_SELF + 1]]
        mine = np.isin(ids[E.ROW_SELF, :top], h)
        hit_self += int(mine.sum())
        for e in np.nonzero(mine)[0]:
            assert ids[E.ROW_SELF, e] not in got_i[E.ROW_SELF, e]
        outside += int(((indices < image_lo) | (indices >= image_lo + img.shape[0])).sum())
        assert (got_i[E.ROW_EMPTY] == -1).all() and (got_i[E.ROW_STRAY, min(1, top - 1)] == -1).all()
        assert (got_i[E.ROW_MINUS1, top // 2] == -1).all() and (got_i[E.ROW_MINUS1, top // 2 + 1:, 0] >= 0).all()
        assert (got_i[0] == -1).all()                                    # an empty history
        if r > 1:
            ties += int((got_s[:, :, 1:] == got_s[:, :, :-1])[got_i[:, :, 1:] >= 0].sum())
        flat = got_i.reshape(-1, r)
        for u in range(12):                                              # every reason is a history item of its user
            hu = set(indices[indptr[u]:indptr[u + 1]].tolist())
            assert set(got_i[u][got_i[u] >= 0].tolist()) <= hu
        assert ((flat[:, 1:] == -1) | (flat[:, :-1] >= 0)).all()         # padding only at the end
    assert hit_self >= 3 and outside >= 3 and ties > 50, (hit_self, outside, ties)
