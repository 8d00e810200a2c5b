"""CPU-side checks of the niche companions: the numpy reference the GPU tests compare against (tests/companions_ref.py) IS the oracle's
discriminator tower without dropout, its list order is ltg_topk's, the four entry points are exported and answer bad arguments before any
HIP call, and companions.py's argument handling, side split and writers work on hand-made tables."""
import ctypes as C
import os

import numpy as np
import pytest

import companions_ref as CR
from oracle import ltg_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -2


def _cfg(cabi, hs=(100, 150, 250, 300), feat=1000):
    return cabi.ltg_config(feat, 600, 200, feat, *hs, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("hs,scale", [((16, 24, 40, 37), 1.0), ((100, 150, 250, 300), 1.0), ((16, 24, 40, 37), 2.0), ((8, 5, 9, 3), 4.0)])
def test_pack_ref_and_score_ref_are_the_oracle_tower_without_dropout(hs, scale):
    """scale: emb, w1 .. w4 multiplied as tests/helpers.hot_discriminator does (2 = a trained model's range); the biases are made non-zero"""
    rng = np.random.default_rng(hs[3])
    F, n = 500, 400
    D = O.init_discriminator(F, *hs, seed=7)
    for key in ("emb", "w1", "w2", "w3", "w4"):
        D[key] = D[key] * scale
    for key in ("b1", "b2", "b3", "b4"):
        D[key] = rng.normal(0, 0.1, np.shape(D[key]))
    a, b = rng.integers(0, F, n), rng.integers(0, F, n)
    ones = [np.ones((n, w)) for w in hs[1:]]
    want = O.d_tower(D, a, b, ones, 1.0)["s"]
    xa, xb = CR.pack_ref(D, "popular", a), CR.pack_ref(D, "niche", b)
    assert xa.shape == xb.shape == (n, hs[3]) and max(np.abs(xa).max(), np.abs(xb).max()) < CR.CLAMP
    got = CR.score_ref(CR.image_ref(xa), CR.image_ref(xb), D["w4"], D["b4"])
    assert np.abs(np.diag(got) - want).max() <= 1e-12
    assert np.abs(got[3, :50] - O.d_tower(D, np.full(50, a[3]), b[:50], [m[:50] for m in ones], 1.0)["s"]).max() <= 1e-12
    # the sides commute: niche queries over popular candidates is the transposed table
    assert np.abs(CR.score_ref(CR.image_ref(xb[:20]), CR.image_ref(xa[:30]), D["w4"], D["b4"]) - got[:30, :20].T).max() <= 1e-12


def test_image_ref_clamps_and_score_ref_saturates():
    x = np.array([[-1000.0, -40.0, 0.0, 40.0, 1000.0]])
    E = CR.image_ref(x)
    assert np.array_equal(E, np.exp([[-80.0, -80.0, 0.0, 80.0, 80.0]])) and np.all(np.isfinite(E.astype(np.float32))) and np.all(E.astype(np.float32) > 0)
    w4 = np.arange(1.0, 6.0)
    s = CR.score_ref(E, E, w4, [0.5])
    assert abs(s[0, 0] - (0.5 + np.tanh([-80.0, -80.0, 0.0, 80.0, 80.0]) @ w4)) < 1e-12
    assert np.array_equal(CR.score_ref(np.hstack([E, [[7.0, 9.0]]]), np.hstack([E, [[np.nan, 0.0]]]), w4, [0.5]), s)     # columns past h3 are not read


def test_lists_ref_order_and_padding():
    S = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, 2.0],
                  [5.0, 5.0, 5.0, 5.0, 5.0, 5.0]], np.float32)
    c_gid = np.array([2, 4, 7, 9, 11, 30])
    sc, ids = CR.lists_ref(S, np.array([7, -1]), c_gid, 4)
    assert ids.tolist() == [[4, 30, 2, 9], [2, 4, 7, 9]] and ids.dtype == np.int32          # 7 is the first query itself; -0.0 ties +0.0, lower id first
    assert sc.tolist() == [[3.0, 2.0, 1.0, 0.0], [5.0] * 4] and np.signbit(sc[0, 3]) and sc.dtype == np.float32
    sc, ids = CR.lists_ref(S, np.array([7, 30]), c_gid, 8)                                   # fewer eligible than k: padded
    assert ids.tolist() == [[4, 30, 2, 9, 11, -1, -1, -1], [2, 4, 7, 9, 11, -1, -1, -1]]
    assert np.all(np.isneginf(sc[:, 5:])) and np.all(np.isfinite(sc[:, :5]))
    sc, ids = CR.lists_ref(S[:, :0], np.array([7, 30]), c_gid[:0], 3)                        # no candidates at all
    assert np.all(ids == -1) and np.all(np.isneginf(sc))
    # against a plain loop on random ties
    rng = np.random.default_rng(0)
    S = rng.integers(-2, 3, (5, 40)).astype(np.float64)
    c_gid = np.sort(rng.choice(1000, 40, replace=False))
    q = np.array([c_gid[3], -1, c_gid[0], 5000, c_gid[39]])
    sc, ids = CR.lists_ref(S, q, c_gid, 10)
    for r in range(5):
        cand = sorted(((-S[r, c], int(c_gid[c])) for c in range(40) if c_gid[c] != q[r]))[:10]
        assert ids[r].tolist() == [g for _, g in cand] and sc[r].tolist() == [-s for s, _ in cand]


# ---------------------------------------------------------------------------------------------- the entry points, without a GPU
def check_refusals(cabi, lib, p, ids_p=None):
    """every LTG_EINVAL / LTG_EWORKSPACE case of include/ltg.h, answered before any HIP call: `p` is any non-NULL address (never read)"""
    ids_p = p if ids_p is None else ids_p
    cfg = _cfg(cabi)
    disc = cabi.ltg_disc_state()
    disc.emb = p
    for i in range(8):
        disc.p[i] = p
    assert lib.ltg_pair_ld(C.byref(cfg)) == 300 and lib.ltg_pair_ld(C.byref(_cfg(cabi, (16, 24, 40, 37)))) == 40
    assert lib.ltg_pair_ld(C.byref(_cfg(cabi, (1, 1, 1, 1)))) == 4 and lib.ltg_pair_ld(C.byref(_cfg(cabi, (100, 150, 250, 352)))) == 352
    bad = [_cfg(cabi, (100, 150, 250, 353)), _cfg(cabi, (100, 150, 250, 0)), _cfg(cabi, (0, 150, 250, 300)), _cfg(cabi, (100, 150, 250, 300), feat=0),
           _cfg(cabi, (1024, 1025, 250, 300)), _cfg(cabi, (1024, 250, 1025, 300))]
    assert lib.ltg_pair_ld(None) == 0 and all(lib.ltg_pair_ld(C.byref(c)) == 0 for c in bad)
    assert lib.ltg_pair_ld(C.byref(_cfg(cabi, (1024, 1024, 1024, 300)))) == 300

    def pack(cfg=cfg, disc=disc, side=0, ids=ids_p, n=4, out=p):
        return lib.ltg_pair_pack(C.byref(cfg) if cfg is not None else None, C.byref(disc) if disc is not None else None, side, ids, n, out, None)
    assert pack(cfg=None) == EINVAL and pack(disc=None) == EINVAL and pack(ids=None) == EINVAL and pack(out=None) == EINVAL
    assert pack(side=2) == EINVAL and pack(side=-1) == EINVAL and pack(n=-1) == EINVAL
    assert all(pack(cfg=c) == EINVAL for c in bad)
    for i in range(6):                                   # a missing master tensor
        d2 = cabi.ltg_disc_state()
        d2.emb = p
        for j in range(8):
            d2.p[j] = None if j == i else p
        assert pack(disc=d2) == EINVAL, i
    no_emb = cabi.ltg_disc_state()
    for j in range(8):
        no_emb.p[j] = p
    assert pack(disc=no_emb) == EINVAL
    assert pack(n=0) == 0 and pack(n=0, side=1) == 0

    big = 1 << 40

    def ws_bytes(n_q=100, n_c=5000, k=20, cfg=cfg):
        return lib.ltg_pair_companions_ws_bytes(C.byref(cfg) if cfg is not None else None, n_q, n_c, k)

    def call(cfg=cfg, disc=disc, q=p, qg=ids_p, n_q=4, c=p, cg=ids_p, n_c=100, k=8, s=p, i=ids_p, ws=p, wsb=big):
        return lib.ltg_pair_companions(C.byref(cfg) if cfg is not None else None, C.byref(disc) if disc is not None else None, q, qg, n_q, c, cg, n_c,
                                       k, s, i, ws, wsb, None)
    assert ws_bytes() > 0 and ws_bytes(n_c=0) > 0
    assert ws_bytes(cfg=None) == 0 and ws_bytes(n_q=0) == 0 and ws_bytes(n_q=-1) == 0 and ws_bytes(n_c=-1) == 0
    assert ws_bytes(k=0) == 0 and ws_bytes(k=257) == 0 and all(ws_bytes(cfg=c) == 0 for c in bad)
    assert call(cfg=None) == EINVAL and call(disc=None) == EINVAL and all(call(cfg=c) == EINVAL for c in bad)
    for name in ("q", "qg", "c", "cg", "s", "i", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n_q=-1) == EINVAL and call(n_c=-1) == EINVAL and call(k=0) == EINVAL and call(k=257) == EINVAL
    for j in (6, 7):                                     # w4 / b4 missing
        d2 = cabi.ltg_disc_state()
        for t in range(8):
            d2.p[t] = None if t == j else p
        assert call(disc=d2) == EINVAL, j
    need = ws_bytes(4, 100, 8)
    assert call(wsb=need - 1) == EWORKSPACE and call(wsb=0) == EWORKSPACE
    assert call(n_q=0) == 0 and call(n_q=0, q=None, qg=None, s=None, i=None, ws=None, wsb=0) == 0          # n_q = 0: LTG_OK, nothing touched
    assert call(n_q=0, k=0) == EINVAL                    # (the ranges are still checked)
    return need


def test_pair_entry_points_are_exported_and_refuse_bad_arguments_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    for name in ("ltg_pair_ld", "ltg_pair_pack", "ltg_pair_companions_ws_bytes", "ltg_pair_companions"):
        assert name in cabi.SYMBOLS and getattr(lib, name).argtypes == cabi.SYMBOLS[name][1]
    assert lib.ltg_abi_version() == 14 and cabi.LTG_PAIR_MAX_K == 256 and cabi.LTG_PAIR_SIDE == {"popular": 0, "niche": 1}
    buf = (C.c_float * 16)()
    check_refusals(cabi, lib, C.cast(buf, C.c_void_p).value)
    assert not any(buf)


def test_the_workspace_is_lists_never_scores():
    """at most 64 segments x n_q x k (score, id) pairs: at config.ini's sizes and the 200 000-item catalogue a full chunk of 4 096 queries
    needs a few MB where the score table would be 2.9 GB"""
    from ltgan import _cabi as cabi
    lib = cabi.load()
    cfg = _cfg(cabi)
    for n_q, n_c, k in ((4096, 180000, 20), (1, 180000, 256), (130, 3001, 256), (17, 1, 1), (5, 0, 3)):
        need = lib.ltg_pair_companions_ws_bytes(C.byref(cfg), n_q, n_c, k)
        assert 0 < need <= 64 * n_q * k * 8 + 256 and need % 256 == 0, (n_q, n_c, k, need)
        assert need >= n_q * k * 8
    assert lib.ltg_pair_companions_ws_bytes(C.byref(cfg), 4096, 180000, 20) < 4096 * 180000 * 4 // 500


# ---------------------------------------------------------------------------------------------- companions.py
def test_cli_arguments():
    from ltgan import companions as CP
    a = CP.parse_args(["ds", "ck.pt"])
    assert (a.dataset_dir, a.checkpoint, a.k, a.items, a.out, a.npz) == ("ds", "ck.pt", 20, "popular", "companions.tsv", None)
    a = CP.parse_args(["ds", "ck.pt", "--k", "256", "--items", "niche", "--out", "o.tsv", "--npz", "o.npz"])
    assert (a.k, a.items, a.out, a.npz) == (256, "niche", "o.tsv", "o.npz")
    for bad in (["--k", "0"], ["--k", "257"], ["--items", "all"], []):
        with pytest.raises(SystemExit):
            CP.parse_args((["ds", "ck.pt"] if bad else ["ds"]) + bad)


def test_cli_side_split(tmp_path):
    from ltgan import companions as CP
    niche, valid, n = {1, 3, 5, 8}, {0, 1, 2, 3, 5, 6, 9}, 10          # 4 and 7 (popular) and 8 (niche) have no features
    side, q, c = CP.split_sides("popular", niche, valid, n)
    assert side == "popular" and q.tolist() == [0, 2, 6, 9] and c.tolist() == [1, 3, 5] and q.dtype == c.dtype == np.int32
    side, q, c = CP.split_sides("niche", niche, valid, n)
    assert side == "niche" and q.tolist() == [1, 3, 5] and c.tolist() == [0, 2, 6, 9]
    f = tmp_path / "q.txt"
    f.write_text("9\n4\n0\n")                                           # a file keeps its order; the item without features is dropped
    side, q, c = CP.split_sides(str(f), niche, valid, n)
    assert side == "popular" and q.tolist() == [9, 0] and c.tolist() == [1, 3, 5]
    f.write_text("5 8 1\n")
    side, q, c = CP.split_sides(str(f), niche, valid, n)
    assert side == "niche" and q.tolist() == [5, 1] and c.tolist() == [0, 2, 6, 9]
    f.write_text("5\n0\n")
    with pytest.raises(ValueError, match="mixes"):
        CP.split_sides(str(f), niche, valid, n)
    f.write_text("10\n")
    with pytest.raises(ValueError, match="outside"):
        CP.split_sides(str(f), niche, valid, n)


def test_cli_writers_and_summary(tmp_path):
    from ltgan import companions as CP
    items = np.array([4, 9, 2], np.int32)
    ids = np.array([[7, 1, -1], [1, 7, 3], [-1, -1, -1]], np.int32)
    scores = np.array([[0.0, -2.0, -np.inf], [3.0, 1.0, -30.0], [-np.inf] * 3], np.float32)
    tsv, npz = str(tmp_path / "c.tsv"), str(tmp_path / "c.npz")
    CP.write_companions(items, ids, scores, tsv, npz)
    lines = open(tsv).read().splitlines()
    assert lines == ["4\t7:0.500000,1:0.119203", "9\t1:0.952574,7:0.731059,3:0.000000", "2\t"]
    z = np.load(npz)
    assert np.array_equal(z["items"], items) and np.array_equal(z["ids"], ids) and np.array_equal(z["scores"], scores)
    assert z["scores"].dtype == np.float32 and z["ids"].dtype == np.int32
    m = CP.companions_summary(ids, scores, 6)
    assert m["items"] == 3 and m["coverage"] == 3 / 6 and abs(m["mean_prob"] - (0.5 + 1 / (1 + np.exp(-3.0))) / 2) < 1e-12
    line = CP.summary_line(m, 3)
    assert line.startswith("items: 3\tcoverage@3: 0.500000\tmean_prob@1: 0.726287")
    f = dict(x.split(": ") for x in line.split("\t"))
    assert set(f) == {"items", "coverage@3", "mean_prob@1"}
    empty = CP.companions_summary(np.full((2, 3), -1, np.int32), np.full((2, 3), -np.inf, np.float32), 0)
    assert empty["items"] == 2 and np.isnan(empty["coverage"]) and np.isnan(empty["mean_prob"])
