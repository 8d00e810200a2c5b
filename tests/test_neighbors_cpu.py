"""CPU-side checks of the item-to-item neighbours: the three entry points are exported and bound, their argument validation answers before
any HIP call, the workspace is lists and never a block of the score matrix, similar.py's argument handling and writers work on hand-made
tables, and the numpy reference the GPU tests compare against (tests/neighbors_ref.py) agrees with a plain loop."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbors_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -2


def _cfg(cabi, n_items=1000, item_lo=0, n_glob=0, h=600):
    return cabi.ltg_config(n_items, h, 200, n_items, 100, 150, 250, 300, 0, 0, item_lo, n_glob, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


def test_neighbor_entry_points_are_exported_and_bound():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    for name in ("ltg_item_pack", "ltg_item_neighbors_ws_bytes", "ltg_item_neighbors"):
        assert name in cabi.SYMBOLS
        assert getattr(lib, name).argtypes == cabi.SYMBOLS[name][1]
    assert lib.ltg_abi_version() == 14 and cabi.LTG_NBR_MAX_K == 256


def test_item_pack_argument_validation_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    cfg = _cfg(cabi)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    gen = cabi.ltg_gen_state()
    gen.p[0] = gen.p[3] = p.value
    assert lib.ltg_item_pack(None, C.byref(gen), 0, 0, p, None) == EINVAL
    assert lib.ltg_item_pack(C.byref(cfg), None, 0, 0, p, None) == EINVAL
    assert lib.ltg_item_pack(C.byref(cfg), C.byref(gen), 0, 0, None, None) == EINVAL
    for space, metric in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert lib.ltg_item_pack(C.byref(cfg), C.byref(gen), space, metric, p, None) == EINVAL, (space, metric)
    assert lib.ltg_item_pack(C.byref(_cfg(cabi, h=609)), C.byref(gen), 0, 0, p, None) == EINVAL
    empty = cabi.ltg_gen_state()                      # the table of the chosen space is missing
    assert lib.ltg_item_pack(C.byref(cfg), C.byref(empty), 0, 0, p, None) == EINVAL
    assert lib.ltg_item_pack(C.byref(cfg), C.byref(empty), 1, 1, p, None) == EINVAL


def test_item_neighbors_argument_validation_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    cfg = _cfg(cabi)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40

    def call(cfg=cfg, table=p, q=p, gid=p, n_q=4, labels=None, mask=0x1FF, k=8, s=p, i=p, ws=p, ws_bytes=big):
        return lib.ltg_item_neighbors(C.byref(cfg) if cfg is not None else None, table, q, gid, n_q, labels, mask, k, s, i, ws, ws_bytes, None)

    for name in ("cfg", "table", "q", "gid", "s", "i", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n_q=-1) == EINVAL
    for k in (0, -1, 257):
        assert call(k=k) == EINVAL, k
    for mask in (0, 0x200, 0xFFFFFFFF):
        assert call(labels=p, mask=mask) == EINVAL, mask
        assert call(labels=None, mask=mask, n_q=0) == 0              # without labels the mask is not looked at
    assert call(cfg=_cfg(cabi, 1000, item_lo=-1, n_glob=5000)) == EINVAL
    assert call(cfg=_cfg(cabi, 1000, item_lo=4001, n_glob=5000)) == EINVAL
    assert call(cfg=_cfg(cabi, 1000, item_lo=1, n_glob=0)) == EINVAL   # n_items_global = 0: unsharded, the slab is the catalogue
    assert call(cfg=_cfg(cabi, h=609)) == EINVAL
    # the workspace: one byte short is refused, n_q = 0 is a no-op that needs none
    need = lib.ltg_item_neighbors_ws_bytes(C.byref(cfg), 4, 8)
    assert need > 0
    assert call(ws_bytes=need - 1) == EWORKSPACE
    assert call(n_q=0, ws=None, ws_bytes=0) == 0
    # arguments the call refuses need no workspace
    assert lib.ltg_item_neighbors_ws_bytes(C.byref(cfg), 4, 257) == 0
    assert lib.ltg_item_neighbors_ws_bytes(C.byref(_cfg(cabi, h=609)), 4, 8) == 0
    assert lib.ltg_item_neighbors_ws_bytes(None, 4, 8) == 0


def test_workspace_is_lists_not_scores():
    """'fused' as a condition: at 200 000 items, 4 096 queries, k = 100 the workspace is below a quarter of the 3.28 GB those queries' fp32
    scores would occupy, it is a whole number of (n_q x k) lists -- the segments --, and doubling the items grows it by no more than the
    number of segments grows (which at most doubles)."""
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n_q, k = 4096, 100
    ws = {I: lib.ltg_item_neighbors_ws_bytes(C.byref(_cfg(cabi, I)), n_q, k) for I in (200000, 400000)}
    scores = 200000 * n_q * 4
    assert scores == 3276800000
    assert 0 < ws[200000] < scores // 4
    per_list = n_q * k * 8                          # one (score, id) list per query row
    seg = {I: -(-w // per_list) for I, w in ws.items()}
    for I, w in ws.items():
        assert (seg[I] - 1) * per_list < w <= seg[I] * per_list + 256 and 1 <= seg[I] <= 64, (I, w, seg[I])
    assert seg[400000] <= 2 * seg[200000]
    assert ws[400000] <= ws[200000] * seg[400000] // seg[200000] + 256
    # few queries: more segments (the grid fills the chip), still lists
    w1 = lib.ltg_item_neighbors_ws_bytes(C.byref(_cfg(cabi, 200000)), 1, 256)
    assert 0 < w1 <= 64 * 256 * 8 + 256


def test_chunked_walk_sizes_its_workspace_for_every_chunk_length():
    """the need is not monotone in n_q (fewer query blocks get more segments): a walk in chunks sizes the workspace for the lengths that
    occur, a ragged last chunk included -- at the catalogue sizes the feature is written for"""
    from ltgan import _cabi as cabi
    from ltgan.trainer import neighbors_ws_bytes
    lib = cabi.load()
    seen_more = False
    for I in (25000, 100000, 200000, 1000000):
        cfg = _cfg(cabi, I)
        for k in (20, 100, 256):
            ws = lambda n, kk: lib.ltg_item_neighbors_ws_bytes(C.byref(cfg), n, kk)
            for n_total, chunk in ((I, 4096), (200000, 4096), (4096 + 3392, 4096), (4064, 4096), (5000, 1500), (7, 4096), (8192, 4096)):
                have = neighbors_ws_bytes(ws, n_total, chunk, k)
                for lo in range(0, n_total, chunk):
                    n = min(chunk, n_total - lo)
                    assert ws(n, k) <= have, (I, k, n_total, chunk, n)
                assert have <= max(ws(n, k) for n in range(1, min(chunk, n_total) + 1, 37)) + ws(min(chunk, n_total), k)   # lists, not scores
            seen_more = seen_more or ws(3392, k) > ws(4096, k)
    assert seen_more, "the case this test exists for: a shorter chunk that needs more than a full one"
    assert neighbors_ws_bytes(lambda n, k: 0, 0, 4096, 20) == 1


def _sim():
    from ltgan import similar
    return similar


def test_similar_cli_arguments():
    sm = _sim()
    a = sm.parse_args(["ds", "model.pt"])
    assert (a.dataset_dir, a.checkpoint, a.k, a.space, a.metric, a.items, a.groups, a.only, a.out, a.npz) == \
        ("ds", "model.pt", 20, "decoder", "cosine", "all", "niche", None, "similar.tsv", None)
    assert a.only_groups is None
    a = sm.parse_args(["ds", "m.pt", "--k", "256", "--space", "encoder", "--metric", "dot", "--items", "popular", "--groups", "niche",
                       "--only", "niche", "--out", "o.tsv", "--npz", "o.npz"])
    assert (a.k, a.space, a.metric, a.items, a.only_groups, a.out, a.npz) == (256, "encoder", "dot", "popular", [1], "o.tsv", "o.npz")
    a = sm.parse_args(["ds", "m.pt", "--groups", "pop:4", "--only", "pop3,pop1"])
    assert (a.group_kind, a.n_groups, a.only_groups) == ("pop", 4, [1, 3])
    for bad in (["ds", "m.pt", "--k", "0"], ["ds", "m.pt", "--k", "257"], ["ds", "m.pt", "--space", "user"], ["ds", "m.pt", "--metric", "l2"],
                ["ds", "m.pt", "--only", "head"], ["ds", "m.pt", "--only", "niche,niche"], ["ds", "m.pt", "--groups", "pop:9"], ["ds"]):
        with pytest.raises(SystemExit):
            sm.parse_args(bad)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "long-tail-gan_amd", "similar.py"), "ds", "m.pt", "--k", "1000"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--k must be in [1, 256]" in out.stderr


def test_similar_query_items_writers_and_summary(tmp_path):
    sm = _sim()
    n_items = 12
    niche = {2, 3, 7, 11}
    assert sm.query_items("all", niche, n_items).tolist() == list(range(12))
    assert sm.query_items("niche", niche, n_items).tolist() == [2, 3, 7, 11]
    assert sm.query_items("popular", niche, n_items).tolist() == [0, 1, 4, 5, 6, 8, 9, 10]
    f = tmp_path / "q.txt"
    f.write_text("5\n3\n11\n")
    q = sm.query_items(str(f), niche, n_items)
    assert q.dtype == np.int32 and q.tolist() == [5, 3, 11]
    f.write_text("5\n12\n")
    with pytest.raises(ValueError):
        sm.query_items(str(f), niche, n_items)
    ids = np.array([[7, 3, 1], [0, 2, -1], [-1, -1, -1]], np.int32)
    scores = np.array([[0.9, 0.5, -0.25], [0.5, -0.0, -np.inf], [-np.inf] * 3], np.float32)
    sm.write_similar([5, 3, 11], ids, scores, str(tmp_path / "s.tsv"), str(tmp_path / "s.npz"))
    assert open(tmp_path / "s.tsv").read().splitlines() == ["5\t7,3,1", "3\t0,2", "11\t"]          # padding is not an item
    z = np.load(tmp_path / "s.npz")
    assert z["items"].tolist() == [5, 3, 11] and z["items"].dtype == np.int32 and np.array_equal(z["ids"], ids) and z["ids"].dtype == np.int32
    assert z["scores"].dtype == np.float32 and np.array_equal(z["scores"].view(np.uint32), scores.view(np.uint32))
    m = sm.similar_summary(ids, niche, n_items)
    assert m["items"] == 3 and m["niche_share"] == pytest.approx(3 / 5) and m["coverage"] == pytest.approx(5 / 12)
    assert sm.summary_line(m, 3) == "items: 3\tniche_share@3: 0.600000\tcoverage@3: 0.416667"
    assert np.isnan(sm.similar_summary(ids[2:], niche, n_items)["niche_share"])


def test_group_mask_of():
    from ltgan.trainer import group_mask_of
    assert group_mask_of(None, 2) == 0x1FF
    assert group_mask_of([1], 2) == 0b10 and group_mask_of([0, 3], 4) == 0b1001
    for bad in ([], [2], [-1]):
        with pytest.raises(ValueError):
            group_mask_of(bad, 2)


def test_reference_image_rounding_and_norms():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e-5, 65280.0, 0.0], np.float32)      # 1 + 2^-8 ties to even (down), 1 + 3 * 2^-8 up
    b = NR.f32_to_bf16(x)
    assert b[:3].tolist() == [0x3F80, 0x3F80, 0x3F82]
    assert np.all(np.abs(NR.bf16_to_f32(b) - x) <= np.abs(x) * 2.0 ** -8)
    rng = np.random.default_rng(0)
    W = rng.standard_normal((9, 40)).astype(np.float32) * np.float32(10.0) ** rng.integers(-12, 12, (9, 1)).astype(np.float32)
    W[4] = 0
    img = NR.pack_image(W, "cosine")
    assert img.shape == (9, 608) and img.dtype == np.uint16 and not img[:, 40:].any() and not img[4].any()
    n = np.sqrt((NR.bf16_to_f32(img).astype(np.float64) ** 2).sum(1))
    assert np.all(np.abs(np.delete(n, 4) - 1) < 2.0 ** -8)
    assert np.array_equal(NR.pack_image(W, "dot")[:, :40], NR.f32_to_bf16(W))
    S, B = NR.scores64(img, img), NR.score_bound(img, img)
    assert np.all(B <= 7.3e-5) and np.all(np.abs(S) <= 1 + 2.0 ** -7)


@pytest.mark.parametrize("k", [1, 5, 40])
def test_reference_lists_equal_a_brute_force_loop(k):
    """ties at every level (scores from a few multiples of 0.25, signed zeros), self-exclusion on and off, a group mask that leaves
    fewer than k eligible items, a slab with item_lo > 0"""
    rng = np.random.default_rng(k)
    n_q, I, item_lo, n_glob = 7, 33, 10, 60
    S = (rng.integers(-3, 4, (n_q, I)) * 0.25).astype(np.float32)
    S[2, ::3] = -0.0
    S[3] = 1.5
    S[4, 5] = -np.inf
    labels = rng.integers(0, 11, n_glob).astype(np.uint8)
    labels[item_lo:item_lo + I][rng.random(I) < 0.8] = 9          # most of the slab in the catch-all bit
    for q_gid in (np.full(n_q, -1, np.int32), (item_lo + rng.integers(0, I, n_q)).astype(np.int32), np.arange(n_q, dtype=np.int32)):
        for lab, mask in ((None, 0x1FF), (labels, 0x1FF), (labels, 0x0FF), (labels, 0x100), (labels, 0b101)):
            got = NR.topk_lists(S, NR.eligible(I, item_lo, q_gid, lab, mask), k, item_lo)
            want = NR.brute_force(S, q_gid, k, lab, mask, item_lo)
            assert np.array_equal(got[1], want[1]), (k, mask)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (k, mask)
            n_el = NR.eligible(I, item_lo, q_gid, lab, mask).sum(1)
            assert np.array_equal((got[1] >= 0).sum(1), np.minimum(n_el, k))
            for r in range(n_q):
                v = got[1][r][got[1][r] >= 0]
                assert len(set(v.tolist())) == v.size and q_gid[r] not in v.tolist()
