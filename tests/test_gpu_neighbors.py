"""Item-to-item neighbours on the GPU (ltg_item_pack / ltg_item_neighbors): the operand image against numpy bit for bit, the lists
against numpy's order bit for bit on tables whose scores are exact in fp32 (heavy ties), against the fp64 oracle of the device's own image
within the derived accumulation bound on real-valued tables, ragged slabs merged with ltg_topk_merge against the whole table bit for bit,
run-to-run identity, and the host layer: ItemNeighbors, similar.py and the item-sharded ShardedItemNeighbors
(tests/dist_neighbors_worker.py).  The reference is tests/neighbors_ref.py."""
import os

import numpy as np
import pytest

import neighbors_ref as NR
from serving_harness import _nbr_dev, _pack_dev, _small_engine, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu


def _u16(img):
    return img.cpu().numpy().view(np.uint16)


def _eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 1. the image
@pytest.mark.parametrize("H", [600, 100, 37])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_item_pack_equals_numpy_bit_for_bit(H, metric):
    rng = np.random.default_rng(H)
    I = 3001
    W = rng.standard_normal((I, H)).astype(np.float32)
    W *= (np.float32(10.0) ** rng.integers(-12, 12, (I, 1)).astype(np.float32))          # rows of very different magnitude
    W[17] = 0                                                                             # a zero row
    W[18, 1:] = 0                                                                         # a single entry
    W[19] = np.float32(1e-30) * rng.standard_normal(H).astype(np.float32)                 # squares below fp32's range: the norm is fp64
    for space in ("decoder", "encoder"):
        got = _u16(_pack_dev(W, metric, space))
        want = NR.pack_image(W, metric)
        assert not got[:, H:].any(), "K padding must be zero"
        assert not got[17].any()
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (space, bad[:10], got[bad[:1]], want[bad[:1]])


def test_item_pack_of_an_engine_equals_its_shadow_and_numpy():
    import torch
    eng = _small_engine(I=8192, steps=3)          # (8 192 items: an engine that keeps the bf16 shadow and the lazy clock)
    assert eng.g_shadow is not None
    img = eng.item_pack("decoder", "dot")
    torch.cuda.synchronize()
    assert torch.equal(img, eng.g_shadow), "decoder / dot must be ltg_refresh_shadow's image"
    for space, p in (("decoder", 3), ("encoder", 0)):
        for metric in ("cosine", "dot"):
            got = _u16(eng.item_pack(space, metric))          # (encoder: flushes the lazy clock first)
            want = NR.pack_image(eng.g_p[p].cpu().numpy(), metric)
            assert np.array_equal(got, want), (space, metric)


# ---------------------------------------------------------------------------------------------- 2. exact order
def _quarter_table(rng, I):
    """entries from the multiples of 0.25 in [-2, 2]: bf16 holds them exactly, and every product and every partial sum of 608 of them is
    exact in fp32 under any summation order"""
    return (rng.integers(-8, 9, (I, 600)) * 0.25).astype(np.float32)


@pytest.mark.parametrize("n_q", [1, 77, 300])
@pytest.mark.parametrize("I", [1000, 4099, 70001])
def test_exact_order_equals_numpy_lexsort(I, n_q):
    """metric dot, exact scores, heavy ties: the lists are numpy's lexsort((id, -score)) bit for bit -- k in {1, 20, 256}, self-exclusion on
    and off, group masks (one leaves fewer than k eligible items), a slab with item_lo > 0.  70 001 items span several segments and end in a
    ragged tile."""
    rng = np.random.default_rng(I + n_q)
    W = _quarter_table(rng, I)
    W[rng.integers(0, I, 40)] = W[3]                       # whole duplicate rows: equal scores against every query
    table = _pack_dev(W, "dot")
    t_host = _u16(table)
    assert np.array_equal(NR.bf16_to_f32(t_host[:, :600]), W)
    q_loc = rng.choice(I, n_q, replace=False).astype(np.int32)
    q_loc[0] = 3
    q_img = table[q_loc.astype(np.int64)].contiguous()
    S = W[q_loc] @ W.T                                     # exact in fp32
    assert np.array_equal(S.astype(np.float64), W[q_loc].astype(np.float64) @ W.astype(np.float64).T)
    item_lo, n_glob = 1234, 1234 + I + 50
    labels = rng.integers(0, 12, n_glob).astype(np.uint8)
    few = labels.copy()                                    # group 2: 11 items of the slab, fewer than k = 20 and 256
    few[few == 2] = 3
    few[item_lo + rng.choice(I, 11, replace=False)] = 2
    first = True
    for k in (1, 20, 256):
        for excl in (True, False):
            gid = q_loc if excl else np.full(n_q, -1, np.int32)
            got = _nbr_dev(table, q_img, gid, k)
            want = NR.neighbors(None, t_host, gid, k, scores=S)
            assert np.array_equal(got[1], want[1]) and _eq(got[0], want[0]), (I, n_q, k, excl)
            if first:                                      # the reference itself, once per case: numpy's lexsort row by row
                first = False
                for r in range(min(n_q, 3)):
                    ok = np.arange(I) != gid[r]
                    loc = np.nonzero(ok)[0]
                    o = loc[np.lexsort((loc, -S[r, loc]))[:k]]
                    assert np.array_equal(want[1][r, :len(o)], o) and np.all(want[1][r, len(o):] == -1)
        for lab, mask in ((few, 0b100), (labels, 0x1FE), (labels, 0x100)):
            gid = q_loc + item_lo
            got = _nbr_dev(table, q_img, gid, k, lab, mask, item_lo, n_glob)
            want = NR.neighbors(None, t_host, gid, k, lab, mask, item_lo, scores=S)
            assert np.array_equal(got[1], want[1]) and _eq(got[0], want[0]), (I, n_q, k, mask)
            if mask == 0b100 and k > 11:
                assert np.all((got[1] >= 0).sum(1) <= 11) and np.all(got[1][:, 11:] == -1) and np.all(np.isneginf(got[0][:, 11:]))


# ---------------------------------------------------------------------------------------------- 3. cosine on real-valued tables
def _check_against_oracle(table, q_img, gid, k, labels=None, mask=0x1FF, item_lo=0, n_glob=0):
    """every returned entry within the pair's bound of the fp64 oracle of the DEVICE image; every eligible item not returned at most the
    row's last returned score + 2 bounds; ids distinct, eligible, ordered by (device score desc, id asc).  -> the largest |score - oracle|"""
    got_s, got_i = _nbr_dev(table, q_img, gid, k, labels, mask, item_lo, n_glob)
    t_host, q_host = _u16(table), _u16(q_img)
    S, B = NR.scores64(q_host, t_host), NR.score_bound(q_host, t_host)
    ok = NR.eligible(t_host.shape[0], item_lo, gid, labels, mask)
    worst = 0.0
    for r in range(q_host.shape[0]):
        ids = got_i[r]
        n = int((ids >= 0).sum())
        assert n == min(k, int(ok[r].sum())), (r, n)
        assert np.all(ids[n:] == -1) and np.all(np.isneginf(got_s[r, n:]))
        loc = ids[:n].astype(np.int64) - item_lo
        assert np.all((loc >= 0) & (loc < t_host.shape[0])) and len(set(loc.tolist())) == n and np.all(ok[r, loc])
        sc = got_s[r, :n]
        assert np.all((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (ids[:n][:-1] < ids[:n][1:]))), r
        err = np.abs(sc.astype(np.float64) - S[r, loc])
        assert np.all(err <= B[r, loc]), (r, float(err.max()), float(B[r, loc].min()))
        worst = max(worst, float(err.max()) if n else 0.0)
        rest = ok[r].copy()
        rest[loc] = False
        if n and rest.any():
            assert np.all(S[r, rest] <= float(sc[-1]) + B[r, rest] + B[r, loc[-1]]), r
    return worst


def test_cosine_gaussian_rows_within_the_accumulation_bound(capsys):
    rng = np.random.default_rng(5)
    I, n_q = 20011, 256
    W = rng.standard_normal((I, 600)).astype(np.float32) * rng.uniform(0.01, 100.0, (I, 1)).astype(np.float32)
    W[11] = 0                                                       # a zero row: score 0 against everything, never NaN
    W[1000:1040] += 30 * W[7]                                       # a cluster of near neighbours of item 7
    table = _pack_dev(W, "cosine")
    q_loc = rng.choice(I, n_q, replace=False).astype(np.int32)
    q_loc[:2] = (7, 11)
    q_img = table[q_loc.astype(np.int64)].contiguous()
    worst = _check_against_oracle(table, q_img, q_loc, 50)
    labels = rng.integers(0, 4, I).astype(np.uint8)
    worst = max(worst, _check_against_oracle(table, q_img, q_loc, 200, labels, 0b0110))
    with capsys.disabled():
        print("\n[neighbors] gaussian rows: largest |score - fp64 oracle| = %.3e (bound for unit rows 7.3e-5)" % worst)
    assert worst <= 7.3e-5


@pytest.mark.parametrize("space", ["decoder", "encoder"])
def test_cosine_tables_of_a_trained_engine_within_the_accumulation_bound(space, capsys):
    eng = _small_engine(I=4000, steps=4)
    table = eng.item_pack(space, "cosine")
    q_loc = np.arange(0, 4000, 13, dtype=np.int32)
    q_img = table[q_loc.astype(np.int64)].contiguous()
    worst = _check_against_oracle(table, q_img, q_loc, 20)
    with capsys.disabled():
        print("\n[neighbors] engine tables (%s): largest |score - fp64 oracle| = %.3e" % (space, worst))
    assert worst <= 7.3e-5


# ---------------------------------------------------------------------------------------------- 4. slabs
@pytest.mark.parametrize("R", [2, 3, 8])
def test_ragged_slabs_merge_to_the_whole_table_bit_for_bit(R):
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    rng = np.random.default_rng(40 + R)
    I, n_q = 30011, 77
    W = rng.standard_normal((I, 600)).astype(np.float32)
    W[rng.integers(0, I, 200)] = W[5]                              # equal scores across slabs
    q_loc = rng.choice(I, n_q, replace=False).astype(np.int32)
    q_loc[0] = 5
    labels = rng.integers(0, 3, I).astype(np.uint8)
    cuts = np.sort(rng.choice(np.arange(100, I - 100), R - 1, replace=False))
    cuts[cuts % 16 == 0] += 3                                      # no cut at a multiple of 16
    cuts[0] = 37                                                   # one slab smaller than k
    edges = [0] + sorted(cuts.tolist()) + [I]
    assert all(c % 16 for c in edges[1:-1])
    whole = _pack_dev(W, "cosine")
    q_img = whole[q_loc.astype(np.int64)].contiguous()
    for k, lab, mask in ((20, None, 0x1FF), (256, None, 0x1FF), (100, labels, 0b101)):
        want_s, want_i = _nbr_dev(whole, q_img, q_loc, k, lab, mask, 0, I if lab is not None else 0)
        ps, pi = [], []
        for a, b in zip(edges[:-1], edges[1:]):
            part = _pack_dev(W[a:b], "cosine")                     # every part packed on its own
            assert torch.equal(part, whole[a:b])
            s, i = _nbr_dev(part, q_img, q_loc, k, lab, mask, a, I)
            assert np.all((i == -1) | ((i >= a) & (i < b)))
            ps.append(s)
            pi.append(i)
        ps = torch.from_numpy(np.stack(ps)).cuda()
        pi = torch.from_numpy(np.stack(pi)).cuda()
        so = torch.empty(n_q, k, dtype=torch.float32, device="cuda")
        io = torch.empty(n_q, k, dtype=torch.int32, device="cuda")
        rc = lib.ltg_topk_merge(R, n_q, k, ps.data_ptr(), pi.data_ptr(), k, so.data_ptr(), io.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(io.cpu().numpy(), want_i) and _eq(so.cpu().numpy(), want_s), (R, k, mask)


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_two_runs_of_the_largest_case_are_bit_identical():
    rng = np.random.default_rng(9)
    I, n_q, k = 70001, 300, 256
    tie = _pack_dev(_quarter_table(rng, I), "dot")
    real = _pack_dev(rng.standard_normal((I, 600)).astype(np.float32), "cosine")
    q_loc = rng.choice(I, n_q, replace=False).astype(np.int32)
    for table in (tie, real):
        q_img = table[q_loc.astype(np.int64)].contiguous()
        a = _nbr_dev(table, q_img, q_loc, k)
        b = _nbr_dev(table, q_img, q_loc, k)
        assert np.array_equal(a[1], b[1]) and _eq(a[0], b[0])
        assert np.all(a[1] >= 0)


# ---------------------------------------------------------------------------------------------- 6. host classes and CLI
def test_item_neighbors_class_equals_the_calls():
    import torch
    from ltgan.trainer import ItemNeighbors
    eng = _small_engine(I=1500, steps=2)
    I = eng.I
    labels = (np.arange(I) % 3).astype(np.uint8)
    for space, metric, k, lab, only in (("decoder", "cosine", 20, None, None), ("encoder", "dot", 7, labels, [2]), ("decoder", "cosine", 256, labels, [0, 1])):
        nb = ItemNeighbors(eng, k=k, space=space, metric=metric, labels=lab, n_groups=3 if lab is not None else None, only=only, chunk=400)
        ids, scores = nb.run()                                     # every item, four chunks (the last short)
        assert ids.shape == scores.shape == (I, k) and ids.dtype == np.int32 and scores.dtype == np.float32
        table = eng.item_pack(space, metric)
        mask = 0x1FF if only is None else sum(1 << g for g in only)
        want_s, want_i = _nbr_dev(table, table, np.arange(I, dtype=np.int32), k, lab, mask, 0, I if lab is not None else 0)
        assert np.array_equal(ids, want_i) and _eq(scores, want_s), (space, metric, k)
        assert not np.any(ids == np.arange(I)[:, None])            # an item is never its own neighbour
        if lab is not None:
            assert np.all(np.isin(lab[ids[ids >= 0]], only))
        q = np.array([5, 1499, 5, 0], np.int32)                    # a query list, a repeated id
        ids_q, scores_q = nb.run(q)
        assert np.array_equal(ids_q, ids[q]) and _eq(scores_q, scores[q])
    torch.cuda.synchronize()


def test_item_neighbors_class_large_catalogue_ragged_last_chunk():
    """100 000 items, 4 096 + 3 392 queries in chunks of 4 096: the short last chunk gets MORE item segments than a full one and needs a
    larger workspace than it (the need is not monotone in the number of queries)"""
    from ltgan.engine import Engine
    from ltgan.trainer import ItemNeighbors
    I, k = 100000, 20
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=5)
    assert eng.item_neighbors_ws_bytes(3392, k) > eng.item_neighbors_ws_bytes(4096, k)
    q = np.random.default_rng(1).choice(I, 4096 + 3392, replace=False).astype(np.int32)
    nb = ItemNeighbors(eng, k=k, chunk=4096)
    ids, scores = nb.run(q)
    table = eng.item_pack("decoder", "cosine")
    for sl in (slice(0, 4096), slice(4096, None)):
        want_s, want_i = _nbr_dev(table, table[q[sl].astype(np.int64)].contiguous(), q[sl], k)
        assert np.array_equal(ids[sl], want_i) and _eq(scores[sl], want_s)


def test_similar_cli_equals_the_class(tmp_path):
    import torch
    from ltgan import data_processing as dp
    from ltgan import longtail as lt
    from ltgan.trainer import ItemNeighbors
    ds, cwd, n_items, eng, ck, _, _, _ = askubuntu_run(tmp_path, split=None)
    _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(ds, "item2id.txt"), os.path.join(ds, "item_list.txt"),
                                               os.path.join(ds, "niche_items.txt"), n_items)
    labels, names = lt.build_groups(ds, "niche", 2, n_items)
    popular = np.nonzero(labels == 0)[0].astype(np.int32)
    ids_all, sc_all = ItemNeighbors(eng, k=20).run()
    ids_shelf, _ = ItemNeighbors(eng, k=10, labels=labels, n_groups=2, only=[1]).run(popular)
    torch.cuda.synchronize()

    def cli(*extra):
        last = [l for l in run_cli("similar.py", [ds, ck] + list(extra), cwd) if l.startswith("items: ")][-1]
        return dict(x.split(": ") for x in last.split("\t"))

    def table(path):
        out = []
        for line in open(os.path.join(cwd, path)).read().splitlines():
            q, items = line.split("\t")
            out.append((int(q), [int(x) for x in items.split(",")] if items else []))
        return out

    f = cli("--out", "sim.tsv", "--npz", "sim.npz")
    got = table("sim.tsv")
    assert [q for q, _ in got] == list(range(n_items))
    assert all(row == [i for i in ids_all[q].tolist() if i >= 0] for q, row in got)
    z = np.load(os.path.join(cwd, "sim.npz"))
    assert np.array_equal(z["ids"], ids_all) and _eq(z["scores"], sc_all) and z["items"].tolist() == list(range(n_items))
    assert int(f["items"]) == n_items and 0.0 <= float(f["niche_share@20"]) <= 1.0 and 0.0 < float(f["coverage@20"]) <= 1.0
    # the niche neighbours of the head items
    f = cli("--k", "10", "--items", "popular", "--groups", "niche", "--only", "niche", "--out", "shelf.tsv")
    got = table("shelf.tsv")
    assert [q for q, _ in got] == popular.tolist()
    assert all(row == [i for i in ids_shelf[n].tolist() if i >= 0] for n, (_, row) in enumerate(got))
    assert float(f["niche_share@10"]) == 1.0 and int(f["items"]) == popular.size
    # two ranks (gloo, one GPU), items sharded: the same table bit for bit
    run_cli("similar.py", [ds, ck, "--out", "sim2.tsv", "--npz", "sim2.npz"], cwd, world=2, limit=900)
    z2 = np.load(os.path.join(cwd, "sim2.npz"))
    assert np.array_equal(z2["ids"], ids_all) and _eq(z2["scores"], sc_all)
    assert open(os.path.join(cwd, "sim2.tsv")).read() == open(os.path.join(cwd, "sim.tsv")).read()


@pytest.mark.parametrize("world", [2])
def test_sharded_item_neighbors(world):
    run_ranks("dist_neighbors_worker.py", ["5003"], world, "NEIGHBORS_SHARDED_OK world=%d" % world)
