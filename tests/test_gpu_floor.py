"""Exposure-floor top-K lists on the GPU: ltg_floor_index / ltg_floor_rounds / ltg_floor_finish against the reference of
tests/floor_ref.py -- ids, score bits, the active table, the held counts and the whole state block (the definition is integer comparisons
of 64-bit words and one fp32 subtraction, so it is held bit for bit) -- on synthetic Zipf candidates at a row shorter than a wave,
segments far longer than a workgroup, 1 024-entry rows, k = 1, c off the wave size, quantised scores and a 3 000 x 1 000 split, with and
without lse and with a floor per item; the properties of the device output that need no reference (the floor, no blocking pair, order,
the composition, run-to-run bits, the batching of the rounds, rounds after convergence); Recommender(floor=) against the entry points
called by hand, with a LongTailReport and an Explain reading the final lists; the item-sharded recommender (tests/dist_floor_worker.py)
and both CLIs on Askubuntu_Sample in fresh child processes."""
import os
import re

import numpy as np
import pytest

import floor_ref as F
from serving_harness import DEV, _bits, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu

#         n,    I,    c,    k,  R,  M,  quant, pad_rows | what the reference gives with lse: rounds, lowerings, rows that differ, items short
SHAPES = [(64, 24, 24, 5, 2, 6, None, 3),                 # a row shorter than a wave                      4,  10, 0.53,  0
          (1500, 48, 24, 6, 2, 100, None, 0),             # segments far longer than a workgroup           8, 531, 0.79,  0
          (64, 1500, 1024, 100, 16, 1, None, 0),          # the longest row                                3,  28, 0.98,  0
          (200, 300, 100, 1, 1, 1, None, 0),              # k = 1                                          6, 229, 1.00, 84
          (130, 70, 65, 40, 8, 40, None, 3),              # c off the wave size                            2,   6, 0.41,  0
          (777, 129, 129, 10, 3, 30, 0.5, 0),             # quantised scores: ties broken by row          11, 472, 0.94,  0
          (3000, 1000, 256, 100, 10, 50, None, 0)]        # a larger split                                 4, 482, 0.92,  0
BATCH = 4


_CASES, _REFS = {}, {}


def case(t):
    """the inputs of shape t, built once and left unchanged -> (cand_s, cand_i, lse, need, k, R)"""
    if t not in _CASES:
        n, I, c, k, R, M, quant, pad = SHAPES[t]
        s, i, lse = F.zipf_case(n + I, n, I, c, quant=quant, pad_rows=pad)
        _CASES[t] = (s, i, lse, F.median_need(i, I, k, M), k, R)
    return _CASES[t]


def mixed_need(t):
    """a floor per item: a third of the items at 0, the rest in [1, 2 M]"""
    n, I, c, k, R, M, _, _ = SHAPES[t]
    rng = np.random.default_rng(91 + t)
    v = rng.integers(1, 2 * M + 1, I).astype(np.int32)
    v[rng.permutation(I)[:(I + 2) // 3]] = 0
    return v


def reference(t, kind):
    """floor_ref.floor_lists of shape t (kind: logprob, logit or mixed), computed once and left unchanged"""
    if (t, kind) not in _REFS:
        s, i, lse, need, k, R = case(t)
        _REFS[t, kind] = F.floor_lists(s, i, None if kind == "logit" else lse, mixed_need(t) if kind == "mixed" else need, k, R, batch=BATCH)
    return _REFS[t, kind]


def match_dev(s, i, lse, need, k, R, batch=BATCH, extra=0, poison=True, tables=True):
    """the matching through the C ABI on host arrays: index, rounds in batches of `batch` until a round lowers no limit, `extra` more
    rounds, finish -> host (scores, ids, active [n, c] bool, held [I], state [8])"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, c = i.shape
    I = len(need)
    st = torch.cuda.current_stream().cuda_stream
    s_d, i_d, need_d = _t(np.asarray(s, np.float32)), _t(np.asarray(i, np.int32)), _t(np.asarray(need, np.int32))
    lse_d = _t(np.asarray(lse, np.float32)) if lse is not None else None
    lp = lse_d.data_ptr() if lse is not None else None
    size = lib.ltg_floor_ws_bytes(n, c, I)
    assert size > 0
    ws = torch.full((size,), 0xA5 if poison else 0, dtype=torch.uint8, device=DEV)       # nothing relies on a zeroed workspace
    state = torch.full((cabi.LTG_FLOOR_STATE,), -9, dtype=torch.int32, device=DEV)
    so = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
    io = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    ao = torch.full((n, c), 9, dtype=torch.uint8, device=DEV)
    ho = torch.full((I,), -5, dtype=torch.int32, device=DEV)
    assert lib.ltg_floor_index(n, c, i_d.data_ptr(), I, state.data_ptr(), ws.data_ptr(), size, st) == 0
    assert state.cpu().tolist() == [0] * 8
    rounds = lambda r: lib.ltg_floor_rounds(n, c, s_d.data_ptr(), i_d.data_ptr(), lp, need_d.data_ptr(), I, k, R, r, state.data_ptr(),
                                            ws.data_ptr(), size, st)
    while True:
        assert rounds(batch) == 0
        h = state.cpu().tolist()
        if h[4] < h[1]:
            break
        assert h[1] <= n * c + 1
    if extra:
        assert rounds(extra) == 0
    assert lib.ltg_floor_finish(n, c, s_d.data_ptr(), i_d.data_ptr(), lp, need_d.data_ptr(), I, k, R, so.data_ptr(), io.data_ptr(),
                                ao.data_ptr() if tables else None, ho.data_ptr() if tables else None, state.data_ptr(), ws.data_ptr(), size,
                                st) == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), io.cpu().numpy(), ao.cpu().numpy() != 0, ho.cpu().numpy(), state.cpu().numpy()


def check_against_reference(s, i, lse, need, k, R, want, what, counts=True):
    wS, wI, wA, wH, wst = want
    differ = float((wI != i[:, :k]).any(1).mean())
    gS, gI, gA, gH, st = match_dev(s, i, lse, need, k, R)
    print("%s: rounds %d (device ran %d), lowerings %d, rows that differ from the plain top-k %.2f, items short of their floor %d, "
          "inserted slots %d, floor items %d" % (what, wst[4] + 1, st[1], wst[0], differ, wst[2], wst[5], wst[6]))
    if counts:                                           # the case counts, on the reference alone
        assert differ >= 0.25 and wst[0] >= 1, what
    bad = np.nonzero((gI != wI).any(1))[0]
    assert bad.size == 0, (what, bad[:5], gI[bad[:1]], wI[bad[:1]])
    assert np.array_equal(_bits(gS), _bits(wS)), what
    assert np.array_equal(gA, wA) and np.array_equal(gH, wH), what
    assert np.array_equal(st.astype(np.int64), wst), (what, st, wst)
    return gS, gI, gA, gH, st


# ---------------------------------------------------------------------------------------------- 1. parity with the reference
@pytest.mark.parametrize("t", range(len(SHAPES)))
@pytest.mark.parametrize("score", ["logprob", "logit"])
def test_parity_with_the_reference(t, score):
    s, i, lse, need, k, R = case(t)
    check_against_reference(s, i, lse if score == "logprob" else None, need, k, R, reference(t, score), (SHAPES[t], score))
    if SHAPES[t][3] == 1:
        assert reference(t, score)[4][2] >= 1            # k = 1 leaves an item short of its floor


@pytest.mark.parametrize("t", range(len(SHAPES)))
def test_parity_with_a_floor_per_item(t):
    s, i, lse, _, k, R = case(t)
    need = mixed_need(t)
    assert (need == 0).sum() >= len(need) // 3 and need.max() <= 2 * SHAPES[t][5]
    _, _, _, gH, _ = check_against_reference(s, i, lse, need, k, R, reference(t, "mixed"), (SHAPES[t], "per item"), counts=False)
    assert (gH[need == 0] == 0).all()


# ---------------------------------------------------------------------------------------------- 2. the device output on its own
@pytest.mark.parametrize("t", range(len(SHAPES)))
def test_properties_of_the_device_output(t):
    s, i, lse, need, k, R = case(t)
    n, I = len(s), len(need)
    gS, gI, gA, gH, st = match_dev(s, i, lse, need, k, R)
    fl, live = F.floor_mask(i, need)
    assert not (gA & ~fl).any()
    assert np.array_equal(gH, np.bincount(i[gA], minlength=I))
    assert (F.exposure(gI, I)[need > 0] >= np.minimum(need, gH)[need > 0]).all()         # the floor
    assert F.blocking_pairs(s, i, lse, need, k, R, gA) == 0
    cS, cI, ts = F.compose(s, i, gA, k, R)                # the lists are the composition of the matching
    assert np.array_equal(gI, cI) and np.array_equal(_bits(gS), _bits(cS))
    assert st[3] == (ts > 0).sum() and st[5] == ts.sum()
    for u in range(n):                                   # distinct ids in candidate order, each with its own logit, every active entry served
        got = gI[u][gI[u] >= 0]
        where = {int(g): p for p, g in enumerate(i[u]) if live[u, p]}
        pos = [where[int(g)] for g in got]
        assert pos == sorted(set(pos)) and set(np.nonzero(gA[u])[0]) <= set(pos), u
        assert pos[:k - R] == list(range(min(k - R, len(pos)))), u
        assert np.array_equal(_bits(gS[u, :len(pos)]), _bits(s[u, pos])), u
        assert (gI[u, len(pos):] == -1).all() and np.isneginf(gS[u, len(pos):]).all(), u
    # twice, with other batchings of the rounds, a zeroed workspace, rounds after convergence and without the tables: the same bits
    for kw in (dict(), dict(batch=1, poison=False), dict(batch=64), dict(batch=7, extra=5), dict(tables=False)):
        gS2, gI2, gA2, gH2, st2 = match_dev(s, i, lse, need, k, R, **kw)
        assert np.array_equal(gI2, gI) and np.array_equal(_bits(gS2), _bits(gS)), kw
        if kw.get("tables", True):
            assert np.array_equal(gA2, gA) and np.array_equal(gH2, gH), kw
        assert st2[0] == st[0] and (st2[2:] == st[2:]).all(), (kw, st, st2)
        assert st2[1] >= st2[4] + 1 + kw.get("extra", 0)
    # no floor, or no reserve: the first k columns of the candidates (padding behind a row's end), bit for bit, after one round
    pI = np.where(live[:, :k], i[:, :k], -1)
    pS = np.where(live[:, :k], s[:, :k], -np.inf).astype(np.float32)
    for nd, r in ((np.zeros(I, np.int32), R), (need, 0)):
        zS, zI, zA, zH, zst = match_dev(s, i, lse, nd, k, r, batch=1)
        assert np.array_equal(zI, pI) and np.array_equal(_bits(zS), _bits(pS))
        assert zst[:6].tolist() == [0, 1, zst[2], 0, 0, 0] and zst[6] == (nd > 0).sum() and not zA[:, k:].any()


def test_padded_rows_ids_outside_the_catalogue_and_zeros():
    """rows cut short by padding (one of them empty), ids at and beyond n_items (served as they are, never an index), entries after the
    padding (ignored), and an item every user scores +-0.0: equal scores keep the lower rows"""
    s, i, lse = F.zipf_case(3, 150, 90, 70, pad_rows=40)
    s, i = s.copy(), i.copy()
    i[5, :], s[5, :] = -1, -np.inf
    rng = np.random.default_rng(0)
    for u in rng.choice(150, 30, replace=False):
        j = int(rng.integers(0, 70))
        if i[u, j] >= 0:
            i[u, j] = 90 + int(rng.integers(0, 5)) * 1000          # 90, 1 090, ... : outside a catalogue of 90
    for u in range(40, 60):
        cut = int(np.argmax(i[u] < 0)) if (i[u] < 0).any() else 69
        i[u, cut] = -1
        i[u, cut + 1:] = rng.integers(0, 90, 69 - cut)             # entries behind the padding
    need = F.median_need(i, 90, 9, 20)
    for L in (lse, None):
        check_against_reference(s, i, L, need, 9, 4, F.floor_lists(s, i, L, need, 9, 4, batch=BATCH), "padded rows", counts=False)
    n = 130
    z = np.zeros((n, 2), np.float32)
    z[::2, 1] = -0.0
    z[:, 0] = 1.0
    zi = np.tile(np.array([[0, 1]], np.int32), (n, 1))
    gS, gI, gA, gH, _ = match_dev(z, zi, None, np.array([0, 70], np.int32), 1, 1)
    assert gI[:, 0].tolist() == [1] * 70 + [0] * (n - 70) and gH.tolist() == [0, 70]
    assert np.array_equal(_bits(gS[:70, 0]), _bits(z[:70, 1]))      # every zero keeps its sign


# ---------------------------------------------------------------------------------------------- 3. the host layer
def test_recommender_with_floor():
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Calibrate, Diversify, Explain, ExposureCap, ExposureFloor, LongTailReport, MinSlots, Recommender, ShareTarget
    I = 1001
    rng = np.random.default_rng(I)
    n, k, c, M, Rv = 300, 100, 400, 12, 10
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    # an output bias of log Zipf popularity, as steep as the users' own logits spread (tests/test_gpu_capped.py): the plain lists pile
    # onto a head and leave a tail that nobody is shown
    acts0 = eng.new_acts(n)
    eng.forward(ev.rows(0, n)[0], acts0, keep_prob=1.0, is_training=0.0, rng_step=77)
    sigma = float(acts0.logits[:n].std(dim=0).mean())
    bias = (-sigma * np.log(np.arange(1, I + 1)))[rng.permutation(I)].astype(np.float32)
    eng.g_p[7].copy_(_t(bias))
    labels = rng.integers(0, 3, I).astype(np.uint8)
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=1.0)
    need = F.median_need(plain_ids, I, k, M)
    print("sigma %.4g, floor items %d, of them below the floor in the plain lists %d" % (
        sigma, (need > 0).sum(), ((need > 0) & (F.exposure(plain_ids, I) < need)).sum()))
    assert ((need > 0) & (F.exposure(plain_ids, I) < need)).any()          # the floor binds
    tables = {}
    for score in ("logprob", "logit"):
        floor = ExposureFloor(need, Rv, score=score)
        rep, why = LongTailReport(labels, 2), Explain(2, top=4)
        rec = Recommender(eng, ev, k=k, chunk=128, floor=floor, report=rep, explain=why)
        ids, sc = rec.run(rng_step=77, keep_prob=1.0)
        assert floor.c == c
        # by hand: per chunk the forward and ltg_topk at c entries (the last chunk is short), then the entry points
        new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
        cs, ci, lse, w_s, w_i = new(n, c), new(n, c, dt=torch.int32), new(n), new(n, k), new(n, k, dt=torch.int32)
        acts = eng.new_acts(128)
        for lo in range(0, n, 128):
            hi = min(n, lo + 128)
            tr, _ = ev.rows(lo, hi)
            eng.forward(tr, acts, keep_prob=1.0, is_training=0.0, rng_step=77 + lo)
            eng.topk(acts, tr, c, cs[lo:hi], ci[lo:hi])
            lse[lo:hi].copy_(acts.lse[:hi - lo])
        need_d = _t(need)
        state, held = new(8, dt=torch.int32), new(I, dt=torch.int32)
        ws = new(eng.floor_ws_bytes(n, c), dt=torch.uint8)
        L = lse if score == "logprob" else None
        eng.floor_index(ci, I, state, ws)
        while True:
            eng.floor_rounds(cs, ci, L, need_d, k, Rv, 3, state, ws)
            h = state.cpu().tolist()
            if h[4] < h[1]:
                break
        eng.floor_finish(cs, ci, L, need_d, k, Rv, w_s, w_i, state, ws, held_out=held)
        torch.cuda.synchronize()
        assert np.array_equal(ids, w_i.cpu().numpy()) and np.array_equal(_bits(sc), _bits(w_s.cpu().numpy())), score
        assert np.array_equal(plain_ids, ci[:, :k].cpu().numpy()) and np.array_equal(floor.plain_ids(k), plain_ids)
        assert np.array_equal(floor.held(), held.cpu().numpy()) and np.array_equal(floor.need_vector(), need)
        # ... and the reference on the gathered candidates
        wS, wI, _, wH, wst = F.floor_lists(cs.cpu().numpy(), ci.cpu().numpy(), None if L is None else L.cpu().numpy(), need, k, Rv)
        assert np.array_equal(ids, wI) and np.array_equal(_bits(sc), _bits(wS)) and np.array_equal(floor.held(), wH), score
        st = floor.stats()
        assert (st["rounds"], st["lowerings"], st["short_items"], st["rows_changed"], st["inserted"], st["floor_items"]) == (
            wst[4] + 1, wst[0], wst[2], wst[3], wst[5], wst[6]), (st, wst)
        assert not np.array_equal(ids, plain_ids) and np.array_equal(ids[:, :k - Rv], plain_ids[:, :k - Rv])
        # the report read the final lists: its item_hits is their exposure, and every floor item has min(floor, held) of them
        hits = np.bincount(ids[ids >= 0], minlength=I)
        rep2 = LongTailReport(labels, 2)
        rep2.bind(eng, n, k)
        ids_d = _t(ids)
        for lo in range(0, n, 128):
            hi = min(n, lo + 128)
            rep2.add(eng, ids_d[lo:hi], ev.rows(lo, hi)[1], lo)
        (o1, h1), (o2, h2) = rep.table(), rep2.table()
        assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(h1, h2) and np.array_equal(h1, hits)
        assert (h1 >= np.minimum(need, floor.held())).all()
        # the explanations read the final lists too: the second pass ran, and equals an Explain over a recommender without a floor
        # wherever the lists agree
        why0 = Explain(2, top=4)
        Recommender(eng, ev, k=k, chunk=128, explain=why0).run(rng_step=77, keep_prob=1.0)
        (e_i, e_s), (p_i, p_s) = why.table(), why0.table()
        assert e_i.shape == p_i.shape and (e_i >= 0).any()
        assert np.array_equal(e_i, p_i) and np.array_equal(_bits(e_s), _bits(p_s))       # (the first 4 entries lie before k - reserve)
        print("%s: %s" % (score, st))
        tables[score] = ids
        ids2, sc2 = Recommender(eng, ev, k=k, chunk=128, floor=ExposureFloor(need, Rv, score=score, batch=1)).run(rng_step=77, keep_prob=1.0)
        assert np.array_equal(ids2, ids) and np.array_equal(_bits(sc2), _bits(sc))     # run to run; the batching of the rounds changes nothing
    assert not np.array_equal(tables["logprob"], tables["logit"])                    # the two scores rank the users differently
    # no floor, no reserve: the plain table, bit for bit; by group: only those items get a floor
    for fl in (ExposureFloor(0, Rv), ExposureFloor(need, 0)):
        ids0, sc0 = Recommender(eng, ev, k=k, chunk=128, floor=fl).run(rng_step=77, keep_prob=1.0)
        assert np.array_equal(ids0, plain_ids) and np.array_equal(_bits(sc0), _bits(plain_sc))
    fg = ExposureFloor((labels, 2, {0: 5}), Rv)
    idsg, _ = Recommender(eng, ev, k=k, chunk=128, floor=fg).run(rng_step=77, keep_prob=1.0)
    hg = np.bincount(idsg[idsg >= 0], minlength=I)
    assert np.array_equal(fg.need_vector(), np.where(labels == 0, 5, 0)) and (fg.held()[labels != 0] == 0).all()
    assert (hg[labels == 0] >= np.minimum(5, fg.held()[labels == 0])).all() and fg.stats()["inserted"] > 0
    good = ExposureFloor(M, Rv)
    for kw in (dict(diversify=Diversify(0.3)), dict(rule=MinSlots(labels, 3, [0, 5, 5])), dict(calibrate=Calibrate(labels, 2, 0.5)),
               dict(cap=ExposureCap(50)), dict(share=ShareTarget(labels, 2, [0], 0.3))):
        with pytest.raises(ValueError):
            Recommender(eng, ev, k=k, chunk=128, floor=good, **kw)
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=0, chunk=128, floor=good)
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=5, chunk=128, floor=good)                 # reserve 10 > k
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recommender_with_floor(world):
    run_ranks("dist_floor_worker.py", ["1001", "230"], world, "FLOOR_SHARDED_OK world=%d" % world)


def test_clis_on_askubuntu(tmp_path):
    import torch
    ds, cwd, n_items, _, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    n_users = tr.shape[0]
    M = max(2, n_users * 100 // n_items)                 # the mean exposure of an item: whatever the model, some items lie below it

    def floor_line(line):
        m = re.fullmatch(r"floor@100: (\d+) floor items, (\d+) short of their floor, below the floor (\d+) -> (\d+), (\d+) inserted slots, "
                         r"(\d+) rows changed, (\d+) rounds", line)
        assert m, line
        items, short, before, after, slots, rows, rounds = (int(x) for x in m.groups())
        assert short <= after <= before <= items and rows <= slots and rows <= n_users and rounds >= 1, line
        return items, short, before, after, slots, rows, rounds

    out = run_cli("recommend.py", [ds, ck, "--floor", str(M), "--floor-reserve", "10", "--out", "floor.tsv"], cwd)
    assert out[-2].startswith("users: %d\tniche_share@100: " % n_users)
    print(out[-1])
    items, short, before, after, slots, rows, _ = floor_line(out[-1])
    assert items == n_items and before >= 1 and slots >= 1              # the floor binds on this catalogue
    lines = open(os.path.join(cwd, "floor.tsv")).read().splitlines()
    assert len(lines) == n_users
    hits = np.zeros(n_items, np.int64)
    for n, line in enumerate(lines):
        u, _, listed = line.partition("\t")
        listed = [int(x) for x in listed.split(",")] if listed else []
        assert int(u) == uid0 + n and len(listed) == len(set(listed)) <= 100 and (not listed or (min(listed) >= 0 and max(listed) < n_items))
        np.add.at(hits, listed, 1)
    assert (hits < M).sum() == after
    out = run_cli("longtail.py", [ds, ck, "--floor", "niche:%d" % M, "--floor-reserve", "5", "--floor-score", "logit", "--floor-candidates", "300",
                                  "--groups", "niche"], cwd)
    print(out[-1])
    assert 1 <= floor_line(out[-1])[0] < n_items           # only the niche items get a floor
    assert out[-2].startswith("all\t") and len(out[-2].split("\t")) == 9
    torch.cuda.synchronize()
