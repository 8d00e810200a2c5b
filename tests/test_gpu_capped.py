"""Exposure-capped top-K lists on the GPU: ltg_cap_index / ltg_cap_rounds / ltg_cap_finish against the reference of tests/capped_ref.py,
ids and score bits (the definition is integer comparisons of 64-bit words and one fp32 subtraction, so it is held bit for bit), on
synthetic Zipf candidates at a row shorter than a wave, segments far longer than a workgroup, 1 024-entry rows, k = 1, c off the wave
size, quantised scores and a 3 000 x 1 000 split, with and without lse and with per-item caps; the properties of the device output that
need no reference (exposure, no blocking pair, order, run-to-run bits, rounds after convergence); Recommender(cap=) against the entry
points called by hand, with a LongTailReport reading the capped lists; the item-sharded recommender (tests/dist_capped_worker.py) and
both CLIs on Askubuntu_Sample in fresh child processes."""
import os

import numpy as np
import pytest

import capped_ref as R
from serving_harness import DEV, _bits, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu

#        n,    I,    c,    k,   cap, quant
SHAPES = [(64, 24, 24, 5, 14, None),                      # a row shorter than a wave
          (1500, 48, 24, 6, 200, None),                   # segments of ~1 400 entries, far longer than a workgroup
          (64, 1500, 1024, 100, 8, None),                 # the longest row
          (200, 300, 100, 1, 1, None),                    # k = 1: chains of displacements, the most rounds
          (130, 70, 65, 64, 125, None),                   # c not a multiple of 64, k ~ c
          (777, 129, 129, 10, 61, 0.5),                   # quantised scores: items break ties by user row
          (3000, 1000, 256, 100, 330, None)]


_CASES = {}


def case(t):
    """the inputs of shape t, built once and left unchanged"""
    if t not in _CASES:
        n, I, c, k, cap, quant = SHAPES[t]
        _CASES[t] = R.zipf_case(n + I, n, I, c, quant=quant) + (np.full(I, cap, np.int32), k)
    return _CASES[t]


def mixed_caps(t):
    """a cap per item: a fifth of the items at 0, a fifth uncapped, the rest spread around the shape's cap"""
    n, I, c, k, cap, _ = SHAPES[t]
    rng = np.random.default_rng(77 + t)
    v = rng.integers(max(1, cap // 2), cap + cap // 2 + 1, I).astype(np.int32)
    kind = rng.integers(0, 5, I)
    v[kind == 0] = 0
    v[kind == 1] = n
    return v


def match_dev(s, i, lse, cap, k, batch=4, extra=0, poison=True):
    """the matching through the C ABI on host arrays: index, rounds in batches of `batch` until a round raises no threshold, `extra`
    more rounds, finish -> host (scores, ids, state [8])"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, c = i.shape
    I = len(cap)
    st = torch.cuda.current_stream().cuda_stream
    s_d, i_d, cap_d = _t(np.asarray(s, np.float32)), _t(np.asarray(i, np.int32)), _t(np.asarray(cap, np.int32))
    lse_d = _t(np.asarray(lse, np.float32)) if lse is not None else None
    lp = lse_d.data_ptr() if lse is not None else None
    need = lib.ltg_cap_ws_bytes(n, c, I)
    assert need > 0
    ws = torch.full((need,), 0xA5 if poison else 0, dtype=torch.uint8, device=DEV)       # nothing relies on a zeroed workspace
    state = torch.full((cabi.LTG_CAP_STATE,), -9, dtype=torch.int32, device=DEV)
    so = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
    io = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    assert lib.ltg_cap_index(n, c, i_d.data_ptr(), I, state.data_ptr(), ws.data_ptr(), need, st) == 0
    assert state.cpu().tolist() == [0] * 8
    while True:
        assert lib.ltg_cap_rounds(n, c, s_d.data_ptr(), i_d.data_ptr(), lp, cap_d.data_ptr(), I, k, batch, state.data_ptr(), ws.data_ptr(),
                                  need, st) == 0
        h = state.cpu().tolist()
        if h[4] < h[1]:
            break
        assert h[1] <= n * c + 1
    if extra:
        assert lib.ltg_cap_rounds(n, c, s_d.data_ptr(), i_d.data_ptr(), lp, cap_d.data_ptr(), I, k, extra, state.data_ptr(), ws.data_ptr(),
                                  need, st) == 0
    assert lib.ltg_cap_finish(n, c, s_d.data_ptr(), i_d.data_ptr(), I, k, so.data_ptr(), io.data_ptr(), state.data_ptr(), ws.data_ptr(),
                              need, st) == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), io.cpu().numpy(), state.cpu().numpy()


def check_against_reference(s, i, lse, cap, k, what):
    wS, wI, wst = R.capped_lists(s, i, lse, cap, k)
    # the case counts: on the reference at least a quarter of the rows differ from the plain top-k and an item sits exactly at its cap
    differ = float((wI != i[:, :k]).any(1).mean())
    hits = R.exposure(wI, len(cap))
    at_cap = int(((hits == cap) & (cap > 0)).sum())
    gS, gI, st = match_dev(s, i, lse, cap, k)
    print("%s: rows that differ from the plain top-k %.2f, items at their cap %d, rounds %d (device ran %d), passed over %d, short %d"
          % (what, differ, at_cap, wst["rounds"], st[1], wst["over"], wst["short"]))
    assert differ >= 0.25 and at_cap >= 1, what
    bad = np.nonzero((gI != wI).any(1))[0]
    assert bad.size == 0, (what, bad[:5], gI[bad[:1]], wI[bad[:1]])
    assert np.array_equal(_bits(gS), _bits(wS)), what
    assert st[4] + 1 == wst["rounds"] and st[2] == wst["over"] and st[3] == wst["short"] and (st[5:] == 0).all(), (what, st, wst)
    return gS, gI, st


# ---------------------------------------------------------------------------------------------- 1. parity with the reference
@pytest.mark.parametrize("t", range(len(SHAPES)))
@pytest.mark.parametrize("score", ["logprob", "logit"])
def test_parity_with_the_reference(t, score):
    s, i, lse, cap, k = case(t)
    check_against_reference(s, i, lse if score == "logprob" else None, cap, k, (SHAPES[t], score))


@pytest.mark.parametrize("t", range(len(SHAPES)))
def test_parity_with_a_cap_per_item(t):
    s, i, lse, _, k = case(t)
    cap = mixed_caps(t)
    assert (cap == 0).any() and (cap >= len(s)).any()
    _, gI, _ = check_against_reference(s, i, lse, cap, k, (SHAPES[t], "per item"))
    hits = R.exposure(gI, len(cap))
    assert (hits[cap == 0] == 0).all()


# ---------------------------------------------------------------------------------------------- 2. the device output on its own
@pytest.mark.parametrize("t", range(len(SHAPES)))
def test_properties_of_the_device_output(t):
    s, i, lse, cap, k = case(t)
    n, I = len(s), len(cap)
    gS, gI, st = match_dev(s, i, lse, cap, k)
    assert (R.exposure(gI, I) <= cap).all()
    assert R.blocking_pairs(s, i, lse, cap, k, gI) == 0
    for u in range(n):                                   # distinct ids in candidate order, each with its own logit
        got = gI[u][gI[u] >= 0]
        where = {int(g): p for p, g in enumerate(i[u]) if g >= 0}
        pos = [where[int(g)] for g in got]
        assert pos == sorted(set(pos)), u
        assert np.array_equal(_bits(gS[u, :len(pos)]), _bits(s[u, pos])), u
        assert (gI[u, len(pos):] == -1).all() and np.isneginf(gS[u, len(pos):]).all(), u
    # twice, with another batching of the rounds, a zeroed workspace and rounds after convergence: the same bits
    for kw in (dict(), dict(batch=1, poison=False), dict(batch=7, extra=5)):
        gS2, gI2, st2 = match_dev(s, i, lse, cap, k, **kw)
        assert np.array_equal(gI2, gI) and np.array_equal(_bits(gS2), _bits(gS)), kw
        assert st2[0] == st[0] and st2[4] == st[4] and (st2[2:4] == st[2:4]).all(), (kw, st, st2)
        assert st2[1] >= st2[4] + 1 + kw.get("extra", 0)
    # caps that cannot bind: the first k columns of the candidates, bit for bit, after one round
    for big in (n, 2 ** 31 - 1):
        pS, pI, pst = match_dev(s, i, lse, np.full(I, big, np.int32), k, batch=1)
        assert np.array_equal(pI, i[:, :k]) and np.array_equal(_bits(pS), _bits(s[:, :k]))
        assert pst[:5].tolist() == [0, 1, 0, int((i[:, k - 1] < 0).sum()), 0]


def test_padded_rows_ids_outside_the_catalogue_and_zeros():
    """rows cut short by padding (one of them empty), ids at and beyond n_items (skipped, never an index), entries after the padding
    (ignored), and an item every user scores +-0.0: equal scores keep the lower rows"""
    s, i, lse = R.zipf_case(3, 150, 90, 70, pad_rows=40)
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
    cap = np.full(90, 12, np.int32)
    for L in (lse, None):
        check_against_reference(s, i, L, cap, 9, "padded rows")
    n = 130
    z = np.zeros((n, 2), np.float32)
    z[::2, 0] = -0.0
    z[:, 1] = -1.0
    zi = np.tile(np.array([[0, 1]], np.int32), (n, 1))
    gS, gI, _ = match_dev(z, zi, None, np.array([70, n], np.int32), 1)
    assert gI[:, 0].tolist() == [0] * 70 + [1] * (n - 70)
    assert np.array_equal(_bits(gS[:70, 0]), _bits(z[:70, 0]))      # every zero keeps its sign


# ---------------------------------------------------------------------------------------------- 3. the host layer
@pytest.mark.parametrize("I", [1001, 1537])
def test_recommender_with_cap(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Calibrate, Diversify, ExposureCap, LongTailReport, MinSlots, Recommender
    rng = np.random.default_rng(I)
    n, k, c, C = 300, 100, 400, 60
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    # an output bias of log Zipf popularity, as steep as the users' own logits spread (the shape of capped_ref.zipf_case): the plain
    # lists pile onto a head, as a trained model's do, and the users still differ
    acts0 = eng.new_acts(n)
    eng.forward(ev.rows(0, n)[0], acts0, keep_prob=1.0, is_training=0.0, rng_step=77)
    sigma = float(acts0.logits[:n].std(dim=0).mean())
    bias = (-sigma * np.log(np.arange(1, I + 1)))[rng.permutation(I)].astype(np.float32)
    eng.g_p[7].copy_(_t(bias))
    labels = rng.integers(0, 3, I).astype(np.uint8)
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=1.0)
    print("I %d: sigma %.4g, max plain exposure %d of %d users" % (I, sigma, R.exposure(plain_ids, I).max(), n))
    assert R.exposure(plain_ids, I).max() > 2 * C        # the cap binds: the head is in most plain lists
    tables = {}
    for score in ("logprob", "logit"):
        cap = ExposureCap(C, score=score)
        rep = LongTailReport(labels, 2)
        rec = Recommender(eng, ev, k=k, chunk=128, cap=cap, report=rep)
        ids, sc = rec.run(rng_step=77, keep_prob=1.0)
        assert cap.c == c
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
        cap_d = torch.full((I,), C, dtype=torch.int32, device=eng.device)
        state = new(8, dt=torch.int32)
        ws = new(eng.cap_ws_bytes(n, c), dt=torch.uint8)
        L = lse if score == "logprob" else None
        eng.cap_index(ci, I, state, ws)
        while True:
            eng.cap_rounds(cs, ci, L, cap_d, k, 3, state, ws)
            h = state.cpu().tolist()
            if h[4] < h[1]:
                break
        eng.cap_finish(cs, ci, I, k, w_s, w_i, state, ws)
        torch.cuda.synchronize()
        assert np.array_equal(ids, w_i.cpu().numpy()) and np.array_equal(_bits(sc), _bits(w_s.cpu().numpy())), score
        assert np.array_equal(plain_ids, ci[:, :k].cpu().numpy()) and np.array_equal(cap.plain_ids(k), plain_ids)
        # ... and the reference on the gathered candidates
        wS, wI, wst = R.capped_lists(cs.cpu().numpy(), ci.cpu().numpy(), None if L is None else L.cpu().numpy(), np.full(I, C, np.int32), k)
        assert np.array_equal(ids, wI) and np.array_equal(_bits(sc), _bits(wS)), score
        st = cap.stats()
        assert (st["rounds"], st["passed_over"], st["short"]) == (wst["rounds"], wst["over"], wst["short"]), (st, wst)
        hits = np.bincount(ids[ids >= 0], minlength=I)
        assert hits.max() == C and not np.array_equal(ids, plain_ids)
        # the report read the capped lists: ltg_topk_metrics over them, chunk by chunk, and its item_hits is their exposure
        rep2 = LongTailReport(labels, 2)
        rep2.bind(eng, n, k)
        ids_d = _t(ids)
        for lo in range(0, n, 128):
            hi = min(n, lo + 128)
            rep2.add(eng, ids_d[lo:hi], ev.rows(lo, hi)[1], lo)
        (o1, h1), (o2, h2) = rep.table(), rep2.table()
        assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(h1, h2) and np.array_equal(h1, hits) and (h1 <= C).all()
        print("I %d %s: max exposure %d -> %d, %s" % (I, score, R.exposure(plain_ids, I).max(), hits.max(), st))
        tables[score] = ids
        ids2, sc2 = Recommender(eng, ev, k=k, chunk=128, cap=ExposureCap(C, score=score, batch=1)).run(rng_step=77, keep_prob=1.0)
        assert np.array_equal(ids2, ids) and np.array_equal(_bits(sc2), _bits(sc))     # run to run; the batching of the rounds changes nothing
    assert not np.array_equal(tables["logprob"], tables["logit"])                    # the two scores rank the users differently
    # a cap nobody reaches: the plain table, bit for bit; by group: only those items are capped
    ids0, sc0 = Recommender(eng, ev, k=k, chunk=128, cap=ExposureCap(n)).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids0, plain_ids) and np.array_equal(_bits(sc0), _bits(plain_sc))
    idsg, _ = Recommender(eng, ev, k=k, chunk=128, cap=ExposureCap((labels, 2, {0: 25}))).run(rng_step=77, keep_prob=1.0)
    hg = np.bincount(idsg[idsg >= 0], minlength=I)
    assert hg[labels == 0].max() == 25 and hg[labels != 0].max() > 25
    good = ExposureCap(C)
    for kw in (dict(diversify=Diversify(0.3)), dict(rule=MinSlots(labels, 3, [0, 5, 5])), dict(calibrate=Calibrate(labels, 2, 0.5))):
        with pytest.raises(ValueError):
            Recommender(eng, ev, k=k, chunk=128, cap=good, **kw)
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=0, chunk=128, cap=good)
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recommender_with_cap(world):
    run_ranks("dist_capped_worker.py", ["1001", "230"], world, "CAPPED_SHARDED_OK world=%d" % world)


def test_clis_on_askubuntu(tmp_path):
    import torch
    ds, cwd, n_items, _, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    n_users = tr.shape[0]
    C = max(2, n_users // 10)                            # far below the head's plain exposure, and enough places for full lists

    def cap_line(line, bound):
        import re
        m = re.fullmatch(r"cap@100: max exposure (\d+) -> (\d+), (\d+) items at their cap, (\d+) short lists, (\d+) rounds", line)
        assert m, line
        before, after, at_cap, short, rounds = (int(x) for x in m.groups())
        assert (bound is None or after <= bound) and rounds >= 1, line
        return before, after, at_cap, short, rounds

    out = run_cli("recommend.py", [ds, ck, "--cap", str(C), "--out", "cap.tsv"], cwd)
    assert out[-2].startswith("users: %d\tniche_share@100: " % n_users)
    print(out[-1])
    before, after, at_cap, short, _ = cap_line(out[-1], C)
    assert before > C and after == C and at_cap >= 1     # the cap binds on this catalogue
    lines = open(os.path.join(cwd, "cap.tsv")).read().splitlines()
    assert len(lines) == n_users
    hits = np.zeros(n_items, np.int64)
    n_short = 0
    for n, line in enumerate(lines):
        u, _, items = line.partition("\t")
        items = [int(x) for x in items.split(",")] if items else []
        assert int(u) == uid0 + n and len(items) == len(set(items)) <= 100 and (not items or (min(items) >= 0 and max(items) < n_items))
        n_short += len(items) < 100
        np.add.at(hits, items, 1)
    assert hits.max() == after and n_short == short
    out = run_cli("longtail.py", [ds, ck, "--cap", "popular:%d" % C, "--cap-score", "logit", "--cap-candidates", "300", "--groups", "niche"], cwd)
    print(out[-1])
    # only the popular items are capped, and the users they turn away land on niche items: the largest exposure has no bound
    assert cap_line(out[-1], None)[2] >= 1
    assert out[-2].startswith("all\t") and len(out[-2].split("\t")) == 9
    torch.cuda.synchronize()
