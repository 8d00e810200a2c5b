"""Critic-checked lists on the GPU (ltg_pair_critic / ltg_critic_finish / ltg_topk_gate): the kernel's sums and best anchors
rebuilt in numpy from ltg_pair_companions' own pair scores, bit for bit; the critic against the fp64 oracle of the device's images within
the companions' derived bound; every shape at which the kernel takes another path against tests/critic_ref.py fed the device's pair
scores, bit for bit; position independence; the gate against gate_ref; the refusals; and the host layer: Critic / CriticGate on a
Recommender, recommend.py / longtail.py, and the item-sharded run (tests/dist_critic_worker.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import companions_ref as CR
import critic_ref as KR
import test_critic_cpu as TK
import test_gpu_companions as TG
from serving_harness import askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu
TINY, CONFIG = (8, 5, 7, 13), (100, 150, 250, 300)       # h3 = 13 is no multiple of 4 (ld = 16); config.ini's sizes
CASES = [(TINY, False), (CONFIG, False), (TINY, True), (CONFIG, True)]
CASE_IDS = ["h3-13", "config", "h3-13-trained-range", "config-trained-range"]
I = 2000
K_IN = 300
ANCHOR_COUNTS = (0, 1, 8, 9, 32, 33, 64, 65, 129)         # 8 | 9: an anchor per wave or two; 32 | 33: one staging of anchor rows or two


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, keys=("sum", "cnt", "best_s", "best_i", "crit", "n_scored")):
    for key in keys:
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key


@functools.lru_cache(maxsize=None)
def _problem(hs, hot):
    """one discriminator (tests/test_gpu_companions._discriminator), a catalogue of 2 000 items cut into popular / niche with 60 items
    without features, both side images and the DEVICE's own score of every (popular, niche) pair -- computed once, never written"""
    rng = np.random.default_rng(5)
    dv = TG.Disc(TG._discriminator(hs, hot))
    niche = set(rng.choice(I - 2, 1000, replace=False).tolist()) | {I - 1}           # I - 1: niche, I - 2: popular, both with features
    valid = set(range(I)) - set(rng.choice(I - 2, 60, replace=False).tolist())
    pop_ids, niche_ids, pop_row, niche_row = KR.side_maps(niche, valid, I)
    P = dict(dv=dv, pop_ids=pop_ids, niche_ids=niche_ids, pop_row=pop_row, niche_row=niche_row, niche=niche, valid=valid)
    P["pop_img"], P["niche_img"] = dv.pack("popular", pop_ids), dv.pack("niche", niche_ids)
    P["pop_row_d"], P["niche_row_d"] = _t(pop_row), _t(niche_row)
    S = dv.score_table(P["pop_img"], P["niche_img"])
    S.setflags(write=False)
    P["S"] = S
    return P


def _critic_dev(P, indptr, indices, ids, top, hist_lo=0, cnt_all=None):
    """ltg_pair_critic and ltg_critic_finish on host arrays -> dict of host arrays (every output starts from a sentinel)"""
    import torch
    dv = P["dv"]
    lib, cabi = dv.lib, dv.cabi
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    n, k_in = ids.shape
    ip, ix, idd = _t(np.asarray(indptr, np.int32)), _t(np.concatenate([np.asarray(indices, np.int32), np.zeros(1, np.int32)])), _t(ids)
    tr = cabi.ltg_batch()
    tr.n_rows, tr.indptr, tr.indices = n, ip.data_ptr(), ix.data_ptr()
    acc = torch.full((n, top), -77, dtype=torch.int64, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    b_s = torch.full((n, top), 7.0, dtype=torch.float32, device="cuda")
    b_i = torch.full((n, top), -7, dtype=torch.int32, device="cuda")
    crit = torch.full((n, top), 7.0, dtype=torch.float32, device="cuda")
    n_sc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.ltg_pair_critic(C.byref(dv.cfg), C.byref(dv.disc), P["pop_img"].data_ptr(), len(P["pop_ids"]), P["niche_img"].data_ptr(),
                             len(P["niche_ids"]), P["pop_row_d"].data_ptr(), P["niche_row_d"].data_ptr(), I, C.byref(tr), hist_lo, n, k_in,
                             idd.data_ptr(), top, acc.data_ptr(), cnt.data_ptr(), b_s.data_ptr(), b_i.data_ptr(), st)
    assert rc == 0
    cnt_f = cnt if cnt_all is None else _t(np.asarray(cnt_all, np.int32))
    rc = lib.ltg_critic_finish(n, k_in, idd.data_ptr(), top, P["niche_row_d"].data_ptr(), I, len(P["niche_ids"]), acc.data_ptr(), cnt_f.data_ptr(),
                               crit.data_ptr(), n_sc.data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()
    return dict(sum=h(acc), cnt=h(cnt), best_s=h(b_s), best_i=h(b_i), crit=h(crit), n_scored=h(n_sc))


# ---------------------------------------------------------------------------------------------- 1. the pair bits
@pytest.mark.parametrize("hs,hot", CASES, ids=CASE_IDS)
def test_pair_bits_are_the_companions_kernels(hs, hot):
    """one user, 5 anchors, 9 entries: ltg_pair_companions with the anchors as queries, the entries as candidates and k = all of them gives
    the device's 45 pair scores; the sums and best anchors rebuilt from them in numpy are the kernel's, bit for bit"""
    P = _problem(hs, hot)
    dv = P["dv"]
    rng = np.random.default_rng(hs[3] + hot)
    a = np.sort(rng.choice(P["pop_ids"], 5, replace=False))
    b = np.sort(rng.choice(P["niche_ids"], 9, replace=False))
    s, i = dv.companions(P["pop_img"][_t(P["pop_row"][a].astype(np.int64))].contiguous(), np.full(5, -1, np.int32),
                         P["niche_img"][_t(P["niche_row"][b].astype(np.int64))].contiguous(), b, 9)
    T = np.empty((5, 9), np.float32)
    for r in range(5):
        assert np.array_equal(np.sort(i[r]), b)
        T[r, np.searchsorted(b, i[r])] = s[r]
    assert np.array_equal(_bits(T), _bits(P["S"][P["pop_row"][a]][:, P["niche_row"][b]]))
    entries = rng.permutation(b)
    got = _critic_dev(P, [0, 5], a, entries[None, :], 9)
    assert got["cnt"].tolist() == [5] and got["n_scored"].tolist() == [9]
    for e, g in enumerate(entries):
        col = T[:, np.searchsorted(b, g)]
        assert got["sum"][0, e] == KR.fixed(col).sum()
        bs, bi = KR.best_of(col, a)
        assert got["best_i"][0, e] == bi and _bits(got["best_s"][0, e:e + 1])[0] == _bits(np.array([bs], np.float32))[0]
        assert _bits(got["crit"][0, e:e + 1])[0] == _bits(np.array([KR.mean_fixed(KR.fixed(col).sum(), 5)]))[0]


# ---------------------------------------------------------------------------------------------- 2. against the fp64 oracle
@pytest.mark.parametrize("hs,hot", CASES, ids=CASE_IDS)
def test_against_the_fp64_oracle_of_the_device_images(hs, hot, capsys):
    """tol = (8 + h3) 2^-24 (sum |w4| + |b4|), the companions' derived bound per pair logit.  |crit - ref| <= tol + 2^-25 + 2^-24 |ref|: the
    mean of logits each within tol, the fixed-point half unit, the final rounding.  anchor_s within tol of the oracle at the returned
    anchor, whose oracle score is at least the best oracle score - 2 tol.  No case is excluded.  Measured on an MI355X."""
    P = _problem(hs, hot)
    dv = P["dv"]
    rng = np.random.default_rng(9)
    pool = P["pop_ids"][:120]
    S64 = CR.score_ref(P["pop_img"][:120].cpu().numpy(), P["niche_img"].cpu().numpy(), dv.D["w4"], dv.D["b4"])
    counts = [1, 2, 5, 9, 17, 33, 64, 65, 120] * 3
    hist = [np.sort(rng.choice(pool, c, replace=False)) for c in counts]
    indptr = np.cumsum([0] + counts)
    ids = np.stack([rng.choice(I, 64, replace=False) for _ in counts])
    got = _critic_dev(P, indptr, np.concatenate(hist), ids, 64)
    worst = [0.0, 0.0, 0.0]
    n_scored = 0
    for u, a in enumerate(hist):
        for e in range(64):
            nr = P["niche_row"][ids[u, e]]
            if nr < 0:
                assert got["best_i"][u, e] == -1 and got["crit"][u, e] == 0.0
                continue
            n_scored += 1
            col = S64[P["pop_row"][a], nr]
            ref = col.mean()
            e0 = abs(float(got["crit"][u, e]) - ref)
            assert e0 <= dv.tol + 2.0 ** -25 + 2.0 ** -24 * abs(ref), (u, e, e0)
            at = int(np.searchsorted(a, got["best_i"][u, e]))
            assert a[at] == got["best_i"][u, e]
            e1 = abs(float(got["best_s"][u, e]) - col[at])
            assert e1 <= dv.tol, (u, e, e1)
            assert col[at] >= col.max() - 2 * dv.tol, (u, e)
            worst = [max(worst[0], e0), max(worst[1], e1), max(worst[2], float(col.max() - col[at]))]
    assert n_scored > 500
    with capsys.disabled():
        print("\n[critic] %s hot=%d: %d scored entries, |crit| <= %.2f, tol %.3e: largest |crit - fp64 oracle| %.3e, |anchor_s - oracle| %.3e, "
              "best oracle - returned anchor's %.3e" % (hs, hot, n_scored, np.abs(got["crit"]).max(), dv.tol, worst[0], worst[1], worst[2]))


# ---------------------------------------------------------------------------------------------- 3. the shapes where it can go wrong
@functools.lru_cache(maxsize=None)
def _shapes(hs, hot):
    """70 users: a history of 1 100 items with 600 anchors (more than the 512 the kernel stages at once), an empty one, one of niche items
    only, then anchor counts 0, 1, 8, 9, 32, 33, 64, 65, 129 in turn among niche items and popular items without features; lists of 300 entries
    with -1 padding inside, popular entries, niche entries without features and the id I - 1; the reference at top = 256, once"""
    P = _problem(hs, hot)
    rng = np.random.default_rng(21)
    others = np.setdiff1d(np.arange(I), P["pop_ids"])                  # niche items and the popular items without features: no anchors
    hist = [np.concatenate([rng.choice(P["pop_ids"], 600, replace=False), rng.choice(others, 500, replace=False)]), np.zeros(0, np.int64),
            rng.choice(P["niche_ids"], 12, replace=False)]
    for u in range(3, 70):
        c = ANCHOR_COUNTS[u % len(ANCHOR_COUNTS)]
        hist.append(np.concatenate([rng.choice(P["pop_ids"], c, replace=False), rng.choice(others, 1 + u % 5, replace=False)]))
    hist[5] = np.union1d(hist[5], [I - 2, I - 1])
    hist = [np.sort(h).astype(np.int32) for h in hist]
    indptr = np.cumsum([0] + [h.size for h in hist]).astype(np.int32)
    ids = np.stack([rng.choice(I, K_IN, replace=False) for _ in range(70)]).astype(np.int32)
    ids[rng.random(ids.shape) < 0.1] = -1
    ids[np.arange(70), np.arange(70) % 64] = I - 1
    ids[7, :70] = -1                                                    # a row whose first 70 entries are padding
    ids[8, :256] = rng.choice(P["niche_ids"], 256, replace=False)       # every entry a candidate: four full steps
    ids[9, :256] = rng.choice(P["pop_ids"], 256, replace=False)         # none is
    want = KR.critic_ref(P["S"], indptr, np.concatenate(hist), P["pop_row"], P["niche_row"], ids, 256)
    assert want["cnt"][:3].tolist() == [600, 0, 0] and set(ANCHOR_COUNTS) <= set(want["cnt"][3:].tolist())
    assert want["scored"][8].all() and not want["scored"][9].any() and want["scored"].sum() > 3000
    assert np.any(~want["scored"] & (ids[:, :256] >= 0) & (P["niche_row"][np.clip(ids[:, :256], 0, I - 1)] < 0) & np.isin(ids[:, :256], list(P["niche"])))
    return P, hist, indptr, ids, want


def _prefix(want, ids, niche_row, n, top):
    """the reference of the first n rows at a shorter `top`: the entries are independent of each other"""
    out = {key: want[key][:n, :top] for key in ("sum", "best_s", "best_i", "crit")}
    out["cnt"] = want["cnt"][:n]
    out["n_scored"] = want["scored"][:n, :top].sum(1).astype(np.int32)
    return out


@pytest.mark.parametrize("top", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("n_rows", [1, 3, 70])
def test_shapes_against_the_reference_bit_for_bit(n_rows, top):
    P, hist, indptr, ids, want = _shapes(CONFIG, False)
    got = _critic_dev(P, indptr[:n_rows + 1], np.concatenate(hist[:n_rows]), ids[:n_rows], top)
    _same(got, _prefix(want, ids, P["niche_row"], n_rows, top))


@pytest.mark.parametrize("hs,hot", CASES[2:] + CASES[:1], ids=CASE_IDS[2:] + CASE_IDS[:1])
def test_shapes_on_the_other_discriminators(hs, hot):
    P, hist, indptr, ids, want = _shapes(hs, hot)
    for top in (65, 256):
        _same(_critic_dev(P, indptr, np.concatenate(hist), ids, top), _prefix(want, ids, P["niche_row"], 70, top))


def test_position_independence_and_slabs():
    """a user's outputs do not change with the row it sits in or with n_rows; two runs are identical; and the histories cut into three
    item slabs (local ids, hist_lo) give sums and counts that add up to the whole run's, best anchors whose best is the whole run's"""
    P, hist, indptr, ids, want = _shapes(CONFIG, False)
    whole = _critic_dev(P, indptr, np.concatenate(hist), ids, 100)
    _same(_critic_dev(P, indptr, np.concatenate(hist), ids, 100), whole)
    for rows in ([0], [69], [8, 0, 33], [33, 5, 1, 0, 8, 64, 65]):
        ip = np.cumsum([0] + [hist[u].size for u in rows])
        got = _critic_dev(P, ip, np.concatenate([hist[u] for u in rows]), ids[rows], 100)
        _same(got, {key: whole[key][rows] for key in whole})
    parts = []
    for lo, hi in ((0, 700), (700, 1301), (1301, I)):
        hs_ = [h[(h >= lo) & (h < hi)] - lo for h in hist]
        parts.append(_critic_dev(P, np.cumsum([0] + [h.size for h in hs_]), np.concatenate(hs_), ids, 100, hist_lo=lo))
    assert np.array_equal(sum(p["sum"] for p in parts), whole["sum"]) and np.array_equal(sum(p["cnt"] for p in parts), whole["cnt"])
    words = lambda p: np.where(p["best_i"] >= 0, p["best_s"].astype(np.float64), -np.inf)
    stack_s, stack_i = np.stack([words(p) for p in parts]), np.stack([p["best_i"] for p in parts])
    for u, e in zip(*np.nonzero(whole["best_i"] >= 0)):
        ok = stack_i[:, u, e] >= 0
        s, g = KR.best_of(stack_s[ok, u, e], stack_i[ok, u, e])
        assert g == whole["best_i"][u, e] and np.float32(s) == whole["best_s"][u, e]
    assert not np.any((stack_i >= 0).any(0) & (whole["best_i"] < 0))
    # the finish with the counts of all slabs on one slab's lists flags the same entries
    fin = _critic_dev(P, indptr, np.concatenate(hist), ids, 100, cnt_all=whole["cnt"])
    assert np.array_equal(_bits(fin["crit"]), _bits(whole["crit"]))


# ---------------------------------------------------------------------------------------------- 4. the gate
@functools.lru_cache(maxsize=None)
def _served(hs):
    """an Engine of 2 000 items, 90 users (one holds all but 10 items: its candidates are padded), random logits in the activations' place"""
    import torch
    import helpers as Hh
    import scipy.sparse as sp
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    rng = np.random.default_rng(hs[3])
    eng = Engine(I, h_sizes=hs, lr=1e-3, precision="bf16", seed=3, d_seed=9)
    X = Hh.random_history(rng, 90, I, mean_nnz=25).tolil()
    X[4, :] = 0
    X[4, rng.choice(I, I - 10, replace=False)] = 1
    X[5, :] = 0                                                        # no history: no anchors, nothing is scored
    X = sp.csr_matrix(X, dtype=np.float32)
    X.eliminate_zeros()
    X.sort_indices()
    ev = EvalData(X, X, eng.device)
    niche = set(rng.choice(I, 1100, replace=False).tolist())
    valid = set(range(I)) - set(rng.choice(I, 50, replace=False).tolist())
    logits = torch.from_numpy(rng.normal(0, 1, (90, I)).astype(np.float32)).to(eng.device)
    return eng, ev, X, niche, valid, logits


def _eng_critic(eng, sides, tr, ids, top):
    import torch
    from ltgan.serving import SlabLists
    n = int(ids.shape[0])
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    acc, cnt, b_s, b_i = new(n, top, dt=torch.int64), new(n, dt=torch.int32), new(n, top), new(n, top, dt=torch.int32)
    crit, n_sc = new(n, top), new(n, dt=torch.int32)
    sides.evaluate(SlabLists(eng, n, top), tr, ids, top, acc, cnt, b_s, b_i, crit, n_sc)
    return dict(crit=crit, anchor_s=b_s, anchor_i=b_i, n_anchor=cnt, n_scored=n_sc)


@pytest.mark.parametrize("c_in", [20, 65, 256])
@pytest.mark.parametrize("hs", [TINY, CONFIG], ids=["h3-13", "config"])
def test_gate_against_the_reference(hs, c_in):
    import torch
    from ltgan.serving import _CriticSides
    eng, ev, X, niche, valid, logits = _served(hs)
    n, k = 90, 20
    tr, _ = ev.rows(0, n)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    c_s, c_i, p_s, p_i = new(n, c_in), new(n, c_in, dt=torch.int32), new(n, k), new(n, k, dt=torch.int32)
    eng.topk(logits, tr, c_in, c_s, c_i)
    eng.topk(logits, tr, k, p_s, p_i)
    sides = _CriticSides(niche, valid)
    sides.bind(eng)
    sides.pack(eng)
    cr = _eng_critic(eng, sides, tr, c_i, c_in)
    h = lambda t: t.cpu().numpy()
    crit, flag = h(cr["crit"]), h(cr["anchor_i"])
    assert (flag >= 0).sum() > 5 * c_in and not (flag[5] >= 0).any() and (h(c_i)[4] >= 0).sum() == 10
    scored = crit[flag >= 0]
    u0 = 0
    e0 = int(np.nonzero(flag[u0] >= 0)[0][0])                          # the first scored candidate of user 0
    for tau in (-np.inf, np.float32(np.nextafter(scored.max(), np.float32(np.inf))), crit[u0, e0], np.float32(np.median(scored)), np.inf):
        g_s, g_i, st = new(n, k), new(n, k, dt=torch.int32), torch.full((n, 3), -7, dtype=torch.int32, device=eng.device)
        eng.topk_gate(c_s, c_i, cr["crit"], cr["anchor_i"], tau, k, g_s, g_i, st)
        torch.cuda.synchronize()
        w_s, w_i, w_st = KR.gate_ref(h(c_s), h(c_i), crit, flag, tau, k)
        assert np.array_equal(h(g_i), w_i) and np.array_equal(_bits(h(g_s)), _bits(w_s)) and np.array_equal(h(st), w_st), tau
        if tau == -np.inf:                                             # the plain top-k
            assert np.array_equal(h(g_i), h(p_i)) and np.array_equal(_bits(h(g_s)), _bits(h(p_s)))
            assert np.all(h(st)[:, 1] == 0)
        elif tau > scored.max():                                       # above every critic: no scored entry is served
            served = h(g_i)
            for u in range(n):
                assert not np.isin(served[u][served[u] >= 0], h(c_i)[u][flag[u] >= 0]).any(), u
            assert np.array_equal(h(st)[:, 0], (flag >= 0).sum(1)) and h(st)[:, 1].sum() > 0
        elif tau == crit[u0, e0] and (flag[u0, :e0 + 1] < 0).sum() + 1 <= k:
            assert h(c_i)[u0, e0] in h(g_i)[u0]                        # crit == tau passes (>=)


def test_refusals_launch_nothing():
    import torch
    from ltgan import _cabi as cabi
    buf = torch.full((1 << 16,), 1234.5, dtype=torch.float32, device="cuda")
    TK.check_refusals(cabi, cabi.load(), buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 1234.5).all()) and torch.cuda.current_stream().query()


# ---------------------------------------------------------------------------------------------- 5. the classes
@pytest.mark.parametrize("kind", ["plain", "min_slots", "cap"])
def test_recommender_with_critic(kind):
    """two chunks (64 + 26 users); the table equals the direct calls on the final lists of the whole split in one call, bit for bit; with
    ExposureCap the critic is fed by the second pass"""
    import torch
    from ltgan.trainer import Critic, ExposureCap, MinSlots, Recommender
    eng, ev, X, niche, valid, _ = _served(TINY)
    k, top = 100, 40
    labels = np.zeros(I, np.uint8)
    labels[list(niche)] = 1
    rule = dict(plain={}, min_slots=dict(rule=MinSlots(labels, 2, [0, 30])), cap=dict(cap=ExposureCap(3)))[kind]
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=64, **rule).run(rng_step=5, keep_prob=1.0)
    crt = Critic(niche, valid, top=top)
    rec = Recommender(eng, ev, k=k, chunk=64, critic=crt, **rule)
    ids, sc = rec.run(rng_step=5, keep_prob=1.0)
    assert np.array_equal(ids, plain_ids) and np.array_equal(_bits(sc), _bits(plain_sc))          # the critic changes no list
    tab = crt.table()
    assert tab["crit"].shape == tab["anchor_i"].shape == tab["anchor_s"].shape == (90, top) and tab["n_anchor"].shape == (90,)
    want = _eng_critic(eng, crt.sides, ev.rows(0, 90)[0], rec.ids, top)
    torch.cuda.synchronize()
    for key in ("crit", "anchor_s", "anchor_i", "n_anchor"):
        assert np.array_equal(_bits(tab[key]), _bits(want[key].cpu().numpy())), key
    pop_row = crt.sides.pop_row.cpu().numpy()
    n_anchor = np.array([(pop_row[X.indices[X.indptr[u]:X.indptr[u + 1]]] >= 0).sum() for u in range(90)])
    assert np.array_equal(tab["n_anchor"], n_anchor) and n_anchor[5] == 0 and (n_anchor > 0).sum() > 80
    is_cand = (ids[:, :top] >= 0) & (crt.sides.niche_row.cpu().numpy()[np.clip(ids[:, :top], 0, I - 1)] >= 0)
    assert np.array_equal(tab["anchor_i"] >= 0, is_cand & (n_anchor[:, None] > 0)) and (tab["anchor_i"] >= 0).sum() > 300
    s = crt.summary()
    assert s["scored"] == int((tab["anchor_i"] >= 0).sum()) and s["users_with_anchors"] == int((n_anchor > 0).sum()) and 0.0 < s["mean_prob"] < 1.0
    assert np.array_equal(np.asarray(want["n_scored"].cpu()), (tab["anchor_i"] >= 0).sum(1))


def test_recommender_with_gate():
    import torch
    from ltgan.trainer import Critic, CriticGate, Recommender
    eng, ev, X, niche, valid, _ = _served(TINY)
    k, c = 50, 120
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=64).run(rng_step=5, keep_prob=1.0)
    g0 = CriticGate(niche, valid, 0.0, candidates=c)
    ids0, sc0 = Recommender(eng, ev, k=k, chunk=64, gate=g0).run(rng_step=5, keep_prob=1.0)
    assert np.array_equal(ids0, plain_ids) and np.array_equal(_bits(sc0), _bits(plain_sc))       # min_prob = 0: the plain lists
    assert np.all(g0.stats()[:, 1] == 0) and np.array_equal(g0.stats()[:, 2], (plain_ids >= 0).sum(1))
    # a threshold in the middle of the critics the plain lists get: by hand on the whole split from the candidates
    probe = Critic(niche, valid)
    Recommender(eng, ev, k=k, chunk=64, critic=probe).run(rng_step=5, keep_prob=1.0)
    t = probe.table()
    p = float(1.0 / (1.0 + np.exp(-np.median(t["crit"][t["anchor_i"] >= 0].astype(np.float64)))))
    gate = CriticGate(niche, valid, p, candidates=c)
    crt = Critic(niche, valid)
    rec = Recommender(eng, ev, k=k, chunk=64, gate=gate, critic=crt)
    ids, sc = rec.run(rng_step=5, keep_prob=1.0)
    wide_ids, wide_sc = Recommender(eng, ev, k=c, chunk=64).run(rng_step=5, keep_prob=1.0)
    cr = _eng_critic(eng, gate.sides, ev.rows(0, 90)[0], torch.from_numpy(wide_ids).to(eng.device), c)
    w_s, w_i, w_st = KR.gate_ref(wide_sc, wide_ids, cr["crit"].cpu().numpy(), cr["anchor_i"].cpu().numpy(), gate.tau, k)
    assert np.array_equal(ids, w_i) and np.array_equal(_bits(sc), _bits(w_s)) and np.array_equal(gate.stats(), w_st)
    assert w_st[:, 1].sum() > 50 and not np.array_equal(ids, plain_ids)
    served = crt.table()                                               # the critic of the gated lists: every scored entry reaches tau
    assert np.all(served["crit"][served["anchor_i"] >= 0] >= gate.tau) and (served["anchor_i"] >= 0).sum() > 50


# ---------------------------------------------------------------------------------------------- 6. over item shards
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_critic_and_gate(world):
    run_ranks("dist_critic_worker.py", ["1001", "230"], world, "CRITIC_SHARDED_OK world=%d" % world)


# ---------------------------------------------------------------------------------------------- 7. the CLIs
def test_cli_on_askubuntu(tmp_path):
    import json
    import torch
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    from ltgan.dataset import EvalData
    from ltgan.trainer import Critic, CriticGate, LongTailReport, Recommender
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    niche, valid = lt.critic_sides(ds, n_items)
    ev = EvalData(tr, te, eng.device)

    # recommend.py --gate --critic against the classes
    gate, crt = CriticGate(niche, valid, 0.5), Critic(niche, valid, top=30)
    ids, sc = Recommender(eng, ev, k=100, gate=gate, critic=crt).run(rng_step=rc.RNG_STEP)
    tab = crt.table()
    torch.cuda.synchronize()
    out = run_cli("recommend.py", [ds, ck, "--gate", "0.5", "--critic", "30", "--critic-out", "c.tsv", "--out", "recs.tsv", "--npz", "recs.npz"], cwd)
    z = np.load(os.path.join(cwd, "recs.npz"))
    assert np.array_equal(z["ids"], ids) and np.array_equal(_bits(z["scores"]), _bits(sc))
    for key, name in (("crit", "crit"), ("anchor_i", "anchor_ids"), ("anchor_s", "anchor_scores"), ("n_anchor", "n_anchor")):
        assert np.array_equal(_bits(z[name]), _bits(tab[key])), key
    assert out[-2] == lt.gate_line(gate.stats(), 0.5, 100) and out[-1] == lt.critic_line(crt.summary(), 30)
    assert out[-3] == rc.summary_line(rc.long_tail_summary(ids, niche, n_items, te), 100)
    lines = open(os.path.join(cwd, "c.tsv")).read().splitlines()
    uu, ee = np.nonzero(tab["anchor_i"] >= 0)
    assert len(lines) == uu.size > 0
    sig = lambda x: 1.0 / (1.0 + np.exp(-float(x)))
    hist = tr.tocsr()
    for line, u, e in zip(lines, uu, ee):
        uid, sid, prob, anchor = line.split("\t")
        a, ap = anchor.split(":")
        assert int(uid) == uid0 + u and int(sid) == ids[u, e] and int(a) == tab["anchor_i"][u, e]
        assert abs(float(prob) - sig(tab["crit"][u, e])) <= 5.1e-7 and abs(float(ap) - sig(tab["anchor_s"][u, e])) <= 5.1e-7
        assert int(a) in hist.indices[hist.indptr[u]:hist.indptr[u + 1]] and int(sid) in niche and int(a) not in niche
        assert float(prob) >= 0.5 - 5.1e-7                             # the gate let it in
    # without the flags: the plain lists, no new line, no file
    plain = run_cli("recommend.py", [ds, ck, "--out", "plain.tsv", "--npz", "plain.npz"], cwd)
    p_ids, _ = Recommender(eng, ev, k=100).run(rng_step=rc.RNG_STEP)
    assert np.array_equal(np.load(os.path.join(cwd, "plain.npz"))["ids"], p_ids) and sorted(np.load(os.path.join(cwd, "plain.npz")).files) == ["ids", "scores", "uids"]
    assert plain[-1] == rc.summary_line(rc.long_tail_summary(p_ids, niche, n_items, te), 100) and not os.path.exists(os.path.join(cwd, "critic.tsv"))
    assert not any(l.startswith(("gate@", "critic@")) for l in plain)
    # longtail.py --gate --critic: the report of the gated lists, the summary in the JSON
    labels, names = lt.build_groups(ds, "niche", 2, n_items)
    report = LongTailReport(labels, 2, k_exp=100)
    gate2, crt2 = CriticGate(niche, valid, 0.5, candidates=150), Critic(niche, valid)
    ids2, _ = Recommender(eng, ev, k=100, report=report, gate=gate2, critic=crt2).run(rng_step=lt.RNG_STEP)
    rep = lt.aggregate(*report.table(), labels, names, 100)
    out = run_cli("longtail.py", [ds, ck, "--gate", "0.5", "--gate-candidates", "150", "--critic", "--json", "r.json"], cwd)
    assert out[-6:-2] == lt.report_lines(rep) and out[-2] == lt.gate_line(gate2.stats(), 0.5, 100) and out[-1] == lt.critic_line(crt2.summary(), 100)
    js = json.load(open(os.path.join(cwd, "r.json")))
    assert js["critic"] == dict(crt2.summary(), top=100) and js["all"]["ndcg"] == rep["all"]["ndcg"] and js["all"]["coverage"] == rep["all"]["coverage"]
    torch.cuda.synchronize()
