"""Replay of exploration logs on the GPU (tests/replay_ref.py is the reference): ltg_list_mass -- states, score bits and the maximum
exactly, the n_pol sums within the bound of DESIGN 5.21's derivation for the same fp32 sum, over both load paths, every kind of row,
planted unsupported entries and padding, slabs of a larger catalogue, ragged slabs combined, and n_pol = 8 against eight calls bit for
bit; ltg_replay_rows against the float64 reference; the exact identity over all 210 ordered lists of the eight-item catalogue on the
device; Recommender(replay=) on a log made by Recommender(explore=); the item-sharded recommender (tests/dist_replay_worker.py) and the
CLIs on Askubuntu_Sample in fresh child processes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import explore_ref as E
import replay_ref as R
import serving_harness
from serving_harness import DEV, _bits, _small_engine, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu
SHARDED = "test_gpu_replay::test_sharded_recommender_with_replay"
assert 29699 not in {port for _, port in serving_harness.PORTS.values()}, "the rendezvous port of the sharded test is taken"
serving_harness.PORTS[SHARDED] = ("dist_replay_worker.py", 29699)
REST_TOL = 4.4e-5          # 362 * 2^-24 for the fp32 sum (352 additions per thread + the tree), with its factor of two
LOGP_TOL = 1e-4            # the project's bound on |logp - reference| wherever x_j >= -80
TEMPS = [1.0, 0.5, 2.0, 0.7, 1.5, 3.0, 0.9, 1.2]
ITS = [E.inv_temp_of(T) for T in TEMPS]


def _cfg(cabi, n_items, item_lo=0, n_glob=0, seed=98765):
    return cabi.ltg_config(n_items, 600, 200, n_items, 100, 150, 250, 300, 0, 0, item_lo, n_glob, 1, 0, 1e-4, 0.9, 0.999, 1e-8, seed)


class _Slab:
    """the device side of the columns lo .. hi of host rows: the logits and the fold-in items with LOCAL ids, uploaded once"""

    def __init__(self, logits, fold, lo=0, hi=None, n_glob=0):
        from ltgan import _cabi as cabi
        from ltgan.engine import CsrRows
        hi = logits.shape[1] if hi is None else hi
        indptr, indices = E.csr_of(fold, lo, hi)
        self.n, self.lo, self.hi = logits.shape[0], lo, hi
        self.logits = _t(np.ascontiguousarray(logits[:, lo:hi]))
        self.tr = CsrRows(_t(indptr), _t(indices), 0, self.n)
        self.cfg = _cfg(cabi, hi - lo, lo, n_glob)


def _mass_dev(slab, ids, its, head=None):
    """ltg_list_mass through the C ABI -> host (score [n, k], state [n, k], max [n], rest [n_pol, n])"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, k = ids.shape
    f = 0 if head is None else head.shape[1]
    ex = _t(np.asarray(head, np.int32)) if f else None
    idd = _t(np.asarray(ids, np.int32))
    so = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)        # sentinels: an unwritten cell shows
    st = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    mo = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    ro = torch.full((len(its), n), -7.0, dtype=torch.float32, device=DEV)
    it = (C.c_float * 8)(*[float(x) for x in its])
    rc = lib.ltg_list_mass(C.byref(slab.cfg), slab.logits.data_ptr(), C.byref(slab.tr.c), n, k, idd.data_ptr(), f,
                           ex.data_ptr() if f else None, len(its), it, so.data_ptr(), st.data_ptr(), mo.data_ptr(), ro.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), st.cpu().numpy(), mo.cpu().numpy(), ro.cpu().numpy()


def _rows_dev(its, head, ids, logp0, y, score, state, M, rest, labels, n_groups, clip, want_logp1=True):
    """ltg_replay_rows through the C ABI on host arrays -> host (rows [n, P, G + 1, 2], w [n, P], first_bad [n, P], logp1 [P, n, k])"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, k = ids.shape
    P, G = len(its), int(n_groups)
    f = 0 if head is None else head.shape[1]
    keep = [_t(np.asarray(a, dt)) for a, dt in ((ids, np.int32), (logp0, np.float32), (y, np.float32), (score, np.float32), (state, np.int32),
                                                (M, np.float32), (rest, np.float32), (labels, np.uint8))]
    hd = _t(np.asarray(head, np.int32)) if f else None
    ro = torch.full((n, P, G + 1, 2), 7.0, dtype=torch.float64, device=DEV)
    wo = torch.full((n, P), 7.0, dtype=torch.float64, device=DEV)
    fo = torch.full((n, P), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((P, n, k), 7.0, dtype=torch.float32, device=DEV) if want_logp1 else None
    it = (C.c_float * 8)(*[float(x) for x in its])
    rc = lib.ltg_replay_rows(n, k, P, it, f, hd.data_ptr() if f else None, *[t.data_ptr() for t in keep[:7]], keep[7].data_ptr(), G,
                             len(labels), float(clip), ro.data_ptr(), wo.data_ptr(), fo.data_ptr(), lp.data_ptr() if lp is not None else None,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return ro.cpu().numpy(), wo.cpu().numpy(), fo.cpu().numpy(), lp.cpu().numpy() if lp is not None else None


def _close(a, b, rel):
    """a within a relative `rel` of b; both nan (an estimate over no supported row) counts as equal"""
    return (a != a and b != b) or abs(a - b) <= rel * abs(b)


def _heads(logits, fold, F):
    return np.stack([E.plain_topk(logits[r], fold[r], F)[0] for r in range(logits.shape[0])]) if F else np.zeros((logits.shape[0], 0), np.int32)


def _logged(logits, fold, g, k, head, f_in):
    """a logged list per row: the reference's own sample of k entries at T = 1 over the whole row, then planted: a fold-in item of the
    row, an item of the TARGET's head in a sampled slot, padding in the middle and at the end -> (ids [n, k], what was planted)"""
    n = logits.shape[0]
    ids = np.stack([E.sample_slab(logits[r], fold[r], k, np.float32(1.0), g[r])[0] for r in range(n)])
    planted = dict(fold=0, head=0, pad=0)
    for r in range(n):
        free = k - f_in
        used = set(ids[r].tolist())
        fo = [i for i in np.nonzero(fold[r])[0].tolist() if i not in used]
        if fo and (free >= 2 or r % 2):
            ids[r, f_in] = fo[0]
            planted["fold"] += 1
            used = set(ids[r].tolist())
        if free >= 2 and f_in:
            hd = [h for h in head[r].tolist() if h >= 0 and h not in used]
            if hd:
                ids[r, f_in + 1] = hd[0]
                planted["head"] += 1
            elif any(h >= 0 and h in ids[r, f_in:].tolist() for h in head[r].tolist()):
                planted["head"] += 1                     # (the sample holds one already)
        if free >= 5:
            ids[r, f_in + 2] = ids[r, k - 1] = -1
            planted["pad"] += 1
        real = ids[r][ids[r] >= 0]
        assert len(set(real.tolist())) == len(real)
    return ids, planted


def _check_mass(got, logits, fold, ids, its, head, f_in, lo, hi, what):
    """one device call against the reference: states, score bits and the maximum exactly, the sums within REST_TOL -> worst relative error"""
    gs, gst, gm, gr = got
    worst = 0.0
    for r in range(logits.shape[0]):
        ws, wst, wm, wr = R.list_mass(logits[r, lo:hi], fold[r, lo:hi], ids[r], its, excl=head[r] if f_in else (), f_in=f_in, item_lo=lo)
        assert np.array_equal(gst[r], wst), (what, r, gst[r][:12], wst[:12])
        assert np.array_equal(_bits(gs[r]), _bits(ws)) and gm[r] == wm, (what, r)            # (the maximum by value: -0.0 == +0.0)
        for p in range(len(its)):
            err = abs(float(gr[p, r]) - wr[p])
            assert err <= REST_TOL * wr[p], (what, r, p, float(gr[p, r]), wr[p])
            worst = max(worst, err / wr[p] if wr[p] > 0 else 0.0)
    return worst


# ---------------------------------------------------------------------------------------------- 1. ltg_list_mass
@pytest.mark.parametrize("n_items", [1, 3, 63, 64, 65, 1027, 4096, 5001])
def test_list_mass_states_scores_maximum_and_sums_against_the_reference(n_items):
    logits, fold, g, kinds = E.build_rows(500 + n_items, n_items)
    slab = _Slab(logits, fold)
    worst, planted = 0.0, dict(fold=0, head=0, pad=0)
    for f_in in (0, 1, 7):
        head = _heads(logits, fold, f_in)
        for k in (1, 5, 64, 65, 100, 1024):
            if f_in >= k:
                continue
            ids, pl = _logged(logits, fold, g, k, head, f_in)
            planted = {key: planted[key] + pl[key] for key in planted}
            got8 = _mass_dev(slab, ids, ITS, head)
            worst = max(worst, _check_mass(got8, logits, fold, ids, ITS, head, f_in, 0, n_items, (n_items, f_in, k)))
            for n_pol in (1, 3):                         # fewer policies: the same bits as the first columns of eight
                got = _mass_dev(slab, ids, ITS[:n_pol], head)
                assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[:3], got8[:3])), (n_items, f_in, k, n_pol)
                assert np.array_equal(_bits(got[3]), _bits(got8[3][:n_pol])), (n_items, f_in, k, n_pol)
            if (f_in, k) in ((0, 1), (1, 65), (7, 1024)):
                # n_pol = 8 in one call equals eight calls at n_pol = 1, bit for bit; and twice in a row the same bits
                for p in range(8):
                    one = _mass_dev(slab, ids, ITS[p:p + 1], head)
                    assert np.array_equal(_bits(one[3][0]), _bits(got8[3][p])) and np.array_equal(_bits(one[0]), _bits(got8[0])), (n_items, k, p)
                again = _mass_dev(slab, ids, ITS, head)
                assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, got8))
    print("n_items %d: largest relative error of a sum %.3g, planted %s" % (n_items, worst, planted))
    assert planted["pad"] > 0 and (n_items < 63 or (planted["fold"] > 0 and planted["head"] > 0))


@pytest.mark.parametrize("n_items,lo", [(65, 60), (1027, 500), (4096, 1028)])
def test_list_mass_on_a_slab_of_a_larger_catalogue(n_items, lo):
    """item_lo > 0: global ids, a head and logged entries that lie partly outside the slab, fold-in items in the slab's LOCAL ids"""
    n_glob = lo + n_items + 137
    logits, fold, g, kinds = E.build_rows(600 + n_items, n_glob)
    slab = _Slab(logits, fold, lo, lo + n_items, n_glob)
    outside = 0
    for f_in in (0, 1, 7):
        head = _heads(logits, fold, f_in)
        for k in (5, 65, 1024):
            if f_in >= k:
                continue
            ids, _ = _logged(logits, fold, g, k, head, f_in)
            outside += int(((ids >= 0) & ((ids < lo) | (ids >= lo + n_items))).sum())
            for n_pol in (1, 3, 8):
                got = _mass_dev(slab, ids, ITS[:n_pol], head)
                _check_mass(got, logits, fold, ids, ITS[:n_pol], head, f_in, lo, lo + n_items, (n_items, lo, f_in, k, n_pol))
                own = (ids >= lo) & (ids < lo + n_items)
                assert (got[1][~own] == 0).all() and np.isneginf(got[0][~own]).all()
    assert outside > 0


@pytest.mark.parametrize("cuts", [(500,), (64, 700), (3, 1024)])
def test_ragged_slabs_combine_into_the_whole_row(cuts):
    I, k, f_in = 1027, 100, 7
    logits, fold, g, kinds = E.build_rows(700 + len(cuts) + cuts[0], I)
    head = _heads(logits, fold, f_in)
    ids, _ = _logged(logits, fold, g, k, head, f_in)
    whole = _mass_dev(_Slab(logits, fold, n_glob=I), ids, ITS, head)
    edges = (0,) + tuple(cuts) + (I,)
    parts = [_mass_dev(_Slab(logits, fold, a, b, I), ids, ITS, head) for a, b in zip(edges[:-1], edges[1:])]
    for r in range(logits.shape[0]):
        sc, st, M, rest = R.combine([(p[0][r], p[1][r], p[2][r], p[3][:, r].astype(np.float64)) for p in parts], ITS)
        assert np.array_equal(st, whole[1][r]) and np.array_equal(_bits(sc), _bits(whole[0][r])) and M == whole[2][r], (cuts, r, kinds[r])
        _, _, _, want = R.list_mass(logits[r], fold[r], ids[r], ITS, excl=head[r], f_in=f_in)
        assert (np.abs(rest - want) <= REST_TOL * want).all(), (cuts, r, kinds[r], rest, want)


# ---------------------------------------------------------------------------------------------- 2. ltg_replay_rows
def _case(n, k, F0, F1, seed, I=1200, T0=1.0, temps=(0.5, 1.0, 2.0), dominant=False, n_groups=3):
    """n logged rows of k entries made by the reference's own logging policy (T0, F0) with injected noise, their float64 replay under
    (temps, F1), and the device inputs taken from that reference -> dict"""
    rng = np.random.default_rng(seed)
    if dominant:
        S = rng.random((n, I)).astype(np.float32)
        S[np.arange(n), rng.integers(0, I, n)] = 7.0
    else:
        S = (2.0 * rng.standard_normal((n, I))).astype(np.float32)
    fold = rng.random((n, I)) < 0.03
    G = E.gumbel_of_uniform(rng.random((n, I), dtype=np.float32))
    labels = rng.integers(0, n_groups + (1 if n_groups < 8 else 0), I).astype(np.uint8)     # (a label n_groups: in no group)
    its = [E.inv_temp_of(T) for T in temps]
    ids = np.empty((n, k), np.int32)
    lp0 = np.empty((n, k), np.float32)
    for r in range(n):
        w = E.explore_row(S[r], fold[r], k, F0, E.inv_temp_of(T0), G[r])
        ids[r], lp0[r] = w["ids"], w["logp"].astype(np.float32)
    y = (rng.random((n, k)) < 0.3).astype(np.float32) * rng.integers(1, 4, (n, k)).astype(np.float32)
    return dict(S=S, fold=fold, labels=labels, its=its, ids=ids, lp0=lp0, y=y, F1=F1, n_groups=n_groups, k=k, n=n)


def _replay_against_reference(c, clip, what):
    """the device call on the reference's own merged values against the reference -> the worst differences"""
    n, k, P, G = c["n"], c["k"], len(c["its"]), c["n_groups"]
    ref = [R.replay_full_row(c["S"][r], c["fold"][r], c["ids"][r], c["lp0"][r], c["y"][r], c["F1"], c["its"], c["labels"], G, clip)
           for r in range(n)]
    x = np.stack([o["x"] for o in ref])
    assert (x[np.isfinite(x)] >= -80).all(), what                        # every listed entry is inside the contract of logp
    head = np.stack([o["head"] for o in ref]) if c["F1"] else None
    rows, w, fb, lp1 = _rows_dev(c["its"], head, c["ids"], c["lp0"], c["y"], np.stack([o["score"] for o in ref]),
                                 np.stack([o["state"] for o in ref]), np.array([o["M"] for o in ref]),
                                 np.stack([o["rest"] for o in ref]).T.astype(np.float32), c["labels"], G, clip)
    worst = dict(logp1=0.0, c=0.0, w=0.0)
    for r, o in enumerate(ref):
        real = c["ids"][r] >= 0
        last = int(np.nonzero(real)[0][-1]) if real.any() else -1
        for p in range(P):
            assert fb[r, p] == o["first_bad"], (what, r, p)
            want = o["logp1"][p]
            fin = np.isfinite(want)
            assert np.array_equal(np.isneginf(lp1[p, r]), np.isneginf(want)) and (lp1[p, r][~real] == 0).all(), (what, r, p)
            d = np.abs(lp1[p, r][fin].astype(np.float64) - want[fin])
            assert (d <= LOGP_TOL).all(), (what, r, p, float(d.max()))
            worst["logp1"] = max(worst["logp1"], float(d.max()) if d.size else 0.0)
            # c_j from the device's logp1, before the first unsupported slot: within (j + 1) x 1e-4
            dc = np.where(real & fin, np.where(fin, lp1[p, r].astype(np.float64), 0.0) - c["lp0"][r], 0.0).cumsum()
            j = np.arange(k)[: o["first_bad"]]
            assert (np.abs(dc[j] - o["c"][p][j]) <= (j + 1) * LOGP_TOL).all(), (what, r, p)
            worst["c"] = max(worst["c"], float(np.abs(dc[j] - o["c"][p][j]).max()) if j.size else 0.0)
            # w at the last slot, A and B: every term within a relative expm1((j + 1) x 1e-4) <= expm1((last + 1) x 1e-4)
            rel = np.expm1((last + 1) * LOGP_TOL)
            assert abs(w[r, p] - o["W"][p]) <= rel * o["W"][p], (what, r, p, w[r, p], o["W"][p])
            absA = np.array([(o["w"][p] * np.abs(c["y"][r]))[(c["labels"][np.where(real, c["ids"][r], 0)] == g) & real].sum() for g in range(G)]
                            + [(o["w"][p] * np.abs(c["y"][r])).sum()])
            assert (np.abs(rows[r, p, :, 0] - o["A"][p]) <= rel * absA + 1e-300).all(), (what, r, p, rows[r, p, :, 0], o["A"][p])
            assert (np.abs(rows[r, p, :, 1] - o["B"][p]) <= rel * o["B"][p] + 1e-300).all(), (what, r, p, rows[r, p, :, 1], o["B"][p])
            if o["W"][p] > 0:
                worst["w"] = max(worst["w"], abs(w[r, p] - o["W"][p]) / o["W"][p])
    return worst, ref, (rows, w, fb, lp1)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 1024])
def test_replay_rows_against_the_float64_reference(k):
    worst = dict(logp1=0.0, c=0.0, w=0.0)
    for n in (1, 3, 5):                                  # (5: one more than the four waves of a workgroup)
        for F0, F1 in ((0, 0), (0, min(7, k - 1)), (min(2, k - 1), min(7, k - 1))):
            c = _case(n, k, F0, F1, 1000 * k + 10 * n + F1)
            if k >= 5 and n >= 3:                        # a fold-in item in a sampled slot of row 1, padding in the middle and at the end of row 2
                fo = [i for i in np.nonzero(c["fold"][1])[0].tolist() if i not in c["ids"][1].tolist()]
                c["ids"][1, k - 2] = fo[0]
                for j in (F1 + 1, k - 1):
                    c["ids"][2, j], c["lp0"][2, j] = -1, 0.0
            got, _, _ = _replay_against_reference(c, 100.0, (k, n, F0, F1))
            worst = {key: max(worst[key], got[key]) for key in worst}
    print("k %d: largest |logp1 - reference| %.3g, |c_j - reference| %.3g, relative error of W %.3g" % (k, worst["logp1"], worst["c"], worst["w"]))


def test_replay_rows_clipping_wrong_heads_padding_zero_rewards_and_group_range():
    # clipping below, at and above a row's weights (a logging temperature far from the targets' makes the weights large and small)
    c = _case(5, 20, 0, 0, 77, T0=1.0, temps=(0.5, 2.0))
    _, ref, _ = _replay_against_reference(c, 1e300, "no clip")
    W = np.array([o["W"] for o in ref])
    assert W.max() > 10 * W.min() > 0
    for clip in (W.min() * 0.5, float(W[2, 0]), float(np.median(W)), W.max() * 2.0):
        _, ref_c, (rows, w, fb, lp1) = _replay_against_reference(c, clip, ("clip", clip))
        assert (w <= clip * (1 + 1e-12)).all() and (fb == 20).all()
        if clip < W.min():                               # below every row's weight: every W is the clip
            assert (np.abs(w - clip) <= 1e-12 * clip).all()
        if clip > W.max():                               # above: nothing is cut at the last slot
            assert (np.abs(w - W) <= np.expm1(20 * LOGP_TOL) * W).all()
    # a wrong head entry at slot 0 and at slot F' - 1; an all-padding row; y = 0 everywhere; n_groups at both ends of its range
    for n_groups in (1, 8):
        c = _case(5, 12, 7, 7, 78 + n_groups, n_groups=n_groups)
        spare = [i for i in range(1200) if i not in c["ids"][0].tolist() and i not in c["ids"][1].tolist() and not c["fold"][:2, i].any()]
        c["ids"][0, 0], c["ids"][1, 6] = spare[0], spare[1]
        c["ids"][3], c["lp0"][3] = -1, 0.0
        c["y"][4] = 0.0
        _, ref, (rows, w, fb, lp1) = _replay_against_reference(c, 100.0, ("heads", n_groups))
        assert (fb[0] == 0).all() and (fb[1] == 6).all() and (fb[2:] == 12).all()
        assert (rows[0] == 0).all() and (w[:2] == 0).all() and (rows[1, :, n_groups, 1] == 6.0).all()      # six head slots of weight exactly 1
        assert (w[3] == 1.0).all() and (rows[3] == 0).all() and (lp1[:, 3] == 0).all()
        assert (rows[4, :, :, 0] == 0).all() and (rows[4, :, n_groups, 1] > 0).all()
        assert tuple(rows.shape) == (5, 3, n_groups + 1, 2)
    # twice in a row: the same bits
    c = _case(3, 65, 2, 7, 80)
    _, _, a = _replay_against_reference(c, 100.0, "again")
    _, _, b = _replay_against_reference(c, 100.0, "again")
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_replay_rows_at_a_low_temperature_with_one_dominant_item():
    """T = 0.1, one item 7 above the others: the entries after it have x in [-70, -60], inside the contract, where only the
    positive-terms form keeps their logp"""
    c = _case(5, 20, 0, 0, 81, temps=(0.1,), dominant=True)
    got, ref, _ = _replay_against_reference(c, 100.0, "dominant")
    x = np.stack([o["x"][0] for o in ref])
    assert (x >= -80).all() and np.sort(x, 1)[:, -2].max() < -55
    print("largest |logp1 - reference| %.3g" % got["logp1"])


# ---------------------------------------------------------------------------------------------- 3. the exact identity on the device
@pytest.mark.parametrize("pair", R.ENUM_PAIRS)
def test_reweighted_reward_over_every_logged_list_equals_the_targets_expectation(pair):
    (T0, F0), (T1, F1) = pair
    Y, labels = R.enum_tables()
    lists, pi0, logp0 = R.enumerate_policy(T0, F0)
    n = len(lists)
    assert n == (210 if F0 == 0 else 30)
    logits = np.tile(E.PAIR_LOGITS, (n, 1))
    fold = np.zeros((n, 8), bool)
    fold[:, R.ENUM_FOLD] = True
    its = [E.inv_temp_of(T1)]
    head = _heads(logits, fold, F1)
    sc, st, M, rest = _mass_dev(_Slab(logits, fold), lists, its, head if F1 else None)
    y = Y[lists, np.arange(R.ENUM_K)[None, :]]
    rows, w, fb, _ = _rows_dev(its, head if F1 else None, lists, logp0, y, sc, st, M, rest, labels, 2, 1e30, want_logp1=False)
    if (F0, F1) == (0, 1):
        assert int((fb[:, 0] == R.ENUM_K).sum()) == 30
    wantA, wantB = R.target_value(T1, F1, Y, labels)
    gotA, gotB = (pi0[:, None] * rows[:, 0, :, 0]).sum(0), (pi0[:, None] * rows[:, 0, :, 1]).sum(0)
    tol = np.expm1(3e-4)
    print("(%g, %d) -> (%g, %d): sum pi0 A %s against %s, sum pi0 B over all groups %.9f" % (T0, F0, T1, F1, gotA, wantA, gotB[2]))
    assert (np.abs(gotA - wantA) <= tol * wantA).all() and (np.abs(gotB - wantB) <= tol * wantB).all()
    assert abs(gotB[2] - 3.0) <= tol * 3.0


# ---------------------------------------------------------------------------------------------- 4. the host layer
@pytest.mark.parametrize("I", [1001, 1537])
def test_recommender_with_replay(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.serving import replay_estimates
    from ltgan.trainer import Explore, Recommender, Replay, ReplayLog
    rng = np.random.default_rng(I)
    n, k, T0, F0, step = 230, 20, 0.8, 2, 77
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = _small_engine(I)
    ev = EvalData(X, X, eng.device)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    exp = Explore(T0, fixed=F0, draw=4)
    ids, _ = Recommender(eng, ev, k=k, chunk=128, explore=exp).run(rng_step=step, keep_prob=1.0)
    y = (rng.random((n, k)) < 0.2).astype(np.float32)
    log = ReplayLog(ids, exp.table(), y, fixed=F0, n_items=I)
    temps = [T0, 0.5, 2.0]

    def run(chunk, fixed=None, k_rec=0):
        rp = Replay(log, temps, fixed=fixed, labels=labels, n_groups=3, keep_logp1=True)
        rec = Recommender(eng, ev, k=k_rec, chunk=chunk, replay=rp)
        rec.run(rng_step=step, keep_prob=1.0)
        return rp, rec

    rp, _ = run(128)                                                     # two chunks, as the log was made
    t, est = rp.table(), rp.estimates()
    # at the logging temperature: every row is supported, logp1 is logp0, the weights are 1
    bound = np.expm1(k * 2e-4)
    assert (t["first_bad"] == k).all() and est[T0]["supported"] == 1.0
    d = float(np.abs(t["logp1"][0].astype(np.float64) - log.logp0).max())
    print("I %d: largest |logp1 - logp0| at the logging temperature %.3g, ess %.3f of %d" % (I, d, est[T0]["ess"], n))
    assert d <= 2e-4
    assert abs(est[T0]["ess"] - n) <= bound * n
    assert abs(est[T0]["all"]["ips"] - float(y.sum()) / n) <= bound * float(y.sum()) / n and est[T0]["all"]["logged"] == float(y.sum()) / n
    assert abs(est[T0]["all"]["exposure"] - k) <= bound * k
    # the chunk size does not change the per-row table, bit for bit; nor does serving plain lists beside it
    for chunk, k_rec in ((77, 0), (n, 0), (128, 10)):
        other, rec = run(chunk, k_rec=k_rec)
        t2 = other.table()
        assert all(np.array_equal(np.ascontiguousarray(t[key]).view(np.uint8), np.ascontiguousarray(t2[key]).view(np.uint8)) for key in t), chunk
    # against the reference, from the logits of the one-chunk run (still in the activations); also with a longer head
    for fixed in (None, 5):
        rp1, rec = run(n, fixed=fixed)
        F1 = rp1.fixed
        t1 = rp1.table()
        lg = rec.acts.logits.reshape(-1)[: n * I].view(n, I).cpu().numpy()
        fold = np.asarray(X.todense()) > 0
        ref = [R.replay_full_row(lg[r], fold[r], log.ids[r], log.logp0[r], y[r], F1, rp1.inv_temps, labels, 3, 100.0) for r in range(n)]
        x = np.stack([o["x"] for o in ref])
        assert (x[np.isfinite(x)] >= -80).all()
        assert np.array_equal(t1["state"], np.stack([o["state"] for o in ref])) and np.array_equal(_bits(t1["score"]), _bits(np.stack([o["score"] for o in ref])))
        assert np.array_equal(t1["M"], np.array([o["M"] for o in ref])) and np.array_equal(t1["first_bad"], np.array([[o["first_bad"]] * 3 for o in ref]))
        if fixed == 5:
            assert (t1["first_bad"] < k).any() and (t1["first_bad"] >= F0).all()      # a sampled slot 2 .. 4 rarely holds the target's head entry
        want1 = np.stack([o["logp1"] for o in ref], 1)
        fin = np.isfinite(want1)
        assert np.array_equal(np.isneginf(t1["logp1"]), np.isneginf(want1)) and np.abs(t1["logp1"][fin] - want1[fin]).max() <= LOGP_TOL
        rel = np.expm1(k * LOGP_TOL)
        wantA, wantB = np.stack([o["A"] for o in ref]), np.stack([o["B"] for o in ref])
        assert (np.abs(t1["rows"][..., 0] - wantA) <= rel * wantA).all() and (np.abs(t1["rows"][..., 1] - wantB) <= rel * wantB).all()
        wantW = np.stack([o["W"] for o in ref])
        assert (np.abs(t1["w"] - wantW) <= rel * wantW).all()
        want = replay_estimates(np.stack([wantA, wantB], -1), wantW, t1["first_bad"], log, temps, labels, 3)
        got = rp1.estimates()
        for T in temps:
            assert got[T]["supported"] == want[T]["supported"] and _close(got[T]["ess"], want[T]["ess"], 2 * rel)
            for name in ("0", "1", "2", "all"):
                for key in ("ips", "snips", "exposure"):
                    assert _close(got[T][name][key], want[T][name][key], 2 * rel), (T, name, key)
                assert got[T][name]["logged"] == want[T][name]["logged"]
    with pytest.raises(ValueError, match="the log holds"):
        Recommender(eng, EvalData(X[:100], X[:100], eng.device), k=0, chunk=128, replay=Replay(log, temps))
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2])
def test_sharded_recommender_with_replay(world):
    run_ranks("dist_replay_worker.py", ["1001", "230"], world, "REPLAY_SHARDED_OK world=%d" % world, port_of=SHARDED)


def test_cli_on_askubuntu(tmp_path):
    import torch
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    from ltgan import replay as rpm
    from ltgan.dataset import EvalData
    from ltgan.trainer import Recommender, Replay, ReplayLog
    n, k = tr.shape[0], 20
    run_cli("recommend.py", [ds, ck, "--explore", "1", "--k", k, "--keep-prob", "1.0", "--npz", "exp.npz", "--propensities", "props.tsv"], cwd)
    out = run_cli("replay.py", [ds, ck, "--log", "exp.npz", "--feedback", "heldout", "--temperature", "1,0.5,2", "--keep-prob", "1.0",
                                "--json", "replay.json"], cwd)
    print("\n".join(out[-9:]))
    lines = [l for l in out if l.startswith("replay T ")]
    assert len(lines) == 9 and lines[0].startswith("replay T 1 popular: ips ") and lines[2].startswith("replay T 1 all: ips ")
    assert lines[5].startswith("replay T 0.5 all: ips ") and lines[8].startswith("replay T 2 all: ips ")
    doc = json.load(open(os.path.join(cwd, "replay.json")))
    assert (doc["k"], doc["users"], doc["fixed"], doc["logged_fixed"]) == (k, n, 0, 0) and [p["temperature"] for p in doc["policies"]] == [1.0, 0.5, 2.0]
    # the T = 1 line: the logging policy itself
    log = ReplayLog.from_npz(os.path.join(cwd, "exp.npz"), n_items=n_items)
    log.rewards_from(te)
    p1, bound = doc["policies"][0], np.expm1(k * 2e-4)
    logged = float(log.reward.sum()) / n
    assert p1["supported"] == 1.0 and abs(p1["ess"] - n) <= bound * n
    assert abs(p1["all"]["ips"] - logged) <= bound * logged and p1["all"]["logged"] == logged and abs(p1["all"]["exposure"] - k) <= bound * k
    field = lambda line, name: float(line.split(name + " ")[1].split(",")[0].split("/")[0].split(" ")[0])
    assert abs(field(lines[2], "ips") - p1["all"]["ips"]) <= 5e-7 and abs(field(lines[2], "exposure") - p1["all"]["exposure"]) <= 5e-5
    assert lines[2].endswith("ess %.1f of %d, supported 1.0000" % (p1["ess"], n))
    # the JSON against the class, in this process
    labels, names = lt.build_groups(ds, "niche", 2, n_items)
    rp = Replay(log, [1.0, 0.5, 2.0], labels=labels, n_groups=2)
    Recommender(eng, EvalData(tr, te, eng.device), k=0, replay=rp).run(rng_step=rc.RNG_STEP, keep_prob=1.0)
    est = rp.estimates(names)
    assert rpm.replay_lines(est, names) == lines
    for p, T in zip(doc["policies"], (1.0, 0.5, 2.0)):
        for name in names + ["all"]:
            assert p[name] == pytest.approx(est[T][name], rel=1e-12, abs=0, nan_ok=True), (T, name)
        assert p["ess"] == pytest.approx(est[T]["ess"], rel=1e-12) and p["supported"] == est[T]["supported"]
    # the tsv log against the npz log: logp0 differs by the %.6g of props.tsv, at most 5e-6 of each value plus its float32 rounding
    out_tsv = run_cli("replay.py", [ds, ck, "--log", "props.tsv", "--feedback", "heldout", "--temperature", "1,0.5,2", "--json", "replay_tsv.json"], cwd)
    doc_tsv = json.load(open(os.path.join(cwd, "replay_tsv.json")))
    rel = np.expm1(float(((5e-6 + 2.0 ** -24) * np.abs(log.logp0.astype(np.float64))).sum(1).max()))
    print("tsv against npz: bound on a weight's relative difference %.3g" % rel)
    assert len([l for l in out_tsv if l.startswith("replay T ")]) == 9 and doc_tsv["k"] == k
    for p, q in zip(doc["policies"], doc_tsv["policies"]):
        assert q["supported"] == p["supported"] and abs(q["ess"] - p["ess"]) <= 4 * rel * p["ess"]
        for name in names + ["all"]:
            for key in ("ips", "snips", "exposure"):
                assert abs(q[name][key] - p[name][key]) <= 2 * rel * abs(p[name][key]), (name, key)
            assert q[name]["logged"] == p[name]["logged"]
    torch.cuda.synchronize()
