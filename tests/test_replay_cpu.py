"""CPU-side checks of the replay of exploration logs: ltg_list_mass / ltg_replay_rows are exported and bound with the header's
argument types, every documented refusal returns LTG_EINVAL without a GPU, ReplayLog / Replay / replay= validate, the npz and tsv readers
round-trip what recommend.py writes, replay.py refuses bad arguments, and the numpy reference the GPU tests lean on (tests/replay_ref.py)
is exact: over all 210 ordered lists of the eight-item catalogue the re-weighted reward equals the target's expectation."""
import ctypes as C
import os

import numpy as np
import pytest

import explore_ref as E
import replay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32, pf = C.c_void_p, C.c_int32, C.POINTER(C.c_float)
    cfg, bt = C.POINTER(cabi.ltg_config), C.POINTER(cabi.ltg_batch)
    want = {"ltg_list_mass": [cfg, vp, bt, i32, i32, vp, i32, vp, i32, pf, vp, vp, vp, vp, vp],
            "ltg_replay_rows": [i32, i32, i32, pf, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, vp, vp]}
    for name, args in want.items():
        assert cabi.SYMBOLS[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert ("int ltg_list_mass(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, const int32_t* id_in, "
            "int32_t f_in,") in header
    assert "int ltg_replay_rows(int32_t n_rows, int32_t k, int32_t n_pol, const float* inv_temp, int32_t f_in, const int32_t* head_id," in header
    assert "#define LTG_REPLAY_MAX_POLICIES 8" in header
    assert header.index("int ltg_topk_sample_finish(") < header.index("int ltg_list_mass(")
    hip = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_kernels.hip")).read()
    assert hip.index('#include "ltg_explore.h"') < hip.index('#include "ltg_replay.h"')


def _cfg(cabi, n_items=1000, item_lo=0, n_glob=0):
    return cabi.ltg_config(n_items, 600, 200, n_items, 100, 150, 250, 300, 0, 0, item_lo, n_glob, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


def test_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    fb, ib, db, bb = (C.c_float * 64)(), (C.c_int32 * 64)(), (C.c_double * 64)(), (C.c_uint8 * 64)()
    good = _cfg(cabi)
    temps = lambda *v: (C.c_float * 8)(*v)
    one = temps(1.0)

    def batch(n_rows=2, indptr=True, indices=True):
        return cabi.ltg_batch(n_rows, 0, C.addressof(ib) if indptr else None, C.addressof(ib) if indices else None, None, None, None, None, None,
                              None, None)

    def mass(cfg=good, logits=fb, tr=None, n=2, k=4, ids=ib, f=0, excl=None, n_pol=1, it=one, so=fb, st=ib, mo=fb, ro=fb):
        return lib.ltg_list_mass(C.byref(cfg) if cfg is not None else None, logits, C.byref(tr) if tr is not None else None, n, k, ids, f, excl,
                                 n_pol, it, so, st, mo, ro, None)

    def rows(n=2, k=4, n_pol=1, it=one, f=0, head=None, ids=ib, lp0=fb, y=fb, sc=fb, st=ib, M=fb, rest=fb, lab=bb, n_groups=2, n_glob=50, clip=100.0,
             ro=db, wo=db, fo=ib, lp1=None):
        return lib.ltg_replay_rows(n, k, n_pol, it, f, head, ids, lp0, y, sc, st, M, rest, lab, n_groups, n_glob, clip, ro, wo, fo, lp1, None)

    # zero rows: nothing is launched, but the arguments are still checked
    assert mass(n=0) == 0 and rows(n=0) == 0
    assert mass(n=0, k=1024, excl=ib, f=7, tr=batch(0), n_pol=8, it=temps(*[0.5 + p for p in range(8)])) == 0
    assert rows(n=0, k=1024, head=ib, f=1023, n_pol=8, it=temps(*[0.5 + p for p in range(8)]), n_groups=8, lp1=fb, clip=1e-3) == 0
    for call, outs in ((mass, ("ids", "it", "so", "st", "mo", "ro")),
                       (rows, ("it", "ids", "lp0", "y", "sc", "st", "M", "rest", "lab", "ro", "wo", "fo"))):
        for name in outs:
            assert call(**{name: None}) == -1 and call(n=0, **{name: None}) == -1, (call.__name__, name)
        for k in (0, -1, 1025):
            assert call(k=k) == -1 and call(n=0, k=k) == -1, (call.__name__, k)
        for n_pol in (0, -1, 9):
            assert call(n_pol=n_pol) == -1 and call(n=0, n_pol=n_pol) == -1, (call.__name__, n_pol)
        for bad in (0.0, -1.0, float("inf"), -float("inf"), float("nan")):
            assert call(it=temps(bad)) == -1 and call(n=0, it=temps(bad)) == -1, (call.__name__, bad)
            assert call(n_pol=3, it=temps(1.0, 2.0, bad)) == -1 and call(n=0, n_pol=2, it=temps(1.0, 2.0, bad)) == 0, (call.__name__, bad)
        assert call(n=-1) == -1
        assert call(f=-1) == -1 and call(f=4) == -1 and call(f=5) == -1 and call(n=0, f=4) == -1        # 0 <= f_in < k
    assert mass(f=-1, excl=ib) == -1 and mass(f=3, excl=None) == -1 and mass(n=0, f=3) == -1
    assert rows(f=-1, head=ib) == -1 and rows(f=3, head=None) == -1 and rows(n=0, f=3) == -1
    assert mass(cfg=None) == -1 and mass(logits=None) == -1
    assert mass(cfg=_cfg(cabi, 0)) == -1 and mass(cfg=_cfg(cabi, -5)) == -1                       # what ltg_topk refuses
    assert mass(cfg=_cfg(cabi, 425985)) == -1                                                     # (a slab beyond the LDS bitset)
    assert mass(cfg=_cfg(cabi, 1000, item_lo=-1)) == -1
    assert mass(tr=batch(3)) == -1 and mass(tr=batch(indptr=False)) == -1 and mass(tr=batch(indices=False)) == -1
    assert mass(n=0, tr=batch(0)) == 0 and mass(n=0, cfg=_cfg(cabi, 360448)) == 0
    for clip in (0.0, -1.0, float("inf"), float("nan")):
        assert rows(clip=clip) == -1 and rows(n=0, clip=clip) == -1, clip
    for g in (0, -1, 9):
        assert rows(n_groups=g) == -1 and rows(n=0, n_groups=g) == -1, g
    assert rows(n_glob=0) == -1 and rows(n_glob=-3) == -1


class _FakeEngine:
    I, I_global, device, item_lo = 50, 50, "cpu", 0


def _log(n=6, k=5, fixed=0, seed=0):
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(50)[:k] for _ in range(n)]).astype(np.int32)
    logp = -rng.random((n, k)).astype(np.float32)
    logp[:, :fixed] = 0
    return ids, logp, (rng.random((n, k)) < 0.3).astype(np.float32)


def test_replay_log_validation():
    from ltgan.serving import ReplayLog as ServingLog
    from ltgan.sharded import ReplayLog as ShardedLog
    from ltgan.trainer import ReplayLog
    assert ServingLog is ShardedLog is ReplayLog
    ids, logp, y = _log()
    log = ReplayLog(ids, logp, y, n_items=50)
    assert (log.n, log.k, log.fixed) == (6, 5, 0) and log.ids.dtype == np.int32 and log.logp0.dtype == log.reward.dtype == np.float32

    def bad(match, ids=ids, logp=logp, y=y, **kw):
        with pytest.raises(ValueError, match=match):
            ReplayLog(ids, logp, y, **kw)

    bad("one shape", logp=logp[:, :4])
    bad("one shape", ids=ids[0])
    bad(r"reward must be", y=y[:5])
    bad(r"k must be in \[1, 1024\]", ids=np.zeros((2, 0), np.int32), logp=np.zeros((2, 0), np.float32), y=np.zeros((2, 0), np.float32))
    bad(r"k must be in \[1, 1024\]", ids=np.tile(np.arange(1025, dtype=np.int32), (1, 1)), logp=np.zeros((1, 1025), np.float32),
        y=np.zeros((1, 1025), np.float32))
    bad("fixed", fixed=5)
    bad("fixed", fixed=-1)
    bad("fixed", fixed=1.5)
    bad("integers", ids=ids.astype(np.float32))
    for r, v in ((3, 50), (2, -2)):
        x = ids.copy()
        x[r, 1] = v
        bad("row %d has an id" % r, ids=x, n_items=50)
    x = ids.copy()
    x[4, 3] = x[4, 0]
    bad("row 4 holds an item twice", ids=x)
    for v in (0.5, np.nan, -np.inf):
        x = logp.copy()
        x[1, 2] = v
        bad("row 1 has a logp0", logp=x)
    x, lp = ids.copy(), logp.copy()
    x[5, 3:] = -1                                                        # two paddings are not "an item twice" ...
    bad("row 5 has a logp0 other than 0.0 on padding", ids=x)            # ... but their logp0 must be 0.0
    lp[5, 3:] = 0
    assert ReplayLog(x, lp, y).k == 5
    bad("row 0 has a logp0 other than 0.0 in the fixed head", fixed=2)
    x = y.copy()
    x[2, 2] = np.inf
    bad("row 2 has a reward", y=x)
    assert ReplayLog(ids, logp).reward is None
    with pytest.raises(ValueError, match="uids"):
        ReplayLog(ids, logp, y, uids=np.arange(5))


def test_replay_validation_and_the_recommender_keyword():
    from ltgan.trainer import Diversify, Recommender, Replay, ReplayLog
    ids, logp, y = _log(fixed=2)
    log = ReplayLog(ids, logp, y, fixed=2)
    with pytest.raises(ValueError, match="no rewards"):
        Replay(ReplayLog(ids, logp, fixed=2), [1.0])
    for T in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            Replay(log, [1.0, T])
    with pytest.raises(ValueError, match="between 1 and 8"):
        Replay(log, [])
    with pytest.raises(ValueError, match="between 1 and 8"):
        Replay(log, [1.0] * 9)
    for F in (0, 1, 5, 2.5):                                             # F' < F0 has no support; F' < k
        with pytest.raises(ValueError, match="fixed"):
            Replay(log, [1.0], fixed=F)
    for clip in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="clip"):
            Replay(log, [1.0], clip=clip)
    with pytest.raises(ValueError):
        Replay(log, [1.0], n_groups=2)
    with pytest.raises(ValueError):
        Replay(log, [1.0], labels=np.zeros(50, np.uint8), n_groups=9)
    rp = Replay(log, 0.5)
    assert rp.fixed == 2 and rp.inv_temps == [np.float32(2.0)] and rp.inv_temps[0].dtype == np.float32 and rp.n_groups == 1
    rp = Replay(log, [1.0, 0.3, 2.0], fixed=4, clip=7, labels=np.arange(50) % 3, keep_logp1=True)
    assert rp.fixed == 4 and rp.inv_temps[1] == E.inv_temp_of(0.3) and rp.n_groups == 3 and rp.clip == 7.0
    with pytest.raises(ValueError, match="the log holds 6 users, the split 7"):
        rp.bind(_FakeEngine(), 4, 7)
    rp.bind(_FakeEngine(), 4, 6)
    assert tuple(rp.rows.shape) == (6, 3, 4, 2) and tuple(rp.w.shape) == (6, 3) and tuple(rp.logp1.shape) == (3, 6, 5)
    assert rp.head_i.numel() == 16 and tuple(rp.rest.shape) == (12,) and rp.rows.dtype.is_floating_point and rp.rows.element_size() == 8
    with pytest.raises(ValueError, match="labels hold"):
        Replay(log, [1.0], labels=np.zeros(49, np.uint8), n_groups=1).bind(_FakeEngine(), 4, 6)
    big = ReplayLog(ids + 10, logp, y, fixed=2)                          # an id outside the catalogue shows at bind time
    with pytest.raises(ValueError, match="has an id outside"):
        Replay(big, [1.0]).bind(_FakeEngine(), 4, 6)
    # replay= goes beside a rule and with k = 0: the first refusal is the rule's own
    with pytest.raises(ValueError, match="diversify= cannot be combined with rule="):
        Recommender(_FakeEngine(), None, k=10, rule=object(), diversify=Diversify(0.5), replay=Replay(log, [1.0]))
    import inspect
    assert "replay" in inspect.signature(Recommender.__init__).parameters


def test_readers_round_trip_what_recommend_py_writes(tmp_path):
    from ltgan import recommend as rc
    from ltgan.trainer import ReplayLog
    ids, logp, y = _log(n=4, k=6, fixed=1, seed=3)
    ids[2, 4:] = -1
    logp[2, 4:] = 0
    logp[1, 3] = np.float32(-2.5e-7)
    npz, tsv = str(tmp_path / "r.npz"), str(tmp_path / "props.tsv")
    rc.write_recs(ids, np.zeros_like(logp), 40, None, npz, logp=logp)
    rc.write_propensities(logp, ids, 40, tsv)
    a = ReplayLog.from_npz(npz, fixed=1, n_items=50)
    assert np.array_equal(a.ids, ids) and np.array_equal(a.logp0.view(np.uint32), logp.view(np.uint32)) and a.uids.tolist() == [40, 41, 42, 43]
    b = ReplayLog.from_tsv(tsv, 6, fixed=1)
    assert np.array_equal(b.ids, ids) and b.uids.tolist() == [40, 41, 42, 43]
    assert np.array_equal(b.logp0, np.array([[float("%.6g" % v) for v in row] for row in logp], np.float32))     # the file's %.6g
    # six significant digits: half a unit of the sixth is at most 5e-6 of the value, and the parsed value rounds to float32 once more
    assert (np.abs(b.logp0.astype(np.float64) - logp) <= (5e-6 + 2.0 ** -24) * np.abs(logp)).all()
    assert ReplayLog.from_tsv(tsv, 8).ids.shape == (4, 8) and (ReplayLog.from_tsv(tsv, 8).ids[:, 6:] == -1).all()
    with pytest.raises(ValueError, match="at most 5"):
        ReplayLog.from_tsv(tsv, 5)
    np.savez(str(tmp_path / "plain.npz"), uids=np.arange(4), ids=ids)
    with pytest.raises(ValueError, match="holds no `logp`"):
        ReplayLog.from_npz(str(tmp_path / "plain.npz"))
    # rewards: the held-out items, and a feedback file by uid
    import scipy.sparse as sp
    te = sp.csr_matrix((np.ones(3, np.float32), ([0, 0, 3], [int(ids[0, 2]), next(i for i in range(50) if i not in ids[0]), int(ids[3, 0])])), shape=(4, 50))
    want = np.zeros((4, 6), np.float32)
    want[0, 2] = want[3, 0] = 1
    assert np.array_equal(a.rewards_from(te), want) and a.reward is not None
    with pytest.raises(ValueError, match="held-out rows"):
        a.rewards_from(te[:3])
    fb = str(tmp_path / "clicks.tsv")
    open(fb, "w").write("40\t%d\n\n43\t%d,%d\n99\t1\n" % (ids[0, 2], ids[3, 0], 1000))
    assert np.array_equal(b.rewards_from_file(fb), want)
    plain = ReplayLog(ids, logp, fixed=1)
    with pytest.raises(ValueError, match="uid_start"):
        plain.rewards_from_file(fb)
    assert np.array_equal(plain.rewards_from_file(fb, uid_start=40), want)
    open(fb, "w").write("40\tx\n")
    with pytest.raises(ValueError, match="line 1"):
        b.rewards_from_file(fb)


def test_cli_arguments():
    from ltgan import replay as rp
    need = ["ds", "m.pt", "--log", "recs.npz", "--feedback", "heldout", "--temperature", "1,0.5,2"]
    a = rp.parse_args(need)
    assert a.temperatures == [1.0, 0.5, 2.0] and a.keep_prob == 1.0 and a.fixed is None and a.logged_fixed == 0 and a.clip == 100.0
    assert (a.group_kind, a.n_groups, a.split, a.k, a.json, a.propensities_out) == ("niche", 2, "test", None, None, None)
    a = rp.parse_args(need + ["--fixed", "5", "--logged-fixed", "5", "--clip", "10", "--groups", "pop:4", "--k", "20", "--json", "o.json"])
    assert (a.fixed, a.logged_fixed, a.clip, a.n_groups, a.k, a.json) == (5, 5, 10.0, 4, 20, "o.json")
    for drop in ("--log", "--feedback", "--temperature"):
        i = need.index(drop)
        with pytest.raises(SystemExit) as e:
            rp.parse_args(need[:i] + need[i + 2:])
        assert e.value.code == 2, drop
    for bad in (["--temperature", "0"], ["--temperature", "1,-1"], ["--temperature", "nan"], ["--temperature", "1,,2"], ["--temperature", "x"],
                ["--temperature", ",".join(["1"] * 9)], ["--temperature", "1e-60"], ["--fixed", "2", "--logged-fixed", "3"],
                ["--logged-fixed", "-1"], ["--clip", "0"], ["--clip", "inf"], ["--clip", "nan"], ["--groups", "pop:1"], ["--k", "0"],
                ["--k", "1025"], ["--keep-prob", "0"], ["--keep-prob", "1.5"], ["--split", "train"]):
        with pytest.raises(SystemExit) as e:
            rp.parse_args(need + bad)
        assert e.value.code == 2, bad
    assert "--keep-prob 1.0 on both sides is the safe choice" in " ".join(rp.__doc__.split())      # the module text says what must match
    ids = np.array([[5, 2, 9], [7, -1, -1]], np.int32)
    lp1 = np.array([[[0.0, -1.25, -np.inf], [-2.5e-7, 0.0, 0.0]], [[0.0, -0.5, -0.333333333], [-1.0, 0.0, 0.0]]], np.float32)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert rp.write_target_propensities(lp1, [0.5, 2.0], ids, 40, os.path.join(tmp, "t.tsv")) == 6
        assert open(os.path.join(tmp, "t.tsv")).read() == ("# T 0.5\n40\t5:0,2:-1.25,9:-inf\n41\t7:-2.5e-07\n"
                                                           "# T 2\n40\t5:0,2:-0.5,9:-0.333333\n41\t7:-1\n")
    est = {0.5: {"niche": dict(ips=0.25, stderr=0.01, snips=0.05, exposure=5.0, logged=0.2, logged_per_slot=0.04),
                 "all": dict(ips=0.5, stderr=0.02, snips=0.025, exposure=20.0, logged=0.4, logged_per_slot=0.02), "ess": 90.5, "supported": 1.0,
                 "n_users": 100}}
    assert rp.replay_lines(est, ["niche"]) == [
        "replay T 0.5 niche: ips 0.250000 +- 0.010000, per-slot 0.050000 (logged 0.040000), exposure 5.0000/user, ess 90.5 of 100, supported 1.0000",
        "replay T 0.5 all: ips 0.500000 +- 0.020000, per-slot 0.025000 (logged 0.020000), exposure 20.0000/user, ess 90.5 of 100, supported 1.0000"]


# ---------------------------------------------------------------------------------------------- the reference
def _enum_rows(T0, F0, T1, F1, clip=1e300):
    """every logged list of (T0, F0) replayed under (T1, F1) by the reference -> (pi0 [n], A [n, 3], B [n, 3], first_bad [n])"""
    Y, labels = R.enum_tables()
    lists, pi0, logp0 = R.enumerate_policy(T0, F0)
    fold = np.zeros(8, bool)
    fold[R.ENUM_FOLD] = True
    A, B, fb = [], [], []
    for ids, lp in zip(lists, logp0):
        y = Y[ids, np.arange(R.ENUM_K)]
        out = R.replay_full_row(E.PAIR_LOGITS, fold, ids, lp, y, F1, [E.inv_temp_of(T1)], labels, 2, clip)
        A.append(out["A"][0]), B.append(out["B"][0]), fb.append(out["first_bad"])
    return pi0, np.array(A), np.array(B), np.array(fb)


@pytest.mark.parametrize("pair", R.ENUM_PAIRS)
def test_reference_equals_the_targets_expectation_over_every_logged_list(pair):
    (T0, F0), (T1, F1) = pair
    pi0, A, B, fb = _enum_rows(T0, F0, T1, F1)
    assert len(pi0) == (210 if F0 == 0 else 30) and abs(pi0.sum() - 1.0) < 1e-12
    if (F0, F1) == (0, 1):
        assert int((fb == R.ENUM_K).sum()) == 30                        # with F' = 1, 30 of the 210 lists are supported
    Y, labels = R.enum_tables()
    wantA, wantB = R.target_value(T1, F1, Y, labels)
    gotA, gotB = (pi0[:, None] * A).sum(0), (pi0[:, None] * B).sum(0)
    print("(%g, %d) -> (%g, %d): largest difference %.3g" % (T0, F0, T1, F1, max(np.abs(gotA - wantA).max(), np.abs(gotB - wantB).max())))
    assert np.abs(gotA - wantA).max() <= 1e-12 and np.abs(gotB - wantB).max() <= 1e-12
    assert abs(gotB[2] - 3.0) <= 1e-12                                   # the exposures add up to k


def test_reference_same_policy_gives_weights_of_exactly_one():
    """the log's own logp0 replayed at the logging policy: d_j = 0.0 exactly, so w = 1.0, A = sum y and B = the real slots"""
    S, fold, G, kinds = E.build_rows(21, 67, kinds=("regular", "neginf", "short"), reps=2)
    labels = (np.arange(67) % 3).astype(np.uint8)
    rng = np.random.default_rng(2)
    for u in range(S.shape[0]):
        for k, F, T in ((5, 0, 1.0), (12, 3, 0.5), (20, 1, 2.0)):
            it = E.inv_temp_of(T)
            w = E.explore_row(S[u], fold[u], k, F, it, G[u])
            y = rng.random(k)
            # logp0 as the replay's own float64 of the same list, so that the comparison is of the definition and not of a rounding
            base = R.replay_full_row(S[u], fold[u], w["ids"], np.zeros(k), y, F, [it], labels, 3, 1e300)
            assert np.allclose(base["logp1"][0], w["logp"], rtol=0, atol=1e-12), (u, kinds[u])
            out = R.replay_full_row(S[u], fold[u], w["ids"], base["logp1"][0], y, F, [it], labels, 3, 100.0)
            real = w["ids"] >= 0
            assert out["first_bad"] == k and (out["w"][0][real] == 1.0).all() and (out["w"][0][~real] == 0.0).all(), (u, kinds[u])
            assert out["W"][0] == 1.0 and out["B"][0, 3] == real.sum() and abs(out["A"][0, 3] - y[real].sum()) < 1e-12


def test_reference_unsupported_entries_padding_and_clipping():
    s = np.array([0.0, 1.0, 2.0, -1.0, 0.5, 3.0, 0.2, -0.3], np.float32)
    fold = np.zeros(8, bool)
    fold[4] = True
    labels = np.array([0, 0, 1, 1, 0, 1, 0, 1], np.uint8)
    it = [np.float32(1.0), np.float32(2.0)]
    ids = np.array([5, 2, -1, 4, 1, -1], np.int32)                       # head 5 (the top-1), padding in the middle, fold-in item 4, padding last
    lp0 = np.array([0, -0.5, 0, -1.0, -0.7, 0])
    y = np.array([1.0, 2.0, 9.0, 4.0, 8.0, 9.0])
    out = R.replay_full_row(s, fold, ids, lp0, y, 1, it, labels, 2, 1e300)
    assert out["state"].tolist() == [0, 1, 0, 2, 1, 0] and out["first_bad"] == 3 and (out["W"] == 0).all() and out["M"] == np.float32(2.0)
    assert np.isneginf(out["logp1"][:, 3]).all() and (out["logp1"][:, [0, 2, 5]] == 0).all()
    # the unsupported entry takes no mass out: rest holds the eligible items 0, 3, 6, 7
    for p in range(2):
        rest = np.exp((s[[0, 3, 6, 7]].astype(np.float64) - 2.0) * float(it[p])).sum()
        assert abs(out["rest"][p] - rest) < 1e-12
        l1 = 0.0 - np.log(rest + 1.0 + np.exp((1.0 - 2.0) * float(it[p])))                      # slot 1 = item 2, x = 0
        assert abs(out["logp1"][p, 1] - l1) < 1e-12
        w1 = np.exp(l1 + 0.5)
        assert np.allclose(out["w"][p], [1.0, w1, 0, 0, 0, 0], atol=1e-12) and np.allclose(out["A"][p], [0.0, 1.0 + 2.0 * w1, 1.0 + 2.0 * w1])
        assert np.allclose(out["B"][p], [0.0, 1.0 + w1, 1.0 + w1])
    # a wrong head entry: nothing is supported from slot 0 on
    bad = R.replay_full_row(s, fold, np.array([2, 5, 1], np.int32), np.array([0, -0.1, -0.2]), np.ones(3), 1, it, labels, 2, 1e300)
    assert bad["first_bad"] == 0 and (bad["w"] == 0).all() and (bad["A"] == 0).all() and bad["state"].tolist() == [0, 2, 1]
    # clipping caps the prefix weight, not the increments; an all-padding row has the empty product
    ids = np.array([5, 2, 1], np.int32)
    lp0 = np.array([0.0, -6.0, -0.1])
    free = R.replay_full_row(s, fold, ids, lp0, np.ones(3), 1, it[:1], labels, 2, 1e300)
    assert free["w"][0][1] > 20
    for clip in (free["w"][0][1] * 0.5, free["w"][0][1], free["w"][0][1] * 2):
        got = R.replay_full_row(s, fold, ids, lp0, np.ones(3), 1, it[:1], labels, 2, clip)
        assert np.allclose(got["w"][0], np.minimum(free["w"][0], clip), rtol=1e-12)
    empty = R.replay_full_row(s, fold, np.full(3, -1, np.int32), np.zeros(3), np.ones(3), 1, it, labels, 2, 0.5)
    assert empty["first_bad"] == 3 and (empty["W"] == 0.5).all() and (empty["B"] == 0).all()


def test_estimates_from_a_per_row_table():
    from ltgan.serving import ReplayLog, replay_estimates
    ids = np.array([[0, 1, 2], [3, 4, -1], [5, 0, 1], [2, 3, 4]], np.int32)
    y = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 0]], np.float32)
    log = ReplayLog(ids, np.zeros((4, 3), np.float32), y)
    labels = np.array([0, 0, 0, 1, 1, 1], np.uint8)
    rows = np.zeros((4, 1, 3, 2))
    rows[:, 0, 0] = [[1, 3], [0, 0], [0, 2], [1, 1]]
    rows[:, 0, 1] = [[0, 0], [1, 2], [0, 1], [1, 2]]
    rows[:, 0, 2] = rows[:, 0, 0] + rows[:, 0, 1]
    w = np.array([[1.0], [1.0], [1.0], [1.0]])
    fb = np.array([[3], [3], [3], [3]], np.int32)
    est = replay_estimates(rows, w, fb, log, [1.0], labels, 2, ["head", "tail"])[1.0]
    assert est["ess"] == 4.0 and est["supported"] == 1.0 and est["n_users"] == 4
    assert est["all"]["ips"] == 1.0 == est["all"]["logged"] and est["all"]["exposure"] == 11 / 4 and est["all"]["snips"] == 4 / 11
    assert est["all"]["logged_per_slot"] == 4 / 11 and est["head"]["logged"] == 2 / 4 and est["tail"]["logged_per_slot"] == 2 / 5
    A = np.array([1.0, 1.0, 0.0, 2.0])
    assert abs(est["all"]["stderr"] - A.std(ddof=1) / 2.0) < 1e-15
    w2 = np.array([[2.0], [0.0], [1.0], [1.0]])
    fb2 = np.array([[3], [1], [3], [3]], np.int32)
    est2 = replay_estimates(rows, w2, fb2, log, [1.0], labels, 2)[1.0]
    assert est2["ess"] == 16.0 / 6.0 and est2["supported"] == 0.75 and "0" in est2 and "1" in est2
