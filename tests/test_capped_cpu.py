"""CPU-side checks of the exposure-capped lists: the ltg_cap_* entry points are exported and bound with the header's argument types, every
documented refusal returns LTG_EINVAL without a GPU, ExposureCap and the Recommender validate, both CLIs handle --cap, the extra summary
line, and the numpy reference the GPU tests lean on (tests/capped_ref.py): its synchronous rounds equal one-proposal-at-a-time deferred
acceptance in other user orders, and its tables have the consequences DESIGN 5.16 lists."""
import ctypes as C
import os

import numpy as np
import pytest

import capped_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    want = {"ltg_cap_ws_bytes": (sz, [i32, i32, i32]),
            "ltg_cap_index": (C.c_int, [i32, i32, vp, i32, vp, vp, sz, vp]),
            "ltg_cap_rounds": (C.c_int, [i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]),
            "ltg_cap_finish": (C.c_int, [i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp])}
    for name, (res, args) in want.items():
        assert cabi.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name
    assert (cabi.LTG_CAP_STATE, cabi.LTG_CAP_MAX_ROUNDS) == (8, 64)
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_CAP_STATE 8" in header and "#define LTG_CAP_MAX_ROUNDS 64" in header and "#define LTG_ABI_VERSION 14" in header
    assert "size_t ltg_cap_ws_bytes(int32_t n_rows, int32_t c_in, int32_t n_items_global);" in header
    assert "int ltg_cap_index(int32_t n_rows, int32_t c_in, const int32_t* cand_id, int32_t n_items_global, int32_t* state" in header
    assert "int ltg_cap_rounds(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse" in header
    assert "int ltg_cap_finish(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, int32_t n_items_global, int32_t k," in header
    kernel = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_cap.h")).read()
    assert "constexpr int CP_STATE = 8;" in kernel
    hip = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_kernels.hip")).read()
    assert hip.index('#include "ltg_audience.h"') < hip.index('#include "ltg_cap.h"')
    assert "ltg_cap.h" in open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "Makefile")).read()


def test_ws_bytes_helper():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    assert lib.ltg_cap_ws_bytes(10, 8, 100) >= 100 * 8 + 101 * 4 + 100 * 4 + 80 * 4 + 80 + 10 * 4
    assert lib.ltg_cap_ws_bytes(0, 1, 1) > 0
    assert lib.ltg_cap_ws_bytes(3000, 256, 1000) < lib.ltg_cap_ws_bytes(3001, 256, 1000) <= lib.ltg_cap_ws_bytes(3001, 256, 360448)
    for bad in ((-1, 8, 100), (10, 0, 100), (10, 1025, 100), (10, 8, 0), (10, 8, -3), (2 ** 21, 1024, 100), (2 ** 30, 2, 100)):
        assert lib.ltg_cap_ws_bytes(*bad) == 0, bad
    assert lib.ltg_cap_ws_bytes(2 ** 21 - 1, 1024, 100) > 0 and lib.ltg_cap_ws_bytes(2 ** 31 - 1, 1, 100) > 0


def test_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    fb, ib, st, ws = (C.c_float * 64)(), (C.c_int32 * 64)(), (C.c_int32 * 8)(), (C.c_uint8 * 8)()
    big = 1 << 40                                        # (never dereferenced: every call below is refused or has no rows)

    def index(n=2, c=8, ci=ib, I=16, state=st, w=ws, wb=big):
        return lib.ltg_cap_index(n, c, ci, I, state, w, wb, None)

    def rounds(n=2, c=8, cs=fb, ci=ib, lse=fb, cap=ib, I=16, k=4, r=1, state=st, w=ws, wb=big):
        return lib.ltg_cap_rounds(n, c, cs, ci, lse, cap, I, k, r, state, w, wb, None)

    def finish(n=2, c=8, cs=fb, ci=ib, I=16, k=4, so=fb, io=ib, state=st, w=ws, wb=big):
        return lib.ltg_cap_finish(n, c, cs, ci, I, k, so, io, state, w, wb, None)

    for call, names in ((index, ("ci", "state", "w")), (rounds, ("cs", "ci", "cap", "state", "w")), (finish, ("cs", "ci", "so", "io", "state", "w"))):
        assert call(n=0) == 0                            # zero rows: nothing to launch
        for name in names:
            assert call(**{name: None}) == -1, (call.__name__, name)
            assert call(n=0, **{name: None}) == -1, (call.__name__, name)     # ... but the arguments are still checked
        for kw in (dict(n=-1), dict(n=2 ** 28, c=8), dict(n=2 ** 21, c=1024), dict(wb=lib.ltg_cap_ws_bytes(2, 8, 16) - 1)):
            assert call(**kw) == -1, (call.__name__, kw)
        for kw in (dict(c=0), dict(c=-1), dict(c=1025), dict(I=0), dict(I=-7), dict(wb=0), dict(wb=lib.ltg_cap_ws_bytes(0, 8, 16) - 1)):
            assert call(**kw) == -1 and call(n=0, **kw) == -1, (call.__name__, kw)
        assert call(n=0, c=1024, wb=lib.ltg_cap_ws_bytes(0, 1024, 16)) == 0
    assert rounds(n=0, lse=None) == 0                    # lse is optional
    for call in (rounds, finish):
        for k in (0, -1, 9, 2 ** 31 - 1):
            assert call(k=k) == -1 and call(n=0, k=k) == -1, (call.__name__, k)
        assert call(n=0, k=8) == 0 and call(n=0, k=1) == 0
    for r in (0, -1, 65):
        assert rounds(r=r) == -1 and rounds(n=0, r=r) == -1, r
    assert rounds(n=0, r=64) == 0


class _FakeEngine:
    I, I_global, device, item_lo = 50, 50, "cpu", 0

    def cap_ws_bytes(self, n, c, n_items=None):
        return 64


def test_exposure_cap_validation():
    from ltgan.sharded import ExposureCap as ShardedExposureCap
    from ltgan.trainer import Calibrate, Diversify, ExposureCap, Recommender
    assert ShardedExposureCap is ExposureCap
    labels = np.array([0, 1, 7] * 16 + [0, 0], np.uint8)
    for bad in (-1, 2.5, np.full(50, -1)):
        with pytest.raises(ValueError):
            ExposureCap(bad)
    for kw in (dict(score="prob"), dict(candidates=0), dict(candidates=1025), dict(batch=0), dict(batch=65)):
        with pytest.raises(ValueError):
            ExposureCap(5, **kw)
    for bad in ((labels, 0, {0: 1}), (labels, 9, {0: 1}), (labels, 2, {2: 1}), (labels, 2, {-1: 1}), (labels, 2, {0: -1})):
        with pytest.raises(ValueError):
            ExposureCap(bad)
    with pytest.raises(ValueError):
        ExposureCap(np.ones(49, np.int32)).bind(_FakeEngine(), 10, 10, 33)      # a cap count that differs from the catalogue
    with pytest.raises(ValueError):
        ExposureCap((labels[:49], 2, {0: 3})).bind(_FakeEngine(), 10, 10, 33)
    with pytest.raises(ValueError):
        ExposureCap(5, candidates=9).bind(_FakeEngine(), 10, 10, 33)           # fewer candidates than list entries
    with pytest.raises(ValueError):
        ExposureCap(5).bind(_FakeEngine(), 10, 300, 2 ** 21)                    # 2^21 users x 1024 candidates: 2^31 entries
    c = ExposureCap(5)
    c.bind(_FakeEngine(), 10, 10, 33)
    assert c.c == 40 and c.needs_lse and tuple(c.cand_i.shape) == (33, 40) and tuple(c.lse.shape) == (33,) and (c.cap_vector() == 5).all()
    c = ExposureCap(0, score="logit")
    c.bind(_FakeEngine(), 10, 300, 7)
    assert c.c == 1024 and not c.needs_lse and c.lse is None and (c.cap_vector() == 0).all()
    c = ExposureCap((labels, 2, {1: 3}), candidates=12)
    c.bind(_FakeEngine(), 10, 10, 33)
    v = c.cap_vector()
    assert c.c == 12 and (v[labels == 1] == 3).all() and (v[labels != 1] == ExposureCap.UNCAPPED).all()
    c = ExposureCap(np.arange(50))
    c.bind(_FakeEngine(), 10, 1, 2)
    assert c.c == 4 and c.cap_vector().tolist() == list(range(50)) and c.cap_vector().dtype == np.int32
    good = ExposureCap(5)
    for kw in (dict(rule=object()), dict(diversify=Diversify(0.5)), dict(calibrate=Calibrate(labels, 2, 0.5))):
        with pytest.raises(ValueError):                  # refused before anything of the engine is touched
            Recommender(_FakeEngine(), None, k=10, cap=good, **kw)
    with pytest.raises(ValueError):
        Recommender(_FakeEngine(), None, k=0, cap=good)


def test_cli_arguments():
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    for mod in (rc, lt):
        a = mod.parse_args(["ds", "model.pt"])                           # nothing changes without the option
        assert a.cap is None and a.caps is None and a.cap_candidates is None and a.cap_score is None
        a = mod.parse_args(["ds", "m.pt", "--cap", "25"])
        assert a.caps == 25 and a.cap_candidates is None and a.cap_score is None
        assert mod.parse_args(["ds", "m.pt", "--cap", "0"]).caps == 0
        a = mod.parse_args(["ds", "m.pt", "--cap", "popular:40", "--cap-candidates", "500", "--cap-score", "logit"])
        assert a.caps == {0: 40} and a.cap_candidates == 500 and a.cap_score == "logit"
        a = mod.parse_args(["ds", "m.pt", "--cap", "pop0:9,pop3:0", "--groups", "pop:4"])
        assert a.caps == {0: 9, 3: 0}
        for bad in (["--cap", "-1"], ["--cap", "x"], ["--cap"], ["--cap", "niche"], ["--cap", "niche:-2"], ["--cap", "niche:x"],
                    ["--cap", "rare:3"], ["--cap", "niche:3,niche:4"], ["--cap", "pop0:3"], ["--cap-candidates", "300"],
                    ["--cap-score", "logit"], ["--cap", "5", "--cap-score", "prob"], ["--cap", "5", "--cap-candidates", "1025"],
                    ["--cap", "5", "--cap-candidates", "99"], ["--cap", "5", "--min-slots", "niche:5"], ["--cap", "5", "--diversify", "0.5"],
                    ["--cap", "5", "--calibrate", "0.5"]):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(["ds", "m.pt"] + bad)
            assert e.value.code == 2, (mod.__name__, bad)
    assert rc.parse_args(["ds", "m.pt", "--cap", "5", "--k", "10", "--cap-candidates", "10"]).cap_candidates == 10
    assert rc.parse_args(["ds", "m.pt", "--cap", "5", "--explain", "3"]).explain == 3      # the explanations read the capped lists
    assert lt.parse_cap("7", ["a", "b"]) == 7 and lt.parse_cap("b:2, a:0", ["a", "b"]) == {1: 2, 0: 0}


def test_cap_line_from_a_hand_made_table():
    from ltgan import longtail as lt
    plain = np.array([[0, 1], [0, 1], [0, 2], [0, -1]], np.int32)
    capped = np.array([[0, 1], [0, 1], [2, 3], [-1, -1]], np.int32)
    line = lt.cap_line(plain, capped, np.array([2, 3, 1, 0, 5], np.int32), dict(short=1, rounds=3), 2)
    assert line == "cap@2: max exposure 4 -> 2, 2 items at their cap, 1 short lists, 3 rounds"


# ---------------------------------------------------------------------------------------------- the reference
# (n, I, c, k, cap, quant, padded rows)
CASES = [(64, 24, 24, 5, 14, None, 0), (300, 48, 24, 6, 40, None, 0), (40, 500, 320, 100, 8, None, 0), (200, 300, 100, 1, 1, None, 0),
         (130, 70, 65, 64, 125, None, 0), (211, 129, 129, 10, 17, 0.5, 0), (90, 60, 33, 7, 6, None, 25), (150, 40, 40, 40, 30, 1.0, 10),
         (1, 10, 10, 3, 1, None, 0), (50, 30, 8, 8, 2, None, 0), (120, 200, 70, 20, 9, 0.25, 30), (500, 100, 64, 12, 50, None, 0)]


@pytest.fixture(scope="module")
def cases():
    out = []
    for n, I, c, k, cap, quant, pad in CASES:
        s, i, lse = R.zipf_case(1000 + n + I, n, I, c, quant=quant, pad_rows=pad)
        out.append((s, i, lse, np.full(I, cap, np.int32), k))
    return out


def per_item_caps(seed, I, lo, hi, n):
    """mixed caps: a third of the items at 0, a third uncapped, the rest in [lo, hi]"""
    rng = np.random.default_rng(seed)
    cap = rng.integers(lo, hi + 1, I).astype(np.int32)
    kind = rng.integers(0, 3, I)
    cap[kind == 0] = 0
    cap[kind == 1] = n
    return cap


def test_the_two_schedules_agree(cases):
    rounds = []
    for t, (s, i, lse, cap, k) in enumerate(cases):
        for L in (lse, None):
            act, thr, r = R.capped_rounds(s, i, L, cap, k, max_rounds=s.size + 1)
            rounds.append(r)
            assert np.array_equal(R.capped_sequential(s, i, L, cap, k), act), t                    # last row first, depth first
            rng = np.random.default_rng(t)
            assert np.array_equal(R.capped_sequential(s, i, L, cap, k, rng.permutation(len(s))), act), t
            # the thresholds are consistent with the active set: every active word is at or above its item's, and a raised threshold
            # is the lowest word its item holds
            W, (ok, _) = R.words(s, L), R.entry_mask(i, cap)
            assert (W[act] >= thr[i[act]]).all() and (act <= ok).all()
            low = np.full(len(cap), np.iinfo(np.uint64).max, np.uint64)
            np.minimum.at(low, i[act], W[act])
            assert (low[thr > 0] == thr[thr > 0]).all(), t
    assert min(rounds) == 1 or min(rounds) >= 2
    assert max(rounds) >= 8, rounds                      # the k = 1 case chains displacements over many rounds


def test_no_blocking_pair_and_exposure_within_the_cap(cases):
    for t, (s, i, lse, cap, k) in enumerate(cases):
        for L in (lse, None):
            sc, ids, st = R.capped_lists(s, i, L, cap, k)
            assert R.blocking_pairs(s, i, L, cap, k, ids) == 0, t
            assert (R.exposure(ids, len(cap)) <= cap).all(), t
            for u in range(len(ids)):                    # distinct ids in candidate order, each with its original score
                got = ids[u][ids[u] >= 0]
                pos = [int(np.nonzero(i[u] == g)[0][0]) for g in got]
                assert pos == sorted(set(pos)) and np.array_equal(sc[u, :len(pos)].view(np.uint32), s[u, pos].view(np.uint32)), (t, u)
                assert (ids[u, len(pos):] == -1).all() and np.isneginf(sc[u, len(pos):]).all()
            assert st["short"] == int((ids[:, -1] < 0).sum())
    # the checker does find blocking pairs in a table that has them: the plain table under a binding cap is over capacity, not blocked;
    # the capped table with one user's best listed entry swapped for a worse candidate is blocked
    s, i, lse, cap, k = cases[0]
    _, ids, _ = R.capped_lists(s, i, lse, cap, k)
    bad = ids.copy()
    u = 3
    unlisted = [g for g in i[u] if g not in ids[u]]
    bad[u, 0] = unlisted[-1]                             # u's worst candidate instead of u's best entry
    assert R.blocking_pairs(s, i, lse, cap, k, bad) >= 1


def test_caps_of_at_least_n_give_the_first_k_columns(cases):
    for s, i, lse, cap, k in cases:
        n = len(s)
        for big in (n, n + 1, 2 ** 31 - 1):
            sc, ids, st = R.capped_lists(s, i, lse, np.full(len(cap), big, np.int64), k)
            assert np.array_equal(ids, i[:, :k]) and np.array_equal(sc.view(np.uint32), s[:, :k].view(np.uint32))
            assert st["rounds"] == 1 and st["over"] == 0


def test_cap_zero_removes_an_item_and_mixed_caps_hold(cases):
    for t, (s, i, lse, cap, k) in enumerate(cases):
        n, I = len(s), len(cap)
        head = int(np.argmax(R.exposure(i[:, :k], I)))
        only = np.full(I, n, np.int32)
        only[head] = 0
        _, ids, _ = R.capped_lists(s, i, lse, only, k)
        assert not (ids == head).any()
        for u in range(n):                               # every other entry stays, in order: the plain list without the head
            want = [g for g in i[u] if g >= 0 and g != head][:k]
            assert ids[u][ids[u] >= 0].tolist() == want, (t, u)
        mixed = per_item_caps(t, I, 1, max(1, n // 8), n)
        _, ids, _ = R.capped_lists(s, i, lse, mixed, k)
        hits = R.exposure(ids, I)
        assert (hits <= mixed).all() and (hits[mixed == 0] == 0).all() and R.blocking_pairs(s, i, lse, mixed, k, ids) == 0, t
        act = R.capped_rounds(s, i, lse, mixed, k)[0]
        assert np.array_equal(R.capped_sequential(s, i, lse, mixed, k), act), t


def test_equal_scores_go_to_the_lower_row_and_zero_has_one_sign():
    """one item, every user scores it 0.0 with either sign: the cap keeps the lowest rows; with quantised scores an item's holders are
    the best scores and, on the boundary score, the lowest rows"""
    n, cap = 12, 5
    s = np.zeros((n, 2), np.float32)
    s[::2, 0] = -0.0
    s[:, 1] = -1.0
    i = np.tile(np.array([[0, 1]], np.int32), (n, 1))
    sc, ids, _ = R.capped_lists(s, i, None, np.array([cap, n], np.int32), 1)
    assert ids[:, 0].tolist() == [0] * cap + [1] * (n - cap)
    assert np.array_equal(sc[:cap, 0].view(np.uint32), s[:cap, 0].view(np.uint32))      # the zeros keep their signs
    assert R.words(s[:, :1])[:, 0].tolist() == sorted(R.words(s[:, :1])[:, 0].tolist(), reverse=True)
    s, i, lse = R.zipf_case(5, 211, 129, 129, quant=0.5)
    capv = np.full(129, 17, np.int32)
    for L in (None, lse):
        _, ids, _ = R.capped_lists(s, i, L, capv, 10)
        sub = s if L is None else (s - L[:, None]).astype(np.float32)
        tied = 0
        for item in np.nonzero(R.exposure(ids, 129) == 17)[0]:
            holders = np.nonzero((ids == item).any(1))[0]
            wanted = np.array([u for u in range(211) if item in i[u] and u not in holders])
            sc_h = np.array([sub[u, np.nonzero(i[u] == item)[0][0]] for u in holders])
            edge = sc_h.min()
            # a user left out with the boundary score would be a blocking pair unless their row is higher than every holder's at that score
            for u in wanted:
                su = sub[u, np.nonzero(i[u] == item)[0][0]]
                pos_u = int(np.nonzero(i[u] == item)[0][0])
                listed_pos = [int(np.nonzero(i[u] == g)[0][0]) for g in ids[u][ids[u] >= 0]]
                if len(listed_pos) == 10 and pos_u > max(listed_pos):
                    continue                             # u never wanted it
                assert su <= edge
                if su == edge:
                    tied += 1
                    assert u > holders[sc_h == edge].max()
        assert tied > 0                                  # the row did decide
