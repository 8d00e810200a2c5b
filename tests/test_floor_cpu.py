"""CPU-side checks of the exposure-floor lists: the ltg_floor_* entry points are exported and bound with the header's argument types,
every documented refusal returns LTG_EINVAL without a GPU, ExposureFloor and the Recommender validate, both CLIs handle --floor, the extra
summary line, and the numpy reference the GPU tests lean on (tests/floor_ref.py): its synchronous rounds equal one-proposal-at-a-time
item-proposing deferred acceptance in three item orders on 200 tiny random cases, and its tables have the consequences DESIGN 5.18 lists."""
import ctypes as C
import os

import numpy as np
import pytest

import floor_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    want = {"ltg_floor_ws_bytes": (sz, [i32, i32, i32]),
            "ltg_floor_index": (C.c_int, [i32, i32, vp, i32, vp, vp, sz, vp]),
            "ltg_floor_rounds": (C.c_int, [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]),
            "ltg_floor_finish": (C.c_int, [i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp])}
    for name, (res, args) in want.items():
        assert cabi.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name
    assert (cabi.LTG_FLOOR_STATE, cabi.LTG_FLOOR_MAX_ROUNDS) == (8, 64)
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_FLOOR_STATE 8" in header and "#define LTG_FLOOR_MAX_ROUNDS 64" in header and "#define LTG_ABI_VERSION 14" in header
    assert "size_t ltg_floor_ws_bytes(int32_t n_rows, int32_t c_in, int32_t n_items_global);" in header
    assert "int ltg_floor_index(int32_t n_rows, int32_t c_in, const int32_t* cand_id, int32_t n_items_global, int32_t* state" in header
    assert "int ltg_floor_rounds(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse" in header
    assert "int ltg_floor_finish(int32_t n_rows, int32_t c_in, const float* cand_score, const int32_t* cand_id, const float* lse" in header
    kernel = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_floor.h")).read()
    assert "constexpr int FL_STATE = 8;" in kernel
    hip = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_kernels.hip")).read()
    assert hip.index('#include "ltg_cap.h"') < hip.index('#include "ltg_floor.h"')
    assert "ltg_floor.h" in open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "Makefile")).read()


def test_ws_bytes_helper():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    # the selection words, the offsets, the cursors, the entry numbers, the limits, one int32 per row, the held counts
    assert lib.ltg_floor_ws_bytes(10, 8, 100) >= 100 * 8 + 101 * 4 + 100 * 4 + 80 * 4 + 10 * 4 + 10 * 4 + 100 * 4
    assert lib.ltg_floor_ws_bytes(0, 1, 1) > 0
    assert lib.ltg_floor_ws_bytes(3000, 256, 1000) < lib.ltg_floor_ws_bytes(3001, 256, 1000) <= lib.ltg_floor_ws_bytes(3001, 256, 360448)
    for bad in ((-1, 8, 100), (10, 0, 100), (10, 1025, 100), (10, 8, 0), (10, 8, -3), (2 ** 21, 1024, 100), (2 ** 30, 2, 100)):
        assert lib.ltg_floor_ws_bytes(*bad) == 0, bad
    assert lib.ltg_floor_ws_bytes(2 ** 21 - 1, 1024, 100) > 0 and lib.ltg_floor_ws_bytes(2 ** 31 - 1, 1, 100) > 0


def test_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    fb, ib, st, ws, ab = (C.c_float * 64)(), (C.c_int32 * 64)(), (C.c_int32 * 8)(), (C.c_uint8 * 8)(), (C.c_uint8 * 64)()
    big = 1 << 40                                        # (never dereferenced: every call below is refused or has no rows)

    def index(n=2, c=8, ci=ib, I=16, state=st, w=ws, wb=big):
        return lib.ltg_floor_index(n, c, ci, I, state, w, wb, None)

    def rounds(n=2, c=8, cs=fb, ci=ib, lse=fb, need=ib, I=16, k=4, R=2, r=1, state=st, w=ws, wb=big):
        return lib.ltg_floor_rounds(n, c, cs, ci, lse, need, I, k, R, r, state, w, wb, None)

    def finish(n=2, c=8, cs=fb, ci=ib, lse=fb, need=ib, I=16, k=4, R=2, so=fb, io=ib, ao=ab, ho=ib, state=st, w=ws, wb=big):
        return lib.ltg_floor_finish(n, c, cs, ci, lse, need, I, k, R, so, io, ao, ho, state, w, wb, None)

    for call, names in ((index, ("ci", "state", "w")), (rounds, ("cs", "ci", "need", "state", "w")),
                        (finish, ("cs", "ci", "need", "so", "io", "state", "w"))):
        assert call(n=0) == 0                            # zero rows: nothing to launch
        for name in names:
            assert call(**{name: None}) == -1, (call.__name__, name)
            assert call(n=0, **{name: None}) == -1, (call.__name__, name)     # ... but the arguments are still checked
        for kw in (dict(n=-1), dict(n=2 ** 28, c=8), dict(n=2 ** 21, c=1024), dict(wb=lib.ltg_floor_ws_bytes(2, 8, 16) - 1)):
            assert call(**kw) == -1, (call.__name__, kw)
        for kw in (dict(c=0), dict(c=-1), dict(c=1025), dict(I=0), dict(I=-7), dict(wb=0), dict(wb=lib.ltg_floor_ws_bytes(0, 8, 16) - 1)):
            assert call(**kw) == -1 and call(n=0, **kw) == -1, (call.__name__, kw)
        assert call(n=0, c=1024, wb=lib.ltg_floor_ws_bytes(0, 1024, 16)) == 0
    assert rounds(n=0, lse=None) == 0 and finish(n=0, lse=None, ao=None, ho=None) == 0      # lse and the two tables are optional
    for call in (rounds, finish):
        for k in (0, -1, 9, 2 ** 31 - 1):
            assert call(k=k) == -1 and call(n=0, k=k) == -1, (call.__name__, k)
        assert call(n=0, k=8) == 0 and call(n=0, k=2) == 0
        for R in (-1, 5, 2 ** 31 - 1):                   # the reserve lies in [0, k]
            assert call(R=R) == -1 and call(n=0, R=R) == -1, (call.__name__, R)
        assert call(n=0, R=0) == 0 and call(n=0, R=4) == 0 and call(n=0, k=1, R=1) == 0 and call(n=0, k=1, R=2) == -1
    for r in (0, -1, 65):
        assert rounds(r=r) == -1 and rounds(n=0, r=r) == -1, r
    assert rounds(n=0, r=64) == 0


class _FakeEngine:
    I, I_global, device, item_lo = 50, 50, "cpu", 0

    def floor_ws_bytes(self, n, c, n_items=None):
        return 64


def test_exposure_floor_validation():
    from ltgan.sharded import ExposureFloor as ShardedExposureFloor
    from ltgan.trainer import Calibrate, Diversify, ExposureCap, ExposureFloor, Recommender, ShareTarget
    assert ShardedExposureFloor is ExposureFloor
    labels = np.array([0, 1, 7] * 16 + [0, 0], np.uint8)
    for bad in (-1, 2.5, np.full(50, -1)):
        with pytest.raises(ValueError):
            ExposureFloor(bad, 2)
    for kw in (dict(score="prob"), dict(candidates=0), dict(candidates=1025), dict(batch=0), dict(batch=65)):
        with pytest.raises(ValueError):
            ExposureFloor(5, 2, **kw)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            ExposureFloor(5, bad)
    for bad in ((labels, 0, {0: 1}), (labels, 9, {0: 1}), (labels, 2, {2: 1}), (labels, 2, {-1: 1}), (labels, 2, {0: -1})):
        with pytest.raises(ValueError):
            ExposureFloor(bad, 2)
    with pytest.raises(ValueError):
        ExposureFloor(np.ones(49, np.int32), 2).bind(_FakeEngine(), 10, 10, 33)   # a floor count that differs from the catalogue
    with pytest.raises(ValueError):
        ExposureFloor((labels[:49], 2, {0: 3}), 2).bind(_FakeEngine(), 10, 10, 33)
    with pytest.raises(ValueError):
        ExposureFloor(5, 2, candidates=9).bind(_FakeEngine(), 10, 10, 33)        # fewer candidates than list entries
    with pytest.raises(ValueError):
        ExposureFloor(5, 11).bind(_FakeEngine(), 10, 10, 33)                     # a reserve beyond the list
    with pytest.raises(ValueError):
        ExposureFloor(5, 2).bind(_FakeEngine(), 10, 300, 2 ** 21)                # 2^21 users x 1024 candidates: 2^31 entries
    f = ExposureFloor(5, 10)
    f.bind(_FakeEngine(), 10, 10, 33)
    assert f.c == 40 and f.needs_lse and tuple(f.cand_i.shape) == (33, 40) and tuple(f.lse.shape) == (33,) and (f.need_vector() == 5).all()
    assert f.reserve == 10 and tuple(f.held_d.shape) == (50,)
    f = ExposureFloor(0, 0, score="logit")
    f.bind(_FakeEngine(), 10, 300, 7)
    assert f.c == 1024 and not f.needs_lse and f.lse is None and (f.need_vector() == 0).all()
    f = ExposureFloor((labels, 2, {1: 3}), 2, candidates=12)
    f.bind(_FakeEngine(), 10, 10, 33)
    v = f.need_vector()
    assert f.c == 12 and (v[labels == 1] == 3).all() and (v[labels != 1] == 0).all()
    f = ExposureFloor(np.arange(50), 1)
    f.bind(_FakeEngine(), 10, 1, 2)
    assert f.c == 4 and f.need_vector().tolist() == list(range(50)) and f.need_vector().dtype == np.int32
    f = ExposureFloor(3, 1)
    f.bind(_FakeEngine(), 10, 4, 0)                      # no users: no launch, empty statistics
    f.match(None, 4, None, None)
    assert f.stats() == dict(rounds=0, lowerings=0, floor_items=50, short_items=0, rows_changed=0, inserted=0) and not f.held().any()
    good = ExposureFloor(5, 2)
    for kw in (dict(rule=object()), dict(diversify=Diversify(0.5)), dict(calibrate=Calibrate(labels, 2, 0.5)), dict(cap=ExposureCap(4)),
               dict(share=ShareTarget(labels, 2, [0], 0.5))):
        with pytest.raises(ValueError):                  # refused before anything of the engine is touched
            Recommender(_FakeEngine(), None, k=10, floor=good, **kw)
    with pytest.raises(ValueError):
        Recommender(_FakeEngine(), None, k=0, floor=good)


def test_cli_arguments():
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    for mod in (rc, lt):
        a = mod.parse_args(["ds", "model.pt"])                           # nothing changes without the option
        assert a.floor is None and a.floors is None and a.floor_reserve is None and a.floor_candidates is None and a.floor_score is None
        a = mod.parse_args(["ds", "m.pt", "--floor", "25", "--floor-reserve", "10"])
        assert a.floors == 25 and a.floor_reserve == 10 and a.floor_candidates is None and a.floor_score is None
        assert mod.parse_args(["ds", "m.pt", "--floor", "0", "--floor-reserve", "0"]).floors == 0
        assert mod.parse_args(["ds", "m.pt", "--floor", "3", "--floor-reserve", "100"]).floor_reserve == 100
        a = mod.parse_args(["ds", "m.pt", "--floor", "niche:4", "--floor-reserve", "5", "--floor-candidates", "500", "--floor-score", "logit"])
        assert a.floors == {1: 4} and a.floor_candidates == 500 and a.floor_score == "logit"
        a = mod.parse_args(["ds", "m.pt", "--floor", "pop0:9,pop3:0", "--floor-reserve", "1", "--groups", "pop:4"])
        assert a.floors == {0: 9, 3: 0}
        res = ["--floor-reserve", "5"]
        for bad in (["--floor", "5"], ["--floor", "-1"] + res, ["--floor", "x"] + res, ["--floor"] + res, ["--floor", "niche"] + res,
                    ["--floor", "niche:-2"] + res, ["--floor", "niche:x"] + res, ["--floor", "rare:3"] + res,
                    ["--floor", "niche:3,niche:4"] + res, ["--floor", "pop0:3"] + res, res, ["--floor-candidates", "300"],
                    ["--floor-score", "logit"], ["--floor", "5", "--floor-reserve", "-1"], ["--floor", "5", "--floor-reserve", "101"],
                    ["--floor", "5", "--floor-reserve", "x"], ["--floor", "5", "--floor-score", "prob"] + res,
                    ["--floor", "5", "--floor-candidates", "1025"] + res, ["--floor", "5", "--floor-candidates", "99"] + res,
                    ["--floor", "5", "--min-slots", "niche:5"] + res, ["--floor", "5", "--diversify", "0.5"] + res,
                    ["--floor", "5", "--calibrate", "0.5"] + res, ["--floor", "5", "--cap", "9"] + res,
                    ["--floor", "5", "--share", "niche:0.3"] + res):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(["ds", "m.pt"] + bad)
            assert e.value.code == 2, (mod.__name__, bad)
    a = rc.parse_args(["ds", "m.pt", "--floor", "5", "--floor-reserve", "10", "--k", "10", "--floor-candidates", "10"])
    assert a.floor_candidates == 10
    with pytest.raises(SystemExit):
        rc.parse_args(["ds", "m.pt", "--floor", "5", "--floor-reserve", "11", "--k", "10"])
    assert rc.parse_args(["ds", "m.pt", "--floor", "5", "--floor-reserve", "2", "--explain", "3"]).explain == 3   # they read the final lists
    assert lt.parse_floor("7", ["a", "b"]) == 7 and lt.parse_floor("b:2, a:0", ["a", "b"]) == {1: 2, 0: 0}


def test_floor_line_from_a_hand_made_table():
    from ltgan import longtail as lt
    plain = np.array([[0, 1], [0, 1], [0, 2], [0, -1]], np.int32)
    served = np.array([[0, 3], [0, 1], [0, 2], [0, -1]], np.int32)
    stats = dict(floor_items=3, short_items=1, inserted=1, rows_changed=1, rounds=2)
    line = lt.floor_line(plain, served, np.array([0, 1, 2, 1, 1], np.int32), stats, 2)
    assert line == "floor@2: 3 floor items, 1 short of their floor, below the floor 3 -> 2, 1 inserted slots, 1 rows changed, 2 rounds"


# ---------------------------------------------------------------------------------------------- the reference
def tiny_case(t):
    """the t-th of the tiny random cases: 1 .. 8 users, 1 .. 7 items, every c, k and reserve, quantised scores every other one, up to two
    padded rows, floors in [0, 3]"""
    rng = np.random.default_rng(5000 + t)
    n, I = int(rng.integers(1, 9)), int(rng.integers(1, 8))
    c = int(rng.integers(1, I + 2))
    k = int(rng.integers(1, c + 1))
    R = int(rng.integers(0, k + 1))
    s, i, lse = F.zipf_case(t, n, I, c, quant=0.5 if t % 2 else None, pad_rows=t % 3)
    return s, i, lse if t % 4 < 2 else None, rng.integers(0, 4, I).astype(np.int32), k, R, rng


# (n, I, c, k, R, M, quant, padded rows): the GPU tests' shapes, the long ones shortened
CASES = [(64, 24, 24, 5, 2, 6, None, 3), (300, 48, 24, 6, 2, 30, None, 0), (40, 500, 320, 100, 16, 1, None, 0), (200, 300, 100, 1, 1, 1, None, 0),
         (130, 70, 65, 40, 8, 40, None, 3), (211, 129, 129, 10, 3, 12, 0.5, 0), (90, 60, 33, 7, 7, 6, None, 25), (1, 10, 10, 3, 2, 1, None, 0)]


@pytest.fixture(scope="module")
def cases():
    out = []
    for n, I, c, k, R, M, quant, pad in CASES:
        s, i, lse = F.zipf_case(1000 + n + I, n, I, c, quant=quant, pad_rows=pad)
        out.append((s, i, lse, F.median_need(i, I, k, M), k, R))
    return out


def test_the_rounds_equal_the_sequential_statement_on_tiny_cases():
    lowered = differ = 0
    for t in range(200):
        s, i, lse, need, k, R, rng = tiny_case(t)
        act, lim, rounds, low = F.floor_rounds(s, i, lse, need, k, R, max_rounds=s.size + 2)
        lowered += low > 0
        I = len(need)
        for order in (None, list(range(I)), list(rng.permutation(I))):       # the last id first, the first id first, at random
            assert np.array_equal(F.floor_sequential(s, i, lse, need, k, R, order), act), (t, order)
        assert F.blocking_pairs(s, i, lse, need, k, R, act) == 0, t
        sc, ids, ts = F.compose(s, i, act, k, R)
        differ += (ts > 0).any()
        fl, live = F.floor_mask(i, need)
        held = np.bincount(i[act], minlength=I)
        assert (act <= fl).all() and (held <= np.maximum(need, 0)).all(), t
        assert (F.exposure(ids, I)[need > 0] >= np.minimum(need, held)[need > 0]).all(), t
        key = F.tk_key(np.where(ids >= 0, sc, 0)).astype(np.int64)
        for u in range(len(ids)):                        # sorted rows: the candidate positions ascend
            got = ids[u][ids[u] >= 0]
            pos = [int(np.nonzero(i[u] == g)[0][0]) for g in got]
            assert pos == sorted(set(pos)) and set(np.nonzero(act[u])[0]) <= set(pos), (t, u)
            assert (np.diff(key[u, :len(pos)]) <= 0).all(), (t, u)
    assert lowered >= 20 and differ >= 20, (lowered, differ)       # the tiny cases do exercise the rounds


def test_the_two_schedules_agree_on_the_shapes(cases):
    rounds = []
    for t, (s, i, lse, need, k, R) in enumerate(cases):
        for L in (lse, None):
            act, lim, r, low = F.floor_rounds(s, i, L, need, k, R, max_rounds=s.size + 2)
            rounds.append(r)
            assert np.array_equal(F.floor_sequential(s, i, L, need, k, R), act), t
            rng = np.random.default_rng(t)
            assert np.array_equal(F.floor_sequential(s, i, L, need, k, R, rng.permutation(len(need))), act), t
            # the limits are consistent with the matching: nothing active lies behind a row's limit
            assert not (act & (np.arange(act.shape[1])[None, :] > lim[:, None])).any()
    assert max(rounds) >= 4, rounds


def test_no_blocking_pair_the_floor_and_sorted_rows(cases):
    for t, (s, i, lse, need, k, R) in enumerate(cases):
        for L in (lse, None):
            sc, ids, act, held, st = F.floor_lists(s, i, L, need, k, R)
            assert F.blocking_pairs(s, i, L, need, k, R, act) == 0, t
            hits = F.exposure(ids, len(need))
            assert (hits[need > 0] >= np.minimum(need, held)[need > 0]).all(), t
            assert st[2] == ((need > 0) & (held < need)).sum() and st[6] == (need > 0).sum() and st[7] == 0
            _, live = F.floor_mask(i, need)
            for u in range(len(ids)):                    # distinct ids in candidate order, each with its original score; the head is plain
                got = ids[u][ids[u] >= 0]
                pos = [int(np.nonzero(i[u] == g)[0][0]) for g in got]
                assert pos == sorted(set(pos)) and np.array_equal(sc[u, :len(pos)].view(np.uint32), s[u, pos].view(np.uint32)), (t, u)
                assert pos[:k - R] == list(range(min(k - R, len(pos)))) and len(pos) == min(k, int(live[u].sum())), (t, u)
                assert (ids[u, len(pos):] == -1).all() and np.isneginf(sc[u, len(pos):]).all()
    # the checker does find blocking pairs in a table that has them: the matching without one of its entries leaves that item short and
    # its user with a free place or a worse entry
    s, i, lse, need, k, R = cases[0]
    act = F.floor_rounds(s, i, lse, need, k, R)[0]
    u, j = (int(x[0]) for x in np.nonzero(act))
    bad = act.copy()
    bad[u, j] = False
    assert F.blocking_pairs(s, i, lse, need, k, R, bad) >= 1
    assert F.blocking_pairs(s, i, lse, need, k, R, np.zeros_like(act)) >= 1


def test_no_floor_and_no_reserve_give_the_plain_lists(cases):
    for s, i, lse, need, k, R in cases:
        _, live = F.floor_mask(i, need)
        pI = np.where(live[:, :k], i[:, :k], -1)
        pS = np.where(live[:, :k], s[:, :k], -np.inf).astype(np.float32)
        for nd, r in ((np.zeros_like(need), R), (need, 0)):
            sc, ids, act, held, st = F.floor_lists(s, i, lse, nd, k, r)
            assert np.array_equal(ids, pI) and np.array_equal(sc.view(np.uint32), pS.view(np.uint32))
            assert st[[0, 1, 3, 4, 5]].tolist() == [0, 1, 0, 0, 0] and not act[:, k:].any()


def test_equal_scores_go_to_the_lower_row_and_zero_has_one_sign():
    """one floor item behind every user's first entry, scored 0.0 with either sign: the floor takes the lowest rows, and the zeros keep
    their signs"""
    n, M = 12, 5
    s = np.zeros((n, 2), np.float32)
    s[::2, 1] = -0.0
    s[:, 0] = 1.0
    i = np.tile(np.array([[0, 1]], np.int32), (n, 1))
    sc, ids, act, held, st = F.floor_lists(s, i, None, np.array([0, M], np.int32), 1, 1)
    assert ids[:, 0].tolist() == [1] * M + [0] * (n - M) and held.tolist() == [0, M]
    assert np.array_equal(sc[:M, 0].view(np.uint32), s[:M, 1].view(np.uint32))
    assert st.tolist() == [0, 1, 0, M, 0, M, 1, 0]
