"""CPU-side checks of the critic-checked lists: the numpy reference the GPU tests compare against (tests/critic_ref.py) --
the fixed-point mean does not depend on the order or the split of the anchors, the gate's walk -- the three entry points are exported and
answer bad arguments before any HIP call, and the constructors' and the CLIs' argument handling."""
import ctypes as C

import numpy as np
import pytest

import critic_ref as KR
from oracle import ltg_oracle as O

EINVAL = -1


# ---------------------------------------------------------------------------------------------- the reference
def _toy(seed=0, I=60, F=60, hs=(8, 5, 7, 13)):
    """a tiny discriminator, sides and CSR histories: user 0 has no history, user 1 niche items only, the others are mixed"""
    rng = np.random.default_rng(seed)
    D = O.init_discriminator(F, *hs, seed=3)
    for key in ("b1", "b2", "b3", "b4"):
        D[key] = rng.normal(0, 0.1, np.shape(D[key]))
    niche = set(range(30, I))
    valid = set(range(I)) - {4, 7, 33, 59}                # two popular and two niche items have no features
    pop_ids, niche_ids, pop_row, niche_row = KR.side_maps(niche, valid, I)
    rows = [[], [31, 35, 58], [0, 1, 2, 4, 40], [5], list(range(0, 30)) + [44], [7, 4]]
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    indices = np.array([x for r in rows for x in r], np.int32)
    S = KR.reference_scores(D, pop_ids, niche_ids)
    return D, pop_ids, niche_ids, pop_row, niche_row, indptr, indices, S


def test_side_maps_and_anchors():
    _, pop_ids, niche_ids, pop_row, niche_row, indptr, indices, S = _toy()
    assert pop_ids.tolist() == [i for i in range(30) if i not in (4, 7)] and niche_ids.tolist() == [i for i in range(30, 60) if i not in (33, 59)]
    assert S.shape == (28, 28) and S.dtype == np.float32
    assert pop_row[4] == pop_row[7] == pop_row[30] == -1 and niche_row[33] == niche_row[59] == niche_row[0] == -1
    assert pop_row[pop_ids].tolist() == list(range(28)) and niche_row[niche_ids].tolist() == list(range(28))
    got = [KR.anchors_of(indptr, indices, u, pop_row).tolist() for u in range(6)]
    assert got == [[], [], [0, 1, 2], [5], [i for i in range(30) if i not in (4, 7)], []]
    # a slab's part of a history: local ids, hist_lo makes them global; ids outside the catalogue count nowhere
    assert KR.anchors_of(np.array([0, 4]), np.array([-25, 0, 1, 45]), 0, pop_row, hist_lo=20).tolist() == [20, 21]


def test_critic_ref_on_a_hand_made_table():
    pop_row = np.array([0, 1, -1, -1, -1], np.int32)
    niche_row = np.array([-1, -1, 0, 1, -1], np.int32)
    S = np.array([[1.5, -0.25], [2.0, -0.25]], np.float32)
    indptr, indices = np.array([0, 2, 2, 3]), np.array([1, 0, 4])
    ids = np.array([[2, 3, 0, -1], [3, 2, 4, 9], [2, -1, -1, -1]])
    r = KR.critic_ref(S, indptr, indices, pop_row, niche_row, ids, 4)
    assert r["cnt"].tolist() == [2, 0, 0]
    assert r["sum"].tolist() == [[int(3.5 * 2 ** 24), -int(0.5 * 2 ** 24), 0, 0], [0] * 4, [0] * 4]
    assert r["best_i"].tolist() == [[1, 0, -1, -1], [-1] * 4, [-1] * 4]          # 2.0 beats 1.5; equal scores: the lower id
    assert r["best_s"][0, :2].tolist() == [2.0, -0.25] and np.all(np.isneginf(r["best_s"][1:])) and np.all(np.isneginf(r["best_s"][0, 2:]))
    assert r["crit"].tolist() == [[1.75, -0.25, 0.0, 0.0], [0.0] * 4, [0.0] * 4] and r["crit"].dtype == np.float32
    assert r["scored"].tolist() == [[True, True, False, False], [False] * 4, [False] * 4] and r["n_scored"].tolist() == [2, 0, 0]
    r2 = KR.critic_ref(S, indptr, indices, pop_row, niche_row, ids, 1)
    assert r2["sum"].tolist() == [[int(3.5 * 2 ** 24)], [0], [0]] and r2["crit"].shape == (3, 1)


def test_fixed_point_is_round_half_even_and_exact():
    s = np.array([2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, -3 * 2.0 ** -25, 1.0, -7.625, 2.0 ** -30, 131071.99], np.float32)
    assert KR.fixed(s).tolist() == [0, 2, 0, -2, 2 ** 24, -int(7.625 * 2 ** 24), 0, int(np.float32(131071.99) * 2 ** 24)]
    assert KR.fixed(s).dtype == np.int64
    assert KR.mean_fixed(3 * 2 ** 24, 2) == np.float32(1.5) and isinstance(KR.mean_fixed(1, 3), np.float32)
    assert KR.mean_fixed(1, 3) == np.float32(1.0 / 3.0 / 2 ** 24)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fixed_point_mean_is_invariant_under_permutation_and_split(seed):
    """integer sums commute and associate: any order of the anchors and any split into parts whose sums and counts are added gives the same
    float32 bits -- what lets item shards merge bit for bit (a float32 or float64 sum of the same logits does NOT have the property)"""
    rng = np.random.default_rng(seed)
    for n in (1, 2, 9, 129, 600):
        s = (rng.normal(0, 3, n) * 10.0 ** rng.integers(-6, 2, n)).astype(np.float32)
        want = KR.mean_fixed(KR.fixed(s).sum(), n)
        for _ in range(5):
            p = rng.permutation(n)
            assert KR.mean_fixed(KR.fixed(s[p]).sum(), n).view(np.uint32) == want.view(np.uint32)
            cuts = np.sort(rng.integers(0, n + 1, rng.integers(1, 5)))
            parts = np.split(s[p], cuts)                     # some parts are empty
            total = sum(int(KR.fixed(x).sum()) for x in parts)
            assert sum(x.size for x in parts) == n
            assert KR.mean_fixed(total, n).view(np.uint32) == want.view(np.uint32)
        assert abs(float(want) - float(s.astype(np.float64).mean())) <= 2.0 ** -25 + 2.0 ** -24 * abs(float(s.astype(np.float64).mean()))


def test_critic_ref_splits_over_slabs():
    """two slabs' histories: the sums and counts added, the better of the two best anchors -- the whole history's result, bit for bit"""
    _, _, _, pop_row, niche_row, indptr, indices, S = _toy()
    ids = np.array([[31, 0, 40, 33, -1, 58]] * 6)
    whole = KR.critic_ref(S, indptr, indices, pop_row, niche_row, ids, 6)
    cut = 12
    parts = []
    for lo, hi in ((0, cut), (cut, 60)):
        rows = [[x - lo for x in indices[indptr[u]:indptr[u + 1]] if lo <= x < hi] for u in range(6)]
        ip = np.cumsum([0] + [len(r) for r in rows])
        ix = np.array([x for r in rows for x in r], np.int64)
        parts.append(KR.critic_ref(S, ip, ix, pop_row, niche_row, ids, 6, hist_lo=lo))
    total, cnt = parts[0]["sum"] + parts[1]["sum"], parts[0]["cnt"] + parts[1]["cnt"]
    assert np.array_equal(total, whole["sum"]) and np.array_equal(cnt, whole["cnt"]) and cnt.tolist() == [0, 0, 3, 1, 28, 0]
    cand = (niche_row[np.clip(ids, 0, 59)] >= 0) & (ids >= 0)
    fin = KR.finish_ref(total, cnt, cand)
    assert np.array_equal(fin["crit"].view(np.uint32), whole["crit"].view(np.uint32)) and np.array_equal(fin["scored"], whole["scored"])
    for u in range(6):
        for e in range(6):
            both = [(p["best_s"][u, e], p["best_i"][u, e]) for p in parts if p["best_i"][u, e] >= 0]
            if not both:
                assert whole["best_i"][u, e] == -1
                continue
            s, g = KR.best_of(np.array([b[0] for b in both]), np.array([b[1] for b in both]))
            assert g == whole["best_i"][u, e] and s == whole["best_s"][u, e]
    assert whole["scored"][4].tolist() == [True, False, True, False, False, True] and not whole["scored"][[0, 1, 5]].any()


def test_gate_ref():
    ninf = -np.inf
    s = np.array([[9.0, 8.0, 7.0, 6.0, 5.0, 4.0]] * 5, np.float32)
    i = np.array([[10, 40, 11, 41, 42, 12]] * 5, np.int32)
    crit = np.array([[0.0, -1.0, 0.0, 0.5, 2.0, 0.0]] * 5, np.float32)
    flag = np.array([[-1, 3, -1, 3, 5, -1]] * 5, np.int32)
    flag[3] = -1                                            # a row without anchors: nothing is scored, everything passes
    i[4, 4:] = -1                                           # padding at the end of the candidates
    gs, gi, st = KR.gate_ref(s, i, crit, flag, ninf, 4)
    assert np.array_equal(gi, i[:, :4]) and np.array_equal(gs, s[:, :4])              # tau = -inf: the plain prefix
    assert st.tolist() == [[3, 0, 4], [3, 0, 4], [3, 0, 4], [0, 0, 4], [2, 0, 4]]
    gs, gi, st = KR.gate_ref(s[:1], i[:1], crit[:1], flag[:1], 0.5, 4)                 # crit == tau passes (>=)
    assert gi.tolist() == [[10, 11, 41, 42]] and gs.tolist() == [[9.0, 7.0, 6.0, 5.0]] and st.tolist() == [[3, 1, 4]]
    # every niche entry rejected: the popular entries in order, then padding
    gs, gi, st = KR.gate_ref(s, i, crit, flag, 3.0, 4)
    assert gi[0].tolist() == [10, 11, 12, -1] and gs[0].tolist() == [9.0, 7.0, 4.0, ninf] and st[0].tolist() == [3, 3, 3]
    assert gi[3].tolist() == [10, 40, 11, 41] and st[3].tolist() == [0, 0, 4]
    assert gi[4].tolist() == [10, 11, -1, -1] and st[4].tolist() == [2, 2, 2]
    # a rejection after the list is full does not count
    gs, gi, st = KR.gate_ref(s[:1], i[:1], crit[:1], flag[:1], 3.0, 2)
    assert gi.tolist() == [[10, 11]] and st.tolist() == [[3, 1, 2]]
    assert gs.dtype == np.float32 and gi.dtype == np.int32 and st.dtype == np.int32


# ---------------------------------------------------------------------------------------------- the entry points, without a GPU
def check_refusals(cabi, lib, p):
    """every LTG_EINVAL case of the three entry points, answered before any HIP call: `p` is any non-NULL address (never read)"""
    cfg = lambda hs=(100, 150, 250, 300), feat=1000: cabi.ltg_config(feat, 600, 200, feat, *hs, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    disc = cabi.ltg_disc_state()
    disc.emb = p
    for j in range(8):
        disc.p[j] = p

    def batch(n):
        b = cabi.ltg_batch()
        b.n_rows, b.indptr, b.indices = n, p, p
        return b

    def critic(cfg=cfg(), disc=disc, pi=p, n_pop=5, ni=p, n_niche=5, pr=p, nr=p, I=100, tr=batch(4), hist_lo=0, n=4, k_in=100, ids=p, top=100,
               so=p, co=p, bs=p, bi=p):
        return lib.ltg_pair_critic(C.byref(cfg) if cfg is not None else None, C.byref(disc) if disc is not None else None, pi, n_pop, ni, n_niche,
                                   pr, nr, I, C.byref(tr) if tr is not None else None, hist_lo, n, k_in, ids, top, so, co, bs, bi, None)
    for name in ("pi", "ni", "pr", "nr", "ids", "so", "co", "bs", "bi", "cfg", "disc", "tr"):
        assert critic(**{name: None}) == EINVAL, name
    assert critic(cfg=cfg((100, 150, 250, 353))) == EINVAL and critic(cfg=cfg((100, 150, 250, 0))) == EINVAL
    assert critic(n=-1, tr=batch(-1)) == EINVAL and critic(n=3) == EINVAL and critic(hist_lo=-1) == EINVAL and critic(I=0) == EINVAL
    assert critic(n_pop=-1) == EINVAL and critic(n_niche=-1) == EINVAL
    assert critic(top=0) == EINVAL and critic(top=101) == EINVAL and critic(k_in=300, top=257) == EINVAL and critic(k_in=0, top=0) == EINVAL
    assert critic(k_in=1025) == EINVAL
    for j in (6, 7):
        d2 = cabi.ltg_disc_state()
        for t in range(8):
            d2.p[t] = None if t == j else p
        assert critic(disc=d2) == EINVAL, j
    no_ptr = batch(4)
    no_ptr.indptr = None
    assert critic(tr=no_ptr) == EINVAL
    assert critic(n=0, tr=batch(0)) == 0 and critic(n=0, tr=batch(0), top=0) == EINVAL

    def finish(n=4, k_in=100, ids=p, top=100, nr=p, I=100, n_niche=5, s=p, c=p, out=p, sc=p):
        return lib.ltg_critic_finish(n, k_in, ids, top, nr, I, n_niche, s, c, out, sc, None)
    for name in ("ids", "nr", "s", "c", "out", "sc"):
        assert finish(**{name: None}) == EINVAL, name
    assert finish(n=-1) == EINVAL and finish(I=0) == EINVAL and finish(n_niche=-1) == EINVAL
    assert finish(top=0) == EINVAL and finish(top=101) == EINVAL and finish(k_in=300, top=257) == EINVAL and finish(k_in=1025) == EINVAL
    assert finish(n=0) == 0

    def gate(n=4, c_in=200, s=p, i=p, cr=p, fl=p, tau=0.0, k=100, so=p, io=p, st=p):
        return lib.ltg_topk_gate(n, c_in, s, i, cr, fl, tau, k, so, io, st, None)
    for name in ("s", "i", "cr", "fl", "so", "io", "st"):
        assert gate(**{name: None}) == EINVAL, name
    assert gate(n=-1) == EINVAL and gate(c_in=0, k=0) == EINVAL and gate(c_in=257) == EINVAL and gate(k=0) == EINVAL and gate(k=201) == EINVAL
    assert gate(tau=float("nan")) == EINVAL
    assert gate(n=0) == 0 and gate(n=0, tau=float("-inf")) == 0 and gate(n=0, k=201) == EINVAL


def test_entry_points_are_exported_and_refuse_bad_arguments_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    for name in ("ltg_pair_critic", "ltg_critic_finish", "ltg_topk_gate"):
        assert name in cabi.SYMBOLS and getattr(lib, name).argtypes == cabi.SYMBOLS[name][1]
    assert lib.ltg_abi_version() == 14 and cabi.LTG_CRITIC_MAX_TOP == cabi.LTG_GATE_MAX_C == 256
    buf = (C.c_float * 16)()
    check_refusals(cabi, lib, C.cast(buf, C.c_void_p).value)
    assert not any(buf)


# ---------------------------------------------------------------------------------------------- the classes and the CLIs
def test_constructors_refuse_bad_arguments():
    from ltgan.serving import Critic, CriticGate, ExposureCap, Recommender, gate_tau
    niche, valid = {3, 4, 5}, {0, 1, 3, 4}
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_prob"):
            CriticGate(niche, valid, bad)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="candidates"):
            CriticGate(niche, valid, 0.5, candidates=bad)
        with pytest.raises(ValueError, match="top"):
            Critic(niche, valid, top=bad)
    g = CriticGate(niche, valid, 0.5, candidates=40)
    assert g.tau == np.float32(0.0) and g.sides.pop_host.tolist() == [0, 1] and g.sides.niche_host.tolist() == [3, 4]
    for k in (41, 100):                                   # candidates outside [k, 256]: refused when the list length is known
        with pytest.raises(ValueError, match=r"candidates must be in \[k, 256\]"):
            g.bind(None, 10, k, 10)
    with pytest.raises(ValueError, match=r"candidates must be in \[k, 256\]"):
        CriticGate(niche, valid, 0.5).bind(None, 10, 257, 10)
    with pytest.raises(ValueError, match="top"):
        Critic(niche, valid, top=50).bind(None, 10, 49, 10)
    assert np.isneginf(gate_tau(0.0)) and gate_tau(0.0).dtype == np.float32
    assert gate_tau(0.75) == np.float32(np.log(3.0)) and gate_tau(0.25) == np.float32(-np.log(3.0))
    # gate= is one of the "at most one of" rules, named last
    with pytest.raises(ValueError, match=r"^gate= cannot be combined with cap=$"):
        Recommender(None, None, cap=ExposureCap(3), gate=g)
    with pytest.raises(ValueError, match="k = 0"):
        Recommender(None, None, k=0, critic=Critic(niche, valid))


def test_cli_arguments():
    from ltgan import longtail as LT
    from ltgan import recommend as RC
    a = RC.parse_args(["ds", "ck.pt"])
    assert a.gate is None and a.gate_candidates is None and a.critic is None and a.critic_out is None
    a = RC.parse_args(["ds", "ck.pt", "--gate", "0.5", "--gate-candidates", "150", "--critic"])
    assert a.gate == 0.5 and a.gate_candidates == 150 and a.critic == 0 and a.critic_out == "critic.tsv"
    a = RC.parse_args(["ds", "ck.pt", "--critic", "7", "--critic-out", "c.tsv", "--min-slots", "niche:5"])
    assert a.critic == 7 and a.critic_out == "c.tsv" and a.gate is None
    a = LT.parse_args(["ds", "ck.pt", "--gate", "0", "--critic", "100"])
    assert a.gate == 0.0 and a.critic == 100
    for mod, bad in ((RC, ["--gate", "1"]), (RC, ["--gate", "-0.1"]), (RC, ["--gate-candidates", "150"]), (RC, ["--gate", "0.5", "--gate-candidates", "99"]),
                     (RC, ["--gate", "0.5", "--gate-candidates", "257"]), (RC, ["--gate", "0.5", "--k", "300"]), (RC, ["--gate", "0.5", "--cap", "3"]),
                     (RC, ["--gate", "0.5", "--diversify", "0.5"]), (RC, ["--critic-out", "c.tsv"]), (RC, ["--critic", "101"]), (RC, ["--critic", "-1"]),
                     (RC, ["--k", "300", "--critic", "257"]), (LT, ["--gate", "1.0"]), (LT, ["--gate", "0.5", "--share", "niche:0.3"]),
                     (LT, ["--gate", "0.5", "--gate-candidates", "50"]), (LT, ["--critic", "300"])):
        with pytest.raises(SystemExit):
            mod.parse_args(["ds", "ck.pt"] + bad)


def test_cli_writers(tmp_path):
    from ltgan import longtail as LT
    from ltgan import recommend as RC
    ids = np.array([[5, 9, -1], [7, 5, 3]], np.int32)
    table = dict(crit=np.array([[0.0, 0.0, 0.0], [np.log(3.0), 0.0, -30.0]], np.float32), anchor_i=np.array([[-1, -1, -1], [2, -1, 0]], np.int32),
                 anchor_s=np.array([[-np.inf] * 3, [2.0, -np.inf, 0.0]], np.float32), n_anchor=np.array([0, 4], np.int32))
    path = str(tmp_path / "critic.tsv")
    assert RC.write_critic(table, ids, 100, path) == 2
    assert open(path).read().splitlines() == ["101\t7\t0.750000\t2:0.880797", "101\t3\t0.000000\t0:0.500000"]
    npz = str(tmp_path / "r.npz")
    RC.write_recs(ids, np.zeros((2, 3), np.float32), 100, None, npz, critic=table)
    z = np.load(npz)
    assert np.array_equal(z["crit"], table["crit"]) and np.array_equal(z["anchor_ids"], table["anchor_i"]) and z["n_anchor"].tolist() == [0, 4]
    assert np.array_equal(z["anchor_scores"], table["anchor_s"]) and "why_ids" not in z.files
    RC.write_recs(ids, np.zeros((2, 3), np.float32), 100, None, npz)
    assert sorted(np.load(npz).files) == ["ids", "scores", "uids"]
    assert LT.gate_line(np.array([[3, 1, 100], [0, 0, 99]]), 0.5, 100) == "gate@100: 3 scored candidates, 1 rejected, 1 short lists (min_prob 0.5)"
    assert LT.critic_line(dict(scored=2, users_with_anchors=1, mean_prob=0.375), 3) == "critic@3: 2 scored entries, 1 users with anchors, mean prob 0.375000"
