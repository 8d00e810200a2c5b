"""CPU-side checks of the exploration lists: ltg_topk_sample / ltg_topk_sample_mass / ltg_topk_sample_finish are exported and bound with
the header's argument types, every documented refusal returns LTG_EINVAL without a GPU, Explore and the Recommender validate, both CLIs
handle --explore, and the numpy reference the GPU tests lean on (tests/explore_ref.py): its Gumbel-top-k lists equal the sequential
definition fed the same noise, logp has its closed form on two items, a fixed head is the plain list, the lists follow the
Plackett-Luce distribution, and the RNG-mode parity cases hold few near-ties."""
import ctypes as C
import os

import numpy as np
import pytest

import explore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHI2_BOUND = 119.9                                       # chi2.ppf(1 - 1e-6, 55)


def test_entry_points_are_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    cfg, bt = C.POINTER(cabi.ltg_config), C.POINTER(cabi.ltg_batch)
    want = {"ltg_topk_sample": [cfg, vp, bt, i32, i32, i32, f32, C.c_uint64, vp, i32, vp, vp, vp, vp],
            "ltg_topk_sample_mass": [cfg, vp, bt, i32, i32, f32, vp, i32, vp, vp, vp, vp, vp],
            "ltg_topk_sample_finish": [i32, i32, vp, vp, vp, f32, vp, vp]}
    for name, args in want.items():
        assert cabi.SYMBOLS[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_ABI_VERSION 14" in header
    assert ("int ltg_topk_sample(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t row_lo, int32_t k, "
            "float inv_temp,") in header
    assert "int ltg_topk_sample_mass(const ltg_config* cfg, const float* logits, const ltg_batch* tr, int32_t n_rows, int32_t k, float inv_temp," in header
    assert "int ltg_topk_sample_finish(int32_t n_rows, int32_t k, const float* score, const float* M, const float* rest, float inv_temp," in header
    rng_h = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_rng.h")).read()
    assert "#define LTG_STREAM_SERVE_GUMBEL 8" in rng_h and R.STREAM_SERVE_GUMBEL == 8
    hip = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_kernels.hip")).read()
    assert hip.index('#include "ltg_topk.h"') < hip.index('#include "ltg_explore.h"')


def _cfg(cabi, n_items=1000, item_lo=0, n_glob=0):
    return cabi.ltg_config(n_items, 600, 200, n_items, 100, 150, 250, 300, 0, 0, item_lo, n_glob, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


def test_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    fb, ib = (C.c_float * 64)(), (C.c_int32 * 64)()
    good = _cfg(cabi)

    def batch(n_rows=2, indptr=True, indices=True):
        return cabi.ltg_batch(n_rows, 0, C.addressof(ib) if indptr else None, C.addressof(ib) if indices else None, None, None, None, None, None,
                              None, None)

    def sample(cfg=good, logits=fb, tr=None, n=2, row_lo=0, k=4, it=1.0, draw=0, excl=None, f=0, g=None, ko=fb, io=ib):
        return lib.ltg_topk_sample(C.byref(cfg) if cfg is not None else None, logits, C.byref(tr) if tr is not None else None, n, row_lo, k, it,
                                   draw, excl, f, g, ko, io, None)

    def mass(cfg=good, logits=fb, tr=None, n=2, k=4, it=1.0, excl=None, f=0, ids=ib, so=fb, mo=fb, ro=fb):
        return lib.ltg_topk_sample_mass(C.byref(cfg) if cfg is not None else None, logits, C.byref(tr) if tr is not None else None, n, k, it,
                                        excl, f, ids, so, mo, ro, None)

    def finish(n=2, k=4, sc=fb, M=fb, rest=fb, it=1.0, lp=fb):
        return lib.ltg_topk_sample_finish(n, k, sc, M, rest, it, lp, None)

    # zero rows: nothing is launched, but the arguments are still checked
    assert sample(n=0) == 0 and mass(n=0) == 0 and finish(n=0) == 0
    assert sample(n=0, k=1024, excl=ib, f=7, tr=batch(0), g=fb, draw=2 ** 64 - 1, row_lo=2 ** 31 - 1) == 0 and mass(n=0, k=1024, excl=ib, f=7) == 0
    for call, outs in ((sample, ("ko", "io")), (mass, ("ids", "so", "mo", "ro")), (finish, ("sc", "M", "rest", "lp"))):
        for name in outs:
            assert call(**{name: None}) == -1 and call(n=0, **{name: None}) == -1, (call.__name__, name)
        for k in (0, -1, 1025):
            assert call(k=k) == -1 and call(n=0, k=k) == -1, (call.__name__, k)
        for it in (0.0, -1.0, float("inf"), -float("inf"), float("nan")):
            assert call(it=it) == -1 and call(n=0, it=it) == -1, (call.__name__, it)
        assert call(n=-1) == -1
    for call in (sample, mass):
        assert call(cfg=None) == -1 and call(logits=None) == -1
        assert call(f=-1) == -1 and call(f=-1, excl=ib) == -1 and call(f=3, excl=None) == -1 and call(n=0, f=3) == -1
        assert call(cfg=_cfg(cabi, 0)) == -1 and call(cfg=_cfg(cabi, -5)) == -1                   # what ltg_topk refuses
        assert call(cfg=_cfg(cabi, 425985)) == -1                                                 # (a slab beyond the LDS bitset)
        assert call(cfg=_cfg(cabi, 1000, item_lo=-1)) == -1
        assert call(tr=batch(3)) == -1 and call(tr=batch(indptr=False)) == -1 and call(tr=batch(indices=False)) == -1
        assert call(n=0, tr=batch(0)) == 0 and call(n=0, cfg=_cfg(cabi, 360448)) == 0
    assert sample(row_lo=-1) == -1 and sample(n=0, row_lo=-1) == -1
    # what ltg_topk itself refuses, for comparison
    assert lib.ltg_topk(C.byref(_cfg(cabi, 0)), fb, None, 2, 4, fb, ib, None) == -1
    assert lib.ltg_topk(C.byref(_cfg(cabi, 425985)), fb, None, 2, 4, fb, ib, None) == -1


class _FakeEngine:
    I, I_global, device, item_lo = 50, 50, "cpu", 0


def test_explore_validation_and_re_exports():
    from ltgan.serving import Explore as ServingExplore
    from ltgan.serving import Rule
    from ltgan.sharded import Explore as ShardedExplore
    from ltgan.trainer import Calibrate, Diversify, Explore, Recommender
    assert ShardedExplore is Explore is ServingExplore and issubclass(Explore, Rule) and not Explore.whole and not Explore.needs_lse
    for T in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            Explore(T)
    for kw in (dict(fixed=-1), dict(fixed=1.5), dict(draw=-1), dict(draw=0.5), dict(draw=2 ** 64)):
        with pytest.raises(ValueError):
            Explore(1.0, **kw)
    e = Explore(0.5, fixed=3, draw=7)
    assert e.inv_temp == np.float32(2.0) and e.inv_temp.dtype == np.float32 and (e.fixed, e.draw) == (3, 7)
    assert Explore(0.3).inv_temp == R.inv_temp_of(0.3) == np.float32(1.0 / 0.3)
    for k in (3, 2, 1):                                                  # 0 <= fixed < k at bind
        with pytest.raises(ValueError):
            Explore(1.0, fixed=3).bind(_FakeEngine(), 10, k, 33)
    e.bind(_FakeEngine(), 10, 20, 33)
    assert e.longest == 20 and tuple(e.logp.shape) == (33, 20) and tuple(e.keys.shape) == (33, 20) and float(e.logp.abs().sum()) == 0.0
    assert e.pick_i.numel() == 10 * 17 and e.head_i.numel() == 10 * 3 and e.table().shape == (33, 20)
    e0 = Explore(1.0)
    e0.bind(_FakeEngine(), 4, 1, 6)                                      # k = 1, no head
    assert e0.longest == 1 and e0.pick_i.numel() == 4
    labels = np.zeros(50, np.uint8)
    for kw in (dict(rule=object()), dict(diversify=Diversify(0.5)), dict(calibrate=Calibrate(labels, 2, 0.5)), dict(cap=object()),
               dict(share=object()), dict(floor=object()), dict(gate=object())):
        with pytest.raises(ValueError, match="explore= cannot be combined with"):
            Recommender(_FakeEngine(), None, k=10, explore=Explore(1.0), **kw)
    with pytest.raises(ValueError):
        Recommender(_FakeEngine(), None, k=0, explore=Explore(1.0))


def test_cli_arguments():
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    for mod in (rc, lt):
        a = mod.parse_args(["ds", "model.pt"])                           # nothing changes without the option
        assert a.explore is None and a.explore_fixed is None and a.explore_draw is None
        assert mod.parse_args(["ds", "m.pt", "--explore", "0.5"]).explore == 0.5
        a = mod.parse_args(["ds", "m.pt", "--explore", "2", "--explore-fixed", "5", "--explore-draw", "11"])
        assert (a.explore, a.explore_fixed, a.explore_draw) == (2.0, 5, 11)
        for bad in (["--explore", "0"], ["--explore", "-1"], ["--explore", "nan"], ["--explore", "inf"], ["--explore", "x"], ["--explore"],
                    ["--explore-fixed", "3"], ["--explore-draw", "3"], ["--explore", "1", "--explore-fixed", "-1"],
                    ["--explore", "1", "--explore-fixed", "100"], ["--explore", "1", "--explore-draw", "-1"],
                    ["--explore", "1", "--min-slots", "niche:5"], ["--explore", "1", "--diversify", "0.5"], ["--explore", "1", "--calibrate", "0.5"],
                    ["--explore", "1", "--cap", "5"], ["--explore", "1", "--share", "niche:0.3"],
                    ["--explore", "1", "--floor", "2", "--floor-reserve", "5"], ["--explore", "1", "--gate", "0.5"]):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(["ds", "m.pt"] + bad)
            assert e.value.code == 2, (mod.__name__, bad)
        assert mod.parse_args(["ds", "m.pt", "--explore", "1", "--critic"]).critic == 0      # the critic reads the explored lists
    a = rc.parse_args(["ds", "m.pt", "--explore", "1"])
    assert a.propensities == "props.tsv" and rc.parse_args(["ds", "m.pt", "--explore", "1", "--propensities", "p.tsv"]).propensities == "p.tsv"
    assert rc.parse_args(["ds", "m.pt", "--explore", "1", "--explain", "3"]).explain == 3
    assert rc.parse_args(["ds", "m.pt", "--explore", "1", "--k", "10", "--explore-fixed", "9"]).explore_fixed == 9
    for bad in (["--propensities", "p.tsv"], ["--explore", "1", "--k", "10", "--explore-fixed", "10"]):
        with pytest.raises(SystemExit):
            rc.parse_args(["ds", "m.pt"] + bad)


def test_propensity_file_and_summary_line(tmp_path):
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    ids = np.array([[5, 2, 9], [7, -1, -1]], np.int32)
    logp = np.array([[0.0, -1.25, -0.333333333], [-2.5e-7, 0.0, 0.0]], np.float32)
    p = str(tmp_path / "props.tsv")
    assert rc.write_propensities(logp, ids, 40, p) == 2
    assert open(p).read() == "40\t5:0,2:-1.25,9:-0.333333\n41\t7:-2.5e-07\n"
    rc.write_recs(ids, logp, 40, None, str(tmp_path / "r.npz"), logp=logp)
    z = np.load(str(tmp_path / "r.npz"))
    assert np.array_equal(z["logp"], logp) and z["logp"].dtype == np.float32

    class _Exp:
        temperature, fixed, draw = 0.5, 2, 3

        def stats(self):
            return dict(mean_logp=-12.5, explored_share=0.25, sampled=8)

    assert lt.explore_line(_Exp(), 100) == "explore@100: T 0.5, fixed 2, draw 3, mean list logp -12.500000, explored share 0.250000"


# ---------------------------------------------------------------------------------------------- the reference
@pytest.fixture(scope="module")
def rows():
    return R.build_rows(11, 67, reps=3)


def test_gumbel_top_k_equals_the_sequential_definition(rows):
    """the lists are the sequential draws' and logp is the log-probability each draw had; rows with a near-tie among the keys are left
    to the tie rule (the sequential form renormalises in float64, the keys are float32)"""
    S, fold, G, kinds = rows
    checked = 0
    for u in range(S.shape[0]):
        for k, F, T in ((5, 0, 1.0), (12, 3, 0.5), (67, 1, 2.0), (80, 7, 1.0)):
            it = R.inv_temp_of(T)
            w = R.explore_row(S[u], fold[u], k, F, it, G[u])
            ids, lps = R.sequential_row(S[u], fold[u], k, F, it, G[u])
            n = len(ids)
            assert n == min(k, int((~fold[u]).sum())) and (w["ids"][n:] == -1).all() and (w["logp"][n:] == 0).all(), (u, kinds[u])
            if kinds[u] in ("regular", "neginf", "short") and not R.near_tie(S[u], fold[u], k - F, it, G[u], excl=w["head"], gap=1e-4):
                assert w["ids"][:n].tolist() == ids, (u, kinds[u], k, F)
                ok = np.isfinite(lps) & (np.concatenate([np.zeros(F), w["x"]])[:n] >= -80)
                assert np.allclose(w["logp"][:n][ok], np.array(lps)[ok], rtol=0, atol=1e-9), (u, kinds[u])
                checked += 1
            elif kinds[u] in ("equal", "zeros"):                         # every key equal: the ids in order, uniform probabilities
                el = np.nonzero(~fold[u])[0]
                assert w["ids"][:n].tolist() == el[:n].tolist()
                assert np.allclose(w["logp"][F:n], -np.log(len(el) - F - np.arange(n - F)), atol=1e-12)
                checked += 1
    assert checked > 40


def test_logp_of_a_two_item_catalogue_has_its_closed_form():
    for a, b, T in ((0.3, -1.2, 1.0), (2.0, 2.0, 0.5), (-4.0, 5.0, 0.1), (1.0, 0.0, 3.0)):
        s, it = np.array([a, b], np.float32), R.inv_temp_of(T)
        for g in (np.array([0.0, 0.0], np.float32), np.array([-50.0, 50.0], np.float32)):
            w = R.explore_row(s, np.zeros(2, bool), 2, 0, it, g)
            first = int(w["ids"][0])
            d = (np.float64(s[1 - first]) - np.float64(s[first])) * np.float64(it)
            assert abs(w["logp"][0] + np.log1p(np.exp(d))) < 1e-12 and abs(w["logp"][1]) < 1e-12   # p = 1 / (1 + exp(d)); the last item is certain
            w1 = R.explore_row(s, np.zeros(2, bool), 1, 0, it, g)
            assert w1["ids"][0] == first and abs(w1["logp"][0] - w["logp"][0]) < 1e-12


def test_a_fixed_head_is_the_plain_list(rows):
    S, fold, G, kinds = rows
    for u in range(S.shape[0]):
        for F in (1, 7):
            w = R.explore_row(S[u], fold[u], 20, F, np.float32(1.0), G[u])
            pi, ps = R.plain_topk(S[u], fold[u], F)
            assert np.array_equal(w["ids"][:F], pi) and np.array_equal(w["scores"][:F].view(np.uint32), ps.view(np.uint32))
            assert (w["logp"][:F] == 0).all()
            real = w["ids"][w["ids"] >= 0]
            assert len(set(real.tolist())) == len(real) and not fold[u][real].any(), (u, kinds[u])


@pytest.mark.parametrize("T", [1.0, 0.5])
def test_reference_lists_follow_the_plackett_luce_distribution(T):
    chi, low = R.pair_chi2(R.pair_lists(T), T)
    print("T %.1f: chi-square %.1f over 56 ordered pairs, smallest expected cell %.1f" % (T, chi, low))
    assert low > 15 and chi < CHI2_BOUND


@pytest.mark.parametrize("case", range(len(R.RNG_CASES)))
def test_rng_parity_cases_hold_few_near_ties(case):
    _, _, tie, _ = R.rng_case_reference(case)
    print("case %s: rows with a near-tie %.4f" % (R.RNG_CASES[case], tie.mean()))
    assert tie.mean() <= 0.02
