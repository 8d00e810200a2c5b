"""CPU-side checks of the diversified lists: ltg_topk_diversify is exported and bound with the header's argument types, every documented
refusal returns LTG_EINVAL without a GPU, Diversify validates, both CLIs handle --diversify / --candidates / --div-space (usage errors
through the scripts themselves), the extra summary line, and the numpy reference the GPU tests lean on: equal to a brute-force loop on
hand-made similarities full of ties, and with identical fp32 and fp64 pick sequences on the exact inputs of the GPU parity test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import diversify_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32 = C.c_void_p, C.c_int32
    args = [vp, i32, i32, i32, i32, vp, vp, C.c_float, i32, vp, vp, vp, vp]
    assert cabi.SYMBOLS["ltg_topk_diversify"] == (C.c_int, args)
    assert lib.ltg_topk_diversify.argtypes == args and lib.ltg_topk_diversify.restype == C.c_int
    assert cabi.LTG_DIV_MAX_C == 256
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_DIV_MAX_C 256" in header
    assert "int ltg_topk_diversify(const uint16_t* image, int32_t image_lo, int32_t image_rows, int32_t n_rows, int32_t c_in," in header


def test_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    img = (C.c_uint16 * (608 * 4 + 8))()
    base = C.addressof(img)
    base += (-base) % 16                                                # the image is read by 16-byte loads
    buf = (C.c_float * 1024)()
    ib = (C.c_int32 * 1024)()

    def call(image=base, lo=0, rows=4, n=2, c_in=8, si=buf, ii=ib, lam=0.5, k=4, so=buf, io=ib, st=None):
        return lib.ltg_topk_diversify(image, lo, rows, n, c_in, si, ii, lam, k, so, io, st, None)

    for name in ("image", "si", "ii", "so", "io"):
        assert call(**{name: None}) == -1, name
    for c_in in (0, -1, 257):
        assert call(c_in=c_in, k=1) == -1, c_in
    for k in (0, -1, 9):
        assert call(k=k) == -1, k
    for lam in (-1e-6, 1.0 + 1e-6, float("nan"), float("inf"), -float("inf")):
        assert call(lam=lam) == -1, lam
    assert call(rows=0) == -1 and call(rows=-3) == -1
    assert call(lo=-1) == -1
    assert call(n=-1) == -1
    assert call(image=base + 2) == -1                                   # not 16-byte aligned
    assert call(n=0) == 0                                               # zero rows: nothing to launch
    assert call(n=0, lam=0.0) == 0 and call(n=0, lam=1.0, c_in=256, k=256, st=buf) == 0
    assert call(n=0, k=9) == -1 and call(n=0, lam=2.0) == -1            # ... but the arguments are still checked


class _FakeEngine:
    I, I_global, device = 50, 50, "cpu"


def test_diversify_validation():
    from ltgan.serving import SlabLists
    from ltgan.trainer import Diversify, Recommender
    for lam in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            Diversify(lam)
    with pytest.raises(ValueError):
        Diversify(0.5, space="items")
    with pytest.raises(ValueError):
        Diversify(0.5, metric="l2")
    d = Diversify(0.5)
    d.bind(_FakeEngine(), 10, 20, 33)
    assert d.c == 40 and tuple(d.stat.shape) == (33, 2) and tuple(d.candidates_of(7)[1].shape) == (7, 40)
    d.bind(_FakeEngine(), 10, 200, 33)
    assert d.c == 256                                                   # min(256, 2 k)
    d = Diversify(0.25, candidates=64, space="encoder", metric="dot")
    d.bind(_FakeEngine(), 10, 64, 5)
    assert d.c == 64 and (d.space, d.metric) == ("encoder", "dot")
    lists = SlabLists(_FakeEngine(), rows=10, longest=64, parts=3)          # the all-gather buffers of three ranks: one set for every list
    assert lists.part_s.numel() == lists.part_i.numel() == 3 * 10 * 64 and lists.loc_s.numel() == lists.loc_i.numel() == 10 * 64
    for k, c in ((65, 64), (10, 257), (257, None)):
        with pytest.raises(ValueError):
            Diversify(0.5, candidates=c).bind(_FakeEngine(), 10, k, 5)
    with pytest.raises(ValueError):                                     # refused before anything of the engine is touched
        Recommender(_FakeEngine(), None, k=10, rule=object(), diversify=Diversify(0.5))


def test_cli_arguments():
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    a = rc.parse_args(["ds", "model.pt"])                                # nothing changes without the option
    assert (a.diversify, a.candidates, a.div_space, a.k, a.min_slots) == (None, None, "decoder", 100, None)
    a = rc.parse_args(["ds", "m.pt", "--diversify", "0.5"])
    assert (a.diversify, a.candidates, a.div_space) == (0.5, None, "decoder")
    a = rc.parse_args(["ds", "m.pt", "--k", "20", "--diversify", "0", "--candidates", "20", "--div-space", "encoder"])
    assert (a.diversify, a.candidates, a.div_space) == (0.0, 20, "encoder")
    a = rc.parse_args(["ds", "m.pt", "--k", "256", "--diversify", "1", "--candidates", "256"])
    assert (a.diversify, a.candidates) == (1.0, 256)
    b = lt.parse_args(["ds", "model.pt"])
    assert (b.diversify, b.candidates, b.div_space, b.k) == (None, None, "decoder", 100)
    b = lt.parse_args(["ds", "m.pt", "--k", "20", "--diversify", "0.7", "--candidates", "100"])     # lists of max(100, --k) entries
    assert (b.diversify, b.candidates) == (0.7, 100)
    bad_both = (["--diversify", "-0.1"], ["--diversify", "1.5"], ["--diversify", "nan"], ["--diversify", "x"],
                ["--diversify", "0.5", "--min-slots", "niche:5"], ["--diversify", "0.5", "--candidates", "257"],
                ["--diversify", "0.5", "--candidates", "99"], ["--candidates", "150"], ["--diversify", "0.5", "--div-space", "items"],
                ["--k", "300", "--diversify", "0.5"], ["--candidates", "150", "--min-slots", "niche:5"])
    for mod in (rc, lt):
        for bad in bad_both:
            with pytest.raises(SystemExit) as e:
                mod.parse_args(["ds", "m.pt"] + bad)
            assert e.value.code == 2, (mod.__name__, bad)
    with pytest.raises(SystemExit):
        lt.parse_args(["ds", "m.pt", "--k", "20", "--diversify", "0.5", "--candidates", "40"])      # below the list length 100
    assert rc.parse_args(["ds", "m.pt", "--k", "20", "--diversify", "0.5", "--candidates", "40"]).candidates == 40


@pytest.mark.parametrize("script,args,msg", [
    ("recommend.py", ["--k", "50", "--diversify", "0.5", "--candidates", "49"], "[k, 256] = [50, 256]"),
    ("recommend.py", ["--diversify", "0.5", "--min-slots", "niche:5"], "cannot be combined with --min-slots"),
    ("longtail.py", ["--diversify", "0.5", "--candidates", "300"], "[k, 256] = [100, 256]"),
    ("longtail.py", ["--diversify", "1.01"], "LAMBDA in [0, 1]"),
])
def test_usage_errors_through_the_scripts(script, args, msg):
    """exit status 2 before any GPU work: the dataset and the checkpoint named here do not exist"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "long-tail-gan_amd", script), "ds", "m.pt"] + args, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 2 and msg in out.stderr, out.stderr[-2000:]


def test_ils_line_from_a_hand_made_table():
    from ltgan import longtail as lt
    stats = np.array([[0.5, 0.25], [0.0, 0.0], [0.25, 0.125], [9.0, 9.0]], np.float32)
    ids = np.array([[3, 1, 2], [7, -1, -1], [4, 5, -1], [-1, -1, -1]], np.int32)      # users 1 and 3 hold fewer than two entries
    assert lt.ils_line(stats, ids, 3) == "ils@3: 0.375000 -> 0.187500"
    assert lt.ils_line(stats[1:2], ids[1:2], 100) == "ils@100: nan -> nan"


def test_reference_equals_brute_force_on_similarities_full_of_ties():
    rng = np.random.default_rng(2)
    ties = 0
    for trial in range(300):
        n = int(rng.integers(1, 14))
        k = int(rng.integers(1, 16))
        A = rng.integers(-2, 3, (n, n)) * 0.25
        S = A + A.T                                                     # symmetric, a handful of distinct values
        s = np.sort(rng.integers(0, 5, n) / 4.0)[::-1].astype(np.float32)
        for lam in (0.0, 0.25, 0.5, 1.0):
            want = D.brute_force_row(s, S, k, lam)
            for dt in (np.float32, np.float64):
                got, t = D.mmr_row(s, S, k, lam, dt, count_ties=True)
                assert got.tolist() == want, (trial, lam, dt)
            ties += t
            assert len(set(want)) == len(want) == min(k, n) and want[0] == 0
            if lam == 1.0:
                assert want == list(range(min(k, n)))                   # equal relevance: the lowest position
    assert ties > 1000, ties
    assert D.ils(np.array([[9.0, 1.0, 2.0], [1.0, 9.0, 4.0], [2.0, 4.0, 9.0]]), [0, 1, 2]) == pytest.approx(7.0 / 3.0)
    assert D.ils(np.eye(3), [2]) == 0.0 and D.ils(np.eye(3), []) == 0.0


@pytest.fixture(scope="module")
def image():
    return D.exact_image()


@pytest.mark.parametrize("c_in,k", D.EXACT_CASES)
def test_fp32_and_fp64_agree_on_the_exact_inputs(image, c_in, k):
    """the inputs of the GPU parity test: every quantity is exact in fp32, so the two evaluations take identical picks -- and the inputs
    discriminate: the lists differ from the plain top-k and the tie rule decides picks"""
    lo = 13
    sc, ids = D.exact_lists(c_in, k, image.shape[0], image_lo=lo)
    n = D.valid_counts(ids, lo, image.shape[0])
    assert n[0] == 0 and n[4] == 1 and (c_in < 3 or n[3] < c_in) and (n == c_in).any()
    S = D.exact_similarities(image, ids, lo, n)
    assert all(np.array_equal(x * 4, np.round(x * 4)) and np.abs(x).max(initial=0) <= 8 for x in S)
    moved = ties = 0
    for lam in D.EXACT_LAMBDAS:
        for r in range(sc.shape[0]):
            p32, t = D.mmr_row(sc[r, :n[r]], S[r], k, lam, np.float32, count_ties=True)
            p64 = D.mmr_row(sc[r, :n[r]], S[r], k, lam, np.float64)
            assert np.array_equal(p32, p64), (lam, r)
            if lam == 1.0:
                assert np.array_equal(p32, np.arange(min(k, n[r])))
            elif lam in (0.5, 0.75):
                moved += int(not np.array_equal(p32, np.arange(min(k, n[r]))))
                ties += t
    if (c_in, k) == (64, 20):
        assert moved >= 2 * 30 and ties >= 50, (moved, ties)
