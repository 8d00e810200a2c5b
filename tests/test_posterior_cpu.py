"""Posterior-aware scores without a GPU: the reference (tests/posterior_ref.py) against its own definition, the fixture property the
GPU tests rely on, the bound's arithmetic, the entry points' types and refusals (every one returns before a HIP call), the arguments of
serving.Posterior and the two CLI parsers."""
import ctypes as C
import os

import numpy as np
import pytest

import posterior_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(fx):
    img, _, _ = R.h2_image(fx["mulv"], fx["eps"], fx["W_p0"], fx["b_p0"])
    return img


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -0.3, 0.0, 3.0e-5, 1.0 + 2.0 ** -8 + 2.0 ** -20], np.float32)
    got = R.bf16_round(x)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == np.float32(1.0 + 2.0 ** -6) and got[3] == np.float32(1.0 + 2.0 ** -7)   # ties to even
    assert got[7] == np.float32(1.0 + 2.0 ** -7)                                                       # above the tie: up
    assert (np.abs(got.astype(np.float64) - x) <= 2.0 ** -8 * np.abs(x)).all()                       # half an ulp of 8 significant bits
    bits = (got.view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(R.bf16_bits_to_float(bits), got) and np.array_equal(R.bf16_bits_to_float(bits.view(np.int16)), got)


def test_degenerate_posterior_and_single_sample():
    fx = R.fixture(5, 64, 8, seed=3)
    mulv = fx["mulv"].copy()
    mulv[:, R.Z:] = -200.0                                                   # exp(-100) eps vanishes against mu
    img, _, z = R.h2_image(mulv, fx["eps"], fx["W_p0"], fx["b_p0"])
    assert np.array_equal(z.reshape(5, 8, R.Z)[:, 0], z.reshape(5, 8, R.Z)[:, 7])
    score, mean, std = R.scores(img, fx["W_bf16"], fx["b_p1"], 8, 1.5)
    one = R.sample_logits(img[::8], fx["W_bf16"], fx["b_p1"], 1)[:, 0]       # the single-sample logit
    assert (std == 0).all() and np.allclose(mean, one, rtol=0, atol=1e-12) and np.array_equal(score, mean)
    # S = 1 equals one sample, std 0
    img1 = _image(fx)[::8]
    s1, m1, d1 = R.scores(img1, fx["W_bf16"], fx["b_p1"], 1, 0.0)
    assert (d1 == 0).all() and np.array_equal(s1, m1) and np.array_equal(m1, R.sample_logits(img1, fx["W_bf16"], fx["b_p1"], 1)[:, 0])


@pytest.mark.parametrize("S", [4, 16])
def test_scores_equal_the_brute_force_loop(S):
    fx = R.fixture(3, 7, S, seed=11)
    img = _image(fx)
    for beta in (0.0, 1.5, -1.0):
        a, b = R.scores(img, fx["W_bf16"], fx["b_p1"], S, beta), R.brute_scores(img, fx["W_bf16"], fx["b_p1"], S, beta)
        for x, y in zip(a, b):
            assert np.abs(x - y).max() <= 1e-12
    sc, mean, std = R.scores(img, fx["W_bf16"], fx["b_p1"], S, 1.5)
    assert (std > 0).all() and np.array_equal(sc, mean + 1.5 * std)


def test_bound_is_the_derived_expression():
    fx = R.fixture(2, 9, 4, seed=5)
    img = _image(fx)
    A = R.magnitude(img, fx["W_bf16"], fx["b_p1"], 4)
    l = R.sample_logits(img, fx["W_bf16"], fx["b_p1"], 4)
    assert A.shape == (2, 9) and (A >= np.abs(l).max(1)).all()
    assert np.array_equal(R.bound(img, fx["W_bf16"], fx["b_p1"], 4), 2.0 * (608 + 4 + 2) * 2.0 ** -24 * A)


@pytest.mark.parametrize("I", [1000, 1003])
@pytest.mark.parametrize("S", [4, 8, 16, 32])
def test_fixture_property_std_far_above_the_bound(S, I):
    """what the GPU tests rely on: on the shared fixture at least 99 % of the (row, item) cells have a reference std of 50 tol or more,
    so a wrong grouping of the sample rows cannot hide under the bound"""
    fx = R.fixture(37, I, S)
    img = _image(fx)
    _, _, std = R.scores(img, fx["W_bf16"], fx["b_p1"], S, 0.0)
    tol = R.bound(img, fx["W_bf16"], fx["b_p1"], S)
    share = float((std >= 50 * tol).mean())
    print("S %d, I %d: share of cells with std >= 50 tol %.4f, median std / tol %.0f" % (S, I, share, float(np.median(std / tol))))
    assert share >= 0.99


def _cfg(cabi, n_items=1000, h=600, z=200, item_lo=0, n_glob=0, prec=0):
    return cabi.ltg_config(n_items, h, z, n_items, 100, 150, 250, 300, prec, 0, item_lo, n_glob, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


def test_entry_points_are_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    cfg, gen = C.POINTER(cabi.ltg_config), C.POINTER(cabi.ltg_gen_state)
    want = {"ltg_posterior_ld": (i32, [cfg]),
            "ltg_posterior_image_bytes": (C.c_size_t, [cfg, i32, i32]),
            "ltg_posterior_h2": (C.c_int, [cfg, gen, vp, i32, i32, i32, C.c_uint64, vp, vp, vp, vp]),
            "ltg_posterior_scores": (C.c_int, [cfg, gen, vp, i32, i32, f32, vp, vp, vp]),
            "ltg_posterior_entries": (C.c_int, [cfg, gen, vp, i32, i32, vp, i32, vp, vp, vp]),
            "ltg_row_lse": (C.c_int, [cfg, vp, i32, vp, vp])}
    for name, (res, args) in want.items():
        assert cabi.SYMBOLS[name] == (res, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_POST_MAX_SAMPLES 32" in header and "bf16 WHATEVER cfg->precision is" in header
    rng_h = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_rng.h")).read()
    assert "#define LTG_STREAM_POSTERIOR_EPS 9" in rng_h and R.STREAM_POSTERIOR_EPS == 9
    hip = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_kernels.hip")).read()
    assert hip.index('#include "ltg_explore.h"') < hip.index('#include "ltg_posterior.h"')


def test_sizes_and_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    good = _cfg(cabi)
    assert lib.ltg_posterior_ld(C.byref(good)) == 608 and lib.ltg_posterior_ld(C.byref(_cfg(cabi, h=64))) == 64
    assert lib.ltg_posterior_ld(C.byref(_cfg(cabi, h=68))) == 96 and lib.ltg_posterior_ld(None) == 0
    assert lib.ltg_posterior_image_bytes(C.byref(good), 37, 16) == 37 * 16 * 608 * 2
    for rows, s in ((37, 2), (37, 0), (37, 64), (-1, 4), (2 ** 30, 4)):
        assert lib.ltg_posterior_image_bytes(C.byref(good), rows, s) == 0
    assert lib.ltg_posterior_image_bytes(C.byref(_cfg(cabi, 0)), 4, 4) == 0 and lib.ltg_posterior_image_bytes(None, 4, 4) == 0
    fb = (C.c_float * 1024)()
    ib = (C.c_int32 * 64)()
    img = (C.c_uint16 * 4096)()
    buf = C.addressof(img) + (-C.addressof(img)) % 16                        # a 16-byte aligned host address: never dereferenced
    gen = cabi.ltg_gen_state()
    for i in (2, 3, 6, 7):
        gen.p[i] = C.addressof(fb)

    def h2(cfg=good, g=gen, mulv=fb, n=2, row_lo=0, s=4, draw=0, eps=None, out=buf, z=None):
        return lib.ltg_posterior_h2(C.byref(cfg) if cfg is not None else None, C.byref(g) if g is not None else None, mulv, n, row_lo, s, draw,
                                    eps, out, z, None)

    def sc(cfg=good, g=gen, image=buf, n=2, s=4, beta=1.0, out=fb, spread=None):
        return lib.ltg_posterior_scores(C.byref(cfg) if cfg is not None else None, C.byref(g) if g is not None else None, image, n, s, beta,
                                        out, spread, None)

    def en(cfg=good, g=gen, image=buf, n=2, s=4, ids=ib, k=4, mean=fb, std=fb):
        return lib.ltg_posterior_entries(C.byref(cfg) if cfg is not None else None, C.byref(g) if g is not None else None, image, n, s, ids, k,
                                         mean, std, None)

    def lse(cfg=good, logits=fb, n=2, out=fb):
        return lib.ltg_row_lse(C.byref(cfg) if cfg is not None else None, logits, n, out, None)

    # zero rows: nothing is launched, the arguments are still checked
    assert h2(n=0) == 0 and sc(n=0) == 0 and en(n=0) == 0 and lse(n=0) == 0
    assert h2(n=0, eps=fb, z=fb, draw=2 ** 64 - 1, row_lo=2 ** 31 - 1, s=32) == 0 and sc(n=0, spread=fb, beta=-2.0) == 0 and sc(n=0, s=1, beta=0.0) == 0
    for call in (h2, sc, en):
        for s in (0, 2, 3, 5, 64, -4):
            assert call(s=s) == -1 and call(n=0, s=s) == -1, (call.__name__, s)
        assert call(cfg=None) == -1 and call(g=None) == -1 and call(n=-1) == -1 and call(n=2 ** 30) == -1
        assert call(cfg=_cfg(cabi, 0)) == -1 and call(cfg=_cfg(cabi, h=602)) == -1 and call(cfg=_cfg(cabi, prec=2)) == -1
    assert lse(cfg=None) == -1 and lse(logits=None) == -1 and lse(out=None) == -1 and lse(n=-1) == -1 and lse(cfg=_cfg(cabi, 0)) == -1
    assert h2(mulv=None) == -1 and h2(out=None) == -1 and h2(row_lo=-1) == -1 and h2(n=0, row_lo=-1) == -1
    assert h2(cfg=_cfg(cabi, z=4096), s=8) == -1                             # the samples of z would not fit the LDS
    no_p0 = cabi.ltg_gen_state()
    no_p0.p[6] = C.addressof(fb)
    assert h2(g=no_p0) == -1
    for beta in (float("inf"), -float("inf"), float("nan")):
        assert sc(beta=beta) == -1 and sc(n=0, beta=beta) == -1
    assert sc(s=1, beta=0.5) == -1 and sc(n=0, s=1, beta=-1.0) == -1 and sc(image=None) == -1 and sc(out=None) == -1
    assert sc(image=buf + 2) == -1                                           # not 16-byte aligned
    no_p1 = cabi.ltg_gen_state()
    no_p1.p[7] = C.addressof(fb)
    assert sc(g=no_p1) == -1 and en(g=no_p1) == -1
    assert sc(cfg=_cfg(cabi, 1000, item_lo=-1)) == -1
    for k in (0, -1, 1025):
        assert en(k=k) == -1 and en(n=0, k=k) == -1
    assert en(ids=None) == -1 and en(mean=None) == -1 and en(std=None) == -1 and en(image=None) == -1


def test_posterior_arguments():
    from ltgan.serving import POSTERIOR_IMAGE_BYTES, POSTERIOR_SAMPLES, Posterior, Rule
    from ltgan.sharded import Posterior as ShardedPosterior
    from ltgan.trainer import Posterior as TrainerPosterior
    from ltgan import longtail as lt
    assert Posterior is ShardedPosterior is TrainerPosterior and not issubclass(Posterior, Rule)
    assert POSTERIOR_IMAGE_BYTES == 256 << 20 and POSTERIOR_SAMPLES == R.SAMPLES == lt.POSTERIOR_SAMPLES
    p = Posterior()
    assert (p.samples, p.beta, p.draw, p.want_entries, p.want_stats) == (16, 1.0, 0, True, False)
    assert Posterior(samples=1, beta=0.0, draw=2 ** 64 - 1).samples == 1 and Posterior(beta=-2, entries=False).want_entries is False
    assert Posterior(entries=False, stats=True).want_entries is True         # the statistics read the entry tables
    for bad in (dict(samples=2), dict(samples=0), dict(samples=64), dict(samples=4.5), dict(beta=float("nan")), dict(beta=float("inf")),
                dict(beta=1e39), dict(samples=1, beta=0.1), dict(samples=1), dict(draw=-1), dict(draw=2 ** 64), dict(draw=0.5)):
        with pytest.raises(ValueError):
            Posterior(**bad)
    with pytest.raises(ValueError):
        Posterior(entries=False).table()
    with pytest.raises(ValueError):
        Posterior().stats()


def test_cli_parsers():
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    a = rc.parse_args(["d", "c", "--posterior", "1.5"])
    assert (a.posterior, a.posterior_samples, a.posterior_draw, a.uncertainty) == (1.5, None, None, "unc.tsv")
    a = rc.parse_args(["d", "c", "--posterior", "-1", "--posterior-samples", "32", "--posterior-draw", "7", "--uncertainty", "u.tsv",
                       "--explore", "0.5"])                                 # it composes with a rule
    assert (a.posterior, a.posterior_samples, a.posterior_draw, a.uncertainty, a.explore) == (-1.0, 32, 7, "u.tsv", 0.5)
    a = lt.parse_args(["d", "c", "--posterior", "0", "--posterior-samples", "1", "--min-slots", "niche:10"])
    assert a.posterior == 0.0 and a.posterior_samples == 1 and a.slots is not None
    assert rc.parse_args(["d", "c"]).posterior is None and rc.parse_args(["d", "c"]).uncertainty is None
    for mod in (rc, lt):
        for bad in (["--posterior", "nan"], ["--posterior", "inf"], ["--posterior", "1e39"], ["--posterior", "1", "--posterior-samples", "3"],
                    ["--posterior", "1", "--posterior-samples", "1"], ["--posterior", "1", "--posterior-draw", "-1"], ["--posterior-samples", "8"],
                    ["--posterior-draw", "1"], ["--posterior"]):
            with pytest.raises(SystemExit):
                mod.parse_args(["d", "c"] + bad)
    with pytest.raises(SystemExit):
        rc.parse_args(["d", "c", "--uncertainty", "u.tsv"])


def test_cli_writers(tmp_path):
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    ids = np.array([[3, 1, -1], [0, 2, 4]], np.int32)
    mean = np.array([[1.5, -0.25, 0.0], [0.125, 2.0, -3.0]], np.float32)
    std = np.array([[0.5, 0.25, 0.0], [0.0, 1.0, 0.75]], np.float32)
    path = str(tmp_path / "unc.tsv")
    assert rc.write_uncertainty(mean, std, ids, 10, path) == 2
    assert open(path).read() == "10\t3:1.5:0.5,1:-0.25:0.25\n11\t0:0.125:0,2:2:1,4:-3:0.75\n"

    class Tab:
        def table(self):
            return mean, std
    lines = lt.posterior_group_lines(Tab(), ids, np.array([0, 1, 0, 1, 2], np.uint8), ["popular", "niche"])
    assert lines == ["posterior_std\tpopular\t2\t0.500000", "posterior_std\tniche\t2\t0.375000"]     # (item 4 is in no group)
    npz = str(tmp_path / "r.npz")
    rc.write_recs(ids, mean, 10, None, npz, posterior=(mean, std))
    z = np.load(npz)
    assert np.array_equal(z["post_mean"], mean) and np.array_equal(z["post_std"], std)
