"""The noise model behind the bounds of tests/test_gpu_quantised_disc.py, on the oracle alone (tests/quantised_ref.py has the model).

* jitter = None changes no bit of O.d_tower / O.d_tower_backward (the goldens of tests/test_oracle_golden.py rest on that).
* For every forward-only tower case the oracle evaluated in float32 -- an independent realisation of the same noise: other accumulation
  order, other tanh, none of the model's Gaussian draws -- lies inside 4 x the jitter floor, maximum and median.  Floors (fp64 oracle,
  3 draws; max |dy| / median |dy| over the valid slots; "hot": Hh.hot_discriminator), as this file prints them:
      bf16  100x150x250x300 9.9e-5 / 1.9e-7 (hot 5.2e-4 / 2.9e-7)   2048x1024x512x256 2.3e-4 / 4.8e-7 (hot 7.3e-4 / 1.6e-7)
            192x64x128x128 6.9e-5 / 1.2e-7   256x128x128x100 5.9e-5 / 1.2e-7   512x256x256x640 1.9e-4 / 3.8e-7   99x151x250x301 1.0e-4 / 1.9e-7
            12x20x28x16 3.6e-7 / 1.1e-8
      fp8   100x150x250x300 3.4e-3 / 7.7e-6 (hot 1.8e-2 / 1.3e-5)   2048x1024x512x256 3.7e-3 / 7.3e-5 (hot 1.6e-2 / 1.2e-5)
            192x64x128x128 1.1e-3 / 4.0e-6   256x128x128x100 1.9e-3 / 3.8e-6   512x256x256x640 5.8e-3 / 1.7e-5   99x151x250x301 1.4e-3 / 9.4e-6
            12x20x28x16 2.7e-5 / 3.9e-7
  The float32 oracle is 5e-8 .. 1.1e-4 (max) and 1.5e-8 .. 4.4e-8 (median) off the fp64 one: the smallest case's median bound, 4.4e-8, is
  three times the 1.5e-8 that rounding y itself to float32 costs.
"""
import numpy as np
import pytest

import quantised_ref as Q
from oracle import ltg_oracle as O

CASES = [(hs, segs, mode, hot) for hs, segs in Q.TOWER_CASES for mode in ("bf16", "fp8") for hot in (False, True) if not hot or (hs, segs) in Q.TOWER_HOT]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("mode", [None, "bf16", "fp8"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jitter_none_changes_no_bit(mode, dtype):
    """jitter = None against jitter = (rng, 0.0) -- a multiplication by exactly 1 -- and against the call without the argument: the same
    bits in every intermediate and every gradient; and a non-zero rel does move them"""
    hs = (20, 24, 40, 36)
    c = Q.d_case(40, 33, hs)
    dm = Q.Hh.d_masks(Q.SEED, 3, 40, hs[1:], 0.7)
    ids = (np.maximum(c["rp"], 0), np.maximum(c["rn"], 0))
    T0 = O.d_tower(c["D"], *ids, dm, 0.7, dtype, mode)
    g0 = O.d_tower_backward(c["D"], T0, dm, 0.7, T0["y"], dtype, mode)
    for jit in (None, (np.random.default_rng(0), 0.0)):
        T = O.d_tower(c["D"], *ids, dm, 0.7, dtype, mode, jitter=jit)
        g = O.d_tower_backward(c["D"], T, dm, 0.7, T["y"], dtype, mode, jitter=jit)
        for k in T0:
            assert T[k].dtype == T0[k].dtype and np.array_equal(_bits(T[k]), _bits(T0[k])), k
        for k in g0:
            assert g[k].dtype == g0[k].dtype and np.array_equal(_bits(g[k]), _bits(g0[k])), k
    Tj = O.d_tower(c["D"], *ids, dm, 0.7, dtype, mode, jitter=(np.random.default_rng(0), 1e-3))
    gj = O.d_tower_backward(c["D"], T0, dm, 0.7, T0["y"], dtype, mode, jitter=(np.random.default_rng(0), 1e-3))
    assert 1e-6 < np.abs(Tj["y"] - T0["y"]).max() < 1e-1
    assert all(1e-5 < Q.energy(gj[k], g0[k]) < 1e-1 for k in ("w1", "b1", "w2", "b2", "w3", "b3")), {k: Q.energy(gj[k], g0[k]) for k in gj}
    assert np.array_equal(gj["w4"], g0["w4"]) and np.array_equal(gj["b4"], g0["b4"])        # (the output layer is no quantised GEMM)


@pytest.mark.parametrize("hs,segs,mode,hot", CASES, ids=["%s-%s%s" % (Q.case_id(hs), m, "-hot" if h else "") for hs, segs, m, h in CASES])
def test_float32_oracle_lies_inside_the_tower_bound(hs, segs, mode, hot):
    c = Q.tower_case(hs, segs, hot=hot)
    y, valid = Q.tower_oracle(c, mode)
    fmax, fmed = Q.tower_floor(c, mode, y, valid)
    y32, _ = Q.tower_oracle(c, mode, dtype=np.float32)
    emax, emed = Q.y_figures(y32, y, valid)
    y_fp32 = Q.tower_oracle(c, None)[0]
    print("tower %s %s%s: floor max / median %.2e / %.2e; float32 oracle %.2e / %.2e; share of slots off by > 1e-5: %.3f; |y - fp32 tower| max %.2e" % (
        hs, mode, " hot" if hot else "", fmax, fmed, emax, emed, float((np.abs(y32 - y)[valid] > 1e-5).mean()), float(np.abs(y - y_fp32)[valid].max())))
    assert np.all(y32[~valid] == 0.0)
    assert emax <= Q.FACTOR * fmax and emed <= Q.FACTOR * fmed


def test_clamp_case_really_clamps():
    """the forward-only clamp case of the GPU file (embeddings x 10): the oracle's scaled embedding operand passes 448, and its conversion
    saturates there"""
    c = Q.tower_case((256, 128, 128, 128), (129,), emb_scale=10.0)
    e = np.asarray(c["D"]["emb"], np.float64) * float(1 << O.FP8_S["emb"])
    assert np.abs(e).max() > 448.0 and float((np.abs(e) > 448.0).mean()) > 0.02      # (truncated normal: 0.2 x 10 x 2^8 = 512 at most)
    assert np.abs(O.fp8_e4m3_round(e)).max() == 448.0


def test_e4m3_table_is_the_rounding_model_s_range():
    t = Q.e4m3_table()
    fin = t[np.isfinite(t)]
    assert fin.size == 254 and fin.max() == 448.0 and np.min(np.abs(fin[fin != 0])) == 2.0 ** -9
    assert np.array_equal(O.fp8_e4m3_round(fin), fin)                       # every e4m3 value is a fixed point of the model
    x = np.random.default_rng(0).normal(0, 30, 4000)
    assert np.all(np.isin(O.fp8_e4m3_round(x), fin))
