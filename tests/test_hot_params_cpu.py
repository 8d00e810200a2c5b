"""The hot parameter sets of tests/helpers.py (a trained model's dynamic range) pinned on the oracle alone: the conditions the GPU tests of
tests/test_gpu_hot_range.py rest on, at every (I, B, profile) that file uses -- and that file's stage comparators against a numpy float32
restatement of the streaming kernels' tile-by-tile online softmax merge, correct and with three planted defects."""
import functools

import numpy as np
import pytest

import helpers as Hh
from oracle import ltg_oracle as O

TINY = 1.2e-38                      # below fp32's smallest normal: exp(logit - lse) underflows on the device


def _oracle_cases():
    """every distinct (I, B, profile, quant, rng_step, is_training, seed) behind HOT_FWD, HOT_SPAN and HOT_G"""
    out = []
    for I, B, prec, _, profiles in Hh.HOT_FWD:
        out += [(I, B, p, prec == "bf16", Hh.HOT_FWD_STEP, 1.0, I + B) for p in profiles]
    I, rows, p, step = Hh.HOT_SPAN
    out += [(I, n, p, True, step + k, 0.0, 3 * I + sum(rows)) for k, n in enumerate(rows)]
    for prec, I, B, _, _ in Hh.HOT_G:
        out += [(I, B, p, prec == "bf16", Hh.HOT_G_STEP, 1.0, 11 * I + B) for p in Hh._TWO]
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def _span_problem(I, R, profile, seed):
    return Hh.hot_problem(I, R, profile, seed)


def _forward(I, B, profile, quant, step, is_training, seed):
    if is_training:
        X, P, mask, eps = Hh.hot_forward_inputs(I, B, profile, step, seed=seed)
    else:       # a batch of the span: its rows of the span's history, its own dropout counter, local row numbers
        span_I, rows, _, step0 = Hh.HOT_SPAN
        _, Xall, P = _span_problem(I, sum(rows), profile, seed)
        r0 = sum(rows[:step - step0])
        X = Xall[r0:r0 + B]
        mask, eps = Hh.dropout_mask_dense(Hh.HOT_SEED, step, B, I, Hh.HOT_KEEP), np.zeros((B, O.Z_DIM))
    return O.vae_forward(P, X.toarray(), mask, Hh.HOT_KEEP, eps, is_training, 1.0, np.float64, quant=quant)


@pytest.mark.parametrize("I,B,profile,quant,step,is_training,seed", _oracle_cases(),
                         ids=["%d-%d-%s-%s-step%d%s-seed%d" % (c[0], c[1], c[2], "bf16" if c[3] else "fp32", c[4], "" if c[5] else "-eval", c[6])
                              for c in _oracle_cases()])
def test_hot_generator_reaches_a_trained_models_range(I, B, profile, quant, step, is_training, seed):
    F = _forward(I, B, profile, quant, step, is_training, seed)
    lg, p = F["logits"], F["probs"]
    assert all(np.all(np.isfinite(F[k])) for k in ("h1", "mu", "logvar", "z", "h2", "logits", "lse", "KL_rows", "probs"))
    span = lg.max(1) - lg.min(1)
    assert span.min() >= 60.0 and span.max() <= 250.0, (span.min(), span.max())
    assert p.min() > 0.0
    tiny = float((p < TINY).mean())
    assert 1e-3 <= tiny <= 0.10, tiny
    lv = F["logvar"]
    assert lv.min() >= -8.0 and lv.max() <= 8.0 and lv.min() < -2.0 and lv.max() > 2.0, (lv.min(), lv.max())
    sat = float((np.abs(F["h2"]) > 0.99).mean())
    assert 0.05 <= sat <= 0.70, sat
    if profile != "spike-last":
        assert np.bincount(lg.argmax(1), minlength=I).max() <= 0.9 * B
    if profile == "dead-tile":      # the whole tile is 0 in fp32 against the row maximum, in every row
        d0, d1 = Hh.DEAD_TILE
        assert (lg[:, d0:d1].max(1) - lg.max(1)).max() < -104.0


D_HOT_SIZES = [(100, 150, 250, 300), (99, 150, 250, 300), (132, 150, 250, 300)]


@pytest.mark.parametrize("hs", D_HOT_SIZES + [(12, 20, 28, 16)], ids=lambda hs: "x".join(map(str, hs)))
def test_hot_discriminator_scores_and_saturation(hs):
    """400 random pairs of 500 items, dropout 0.7: |s| <= 10 for every pair, more than 1 % of the fc layer's tanh above 0.99 (at the sizes
    of config.ini's order; the 76-wide towers of the small forward-only case saturate nothing: |s| alone is pinned there)"""
    I, n, keep = 500, 400, 0.7
    rng = np.random.default_rng(hs[0])
    D = Hh.hot_discriminator(O.init_discriminator(I, *hs, seed=3))
    assert all(not D[k].any() for k in ("b1", "b2", "b3", "b4"))
    pop, nic = rng.integers(0, I, n), rng.integers(0, I, n)
    dm = Hh.d_masks(Hh.HOT_SEED, 21, n, hs[1:], keep)
    T = O.d_tower(D, pop, nic, dm, keep)
    assert np.abs(T["s"]).max() <= 10.0, np.abs(T["s"]).max()
    if hs in D_HOT_SIZES:
        assert (np.abs(T["tC"]) > 0.99).mean() > 0.01
        assert np.abs(T["s"]).max() > 4.0


# ---- the comparators against a restatement of the streaming kernels' online merge
def _online_lse(logits, defect=None):
    """csrc/ltg_stream.h's running (max, sum) over 32-item tiles in float32: mn = max(rm, max of the tile), mr = max(mn, -1e30),
    rs = rs exp(rm - mr) + sum exp(x - mr), rm = mn; the ragged last tile has I % 32 items.  defect: "no-rescale" (rs is not rescaled),
    "skip-tail" (the ragged tile is left out), "dead-as-one" (a term that underflows counts as exp(0))."""
    x = np.asarray(logits, np.float32)
    B, I = x.shape
    rm, rs = np.full(B, -np.inf, np.float32), np.zeros(B, np.float32)
    with np.errstate(under="ignore"):
        for i0 in range(0, I, 32):
            t = x[:, i0:i0 + 32]
            if defect == "skip-tail" and t.shape[1] < 32:
                continue
            mn = np.maximum(rm, t.max(1))
            mr = np.maximum(mn, np.float32(-1e30))
            e = np.exp(t - mr[:, None])
            if defect == "dead-as-one":
                e = np.where(e == 0, np.float32(1), e)
            scale = np.float32(1) if defect == "no-rescale" else np.exp(rm - mr)
            rs = (rs * scale + e.sum(1, dtype=np.float32)).astype(np.float32)
            rm = mn
    assert rs.dtype == np.float32
    return rm + np.log(rs)


@functools.lru_cache(maxsize=None)
def _hot_logits(I, profile):
    B = 24
    F = _forward(I, B, profile, True, Hh.HOT_FWD_STEP, 1.0, I + B)
    return F["logits"].astype(np.float32)


@pytest.mark.parametrize("I", [1000, 8200])
@pytest.mark.parametrize("profile", Hh.HOT_PROFILES)
def test_the_correct_online_merge_passes_the_comparators(I, profile):
    lg = _hot_logits(I, profile)
    lse = _online_lse(lg)
    err, bound, gap = Hh.check_lse(lse, lg)
    assert gap > 0.0 and bound < 1e-4           # the bound is a few fp32 ulp of an lse below 128, whatever the gap
    with np.errstate(under="ignore"):
        p = np.exp(lg - lse[:, None])
    assert p.dtype == np.float32
    assert Hh.check_probs(p, lg, lse) <= 1.0
    assert (p == 0).any() or (p < 1.2e-38).any()


@pytest.mark.parametrize("I", [1000, 8200])
@pytest.mark.parametrize("defect,profile", [("no-rescale", "ramp-up"), ("skip-tail", "spike-last"), ("dead-as-one", "dead-tile"),
                                            ("skip-tail", "dead-tile")])
def test_a_planted_defect_of_the_online_merge_fails_stage_c(I, defect, profile):
    lg = _hot_logits(I, profile)
    assert I % 32 == 8
    with pytest.raises(AssertionError, match="lse row"):
        Hh.check_lse(_online_lse(lg, defect), lg)


def test_the_probability_comparator_rejects_a_flushed_or_misscaled_value():
    lg = _hot_logits(1000, "dead-tile")
    lse = Hh.lse64(lg).astype(np.float32)
    with np.errstate(under="ignore"):
        p = np.exp(lg - lse[:, None])
    x = lg.astype(np.float64) - lse[:, None]
    flush = (x < -60.0) & (x > -69.0)           # >= 2^-100: a fast exponential that flushes here is an error, not an underflow
    assert flush.any()
    with pytest.raises(AssertionError, match="probs"):
        Hh.check_probs(np.where(flush, np.float32(0), p), lg, lse)
    with pytest.raises(AssertionError, match="probs"):
        Hh.check_probs(p * np.float32(1 + 2e-5), lg, lse)
    with pytest.raises(AssertionError, match="2\\^-100"):
        Hh.check_probs(np.where(x < -80.0, np.float32(1e-29), p), lg, lse)


def test_the_logit_comparator_is_an_accumulation_bound():
    rng = np.random.default_rng(2)
    h2 = np.tanh(rng.normal(0, 2, (8, 600))).astype(np.float32)
    W = rng.normal(0, 0.5, (600, 96)).astype(np.float32)
    b = rng.normal(0, 30, 96).astype(np.float32)
    fwd = (h2 @ W + b).astype(np.float32)       # fp32 accumulation in another order
    assert Hh.check_logits(fwd, h2, W, b) < 0.2
    with pytest.raises(AssertionError, match="logits"):
        Hh.check_logits((O.bf16_round(h2) @ W + b).astype(np.float32), h2, W, b)     # an operand rounded to bf16 is no accumulation error
