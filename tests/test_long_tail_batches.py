"""The long-tail batch builders of helpers.py (no GPU): the batches the parity tests feed the generator must reach every threshold where the
kernels' dispatch splits.  The thresholds are read from the kernel sources, so that a changed constant fails here instead of leaving the
GPU cases quietly below it."""
import os
import re

import numpy as np
import pytest

import helpers as Hh
from test_gpu_parity import CLOCK_CASES, FWD_CASES, G_SKEWED, WARM_CASES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "long-tail-gan_amd", "csrc")


def _constant(name, fname, pattern=r"constexpr int [^;]*\b{name} = (\d+)"):
    with open(os.path.join(CSRC, fname)) as f:
        vals = {int(v) for v in re.findall(pattern.format(name=name), f.read())}
    assert len(vals) == 1, (name, fname, vals)
    return vals.pop()


NT = _constant("NT", "ltg_kernels.hip")                 # the strided row loops: a row past NT entries takes a second pass
ENC_NT = _constant("ENC_NT", "ltg_gen_fwd.h")           # fk_enc0_fwd / k_enc0_fwd: a row past ENC_NT entries takes a second chunk
G0_LIGHT = _constant("G0_LIGHT", "ltg_fast_gen.h")      # fk_enc0_grad*: an item in more rows is a heavy row (eight waves, LDS reduction)
FU = _constant("FU", "ltg_gstep.h")                     # k_row_stats_merge / k_dlogits_combine: fake pairs past FU * NT in a second batch
RD_U = _constant("RD_U", "ltg_fast_small.h")            # fk_row_dlogits: the same with RD_U


def test_the_kernel_constants_are_where_the_builders_aim():
    """LONG_TAIL_ROWS brackets NT and ENC_NT; the fake-pair builder gives a user of n entries at least n pairs"""
    assert {NT - 1, NT, NT + 1} <= set(Hh.LONG_TAIL_ROWS), NT
    assert {ENC_NT - 1, ENC_NT, ENC_NT + 1} <= set(Hh.LONG_TAIL_ROWS), ENC_NT
    assert max(Hh.LONG_TAIL_ROWS) > 2 * ENC_NT
    assert RD_U == FU


def _check_history(X, I, B):
    L = np.diff(X.indptr)
    assert X.shape == (B, I) and X.has_sorted_indices and L.min() >= 1
    for r in range(B):                                  # distinct items within a row
        assert np.all(np.diff(X.indices[X.indptr[r]:X.indptr[r + 1]]) > 0)
    n_rows_of = np.bincount(X.indices, minlength=I)
    assert n_rows_of.max() == B                         # an item in every row
    assert (n_rows_of > G0_LIGHT).sum() >= 3            # several heavy items
    assert L.max() > NT and {k for k in (NT - 1, NT, NT + 1) if k <= I} <= set(L.tolist())
    if I > ENC_NT:
        assert L.max() > ENC_NT and {ENC_NT - 1, ENC_NT, ENC_NT + 1} <= set(L.tolist())
    if I >= max(Hh.LONG_TAIL_ROWS):
        assert L.max() > 2 * ENC_NT                     # a third chunk
    assert L.max() <= I
    return L


def _check_pairs(pairs, L, I):
    rows, gen, pop = pairs
    assert len(rows) == len(gen) == len(pop) and np.all(np.diff(rows) >= 0)
    assert len(rows) > FU * NT                          # the second batch of fake-pair triples
    assert np.bincount(rows).max() > NT                 # one user past NT pairs
    assert np.all((gen >= 0) == (pop >= 0)) and 0 < (gen < 0).mean() < 0.1 and gen.max() < I and pop.max() < I
    for r in np.unique(rows):
        g = gen[(rows == r) & (gen >= 0)]
        assert len(np.unique(g)) == len(g)
    assert rows.max() < len(L)


SHAPES = sorted({(I, B, h) for I, B, _, _, h in FWD_CASES if h != "uniform"} | {(I, B, h) for _, I, B, _, h in G_SKEWED} |
                {(I, B, h) for _, I, B, _, h in WARM_CASES if h != "uniform"})


@pytest.mark.parametrize("I,B,history", SHAPES, ids=["%d-%d-%s" % s for s in SHAPES])
def test_long_tail_batches_of_the_parity_cases_reach_every_threshold(I, B, history):
    X_all, X, pairs = Hh.long_tail_batch(I, B, values=history.endswith("-values"))
    assert X_all.shape == (2 * B, I) and (X_all[B:] != X).nnz == 0
    assert X_all.indptr[B] > 0                          # batch 1: non-zero row / entry / distinct-item offsets
    L = _check_history(X, I, B)
    _check_history(X_all[:B].tocsr(), I, B)
    _check_pairs(pairs, L, I)
    vals = set(np.unique(X.data).tolist())
    if history.endswith("-values"):
        assert vals == {0.5, 1.0, 2.0, 3.0, 5.0}        # DeviceData uploads ltg_batch.values
    else:
        assert vals == {1.0}


def test_lazy_clock_batches_reach_every_threshold():
    """the skewed case of the lazy-clock test: seven G-step batches of 48 rows, a forward-only batch of 40, at 9 000 items"""
    assert ("fp32", 3, "skewed") in CLOCK_CASES and ("bf16", 5, "skewed") in CLOCK_CASES
    rng = np.random.default_rng(4242)
    I = 9000
    for _ in range(7):
        X = Hh.skewed_history(rng, 48, I)
        _check_pairs(Hh.skewed_fake_pairs(rng, X, I), _check_history(X, I, 48), I)
    _check_history(Hh.skewed_history(rng, 40, I), I, 40)   # (item 0 in all 40 rows: 40 workgroups of k_q0_touch_rows claim its row)


def test_a_length_past_the_item_count_is_dropped():
    rng = np.random.default_rng(1)
    X = Hh.skewed_history(rng, 20, 300)
    L = np.diff(X.indptr)
    assert {1, 255, 256, 257} <= set(L.tolist()) and L.max() <= 300
    X = Hh.skewed_history(rng, 3, 5000, values=True)     # fewer rows than LONG_TAIL_ROWS: the first three of them
    assert sorted(np.diff(X.indptr).tolist()) == [1, 255, 256]
