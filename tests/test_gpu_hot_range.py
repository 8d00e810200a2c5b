"""The HIP kernels against the fp64 oracle at a trained model's dynamic range (Hh.hot_generator / Hh.hot_discriminator; what those sets give
is pinned on the oracle alone by tests/test_hot_params_cpu.py).  Every other parity test starts from the Xavier initialiser: logits within
+-2 of a row, no tanh above 0.99, every rescale exp(m_old - m_new) of the online softmax about 1.  Here rows span 60 .. 250, whole tiles
underflow against the row maximum, a quarter of h2 is saturated.

The forward is checked STAGE BY STAGE, each stage against the fp64 evaluation of what the device itself produced in the stage before: with
hot parameters the oracle at float32 is 1e-3 off the oracle at float64 on probabilities end to end (a probability's relative error is the
absolute error of logit - lse, and the logits reach a hundred), so north_star's end-to-end 1e-3 says nothing about a kernel here.
Bounds: (a) test_forward_parity's; (b), (d) derived in Hh.logits_ratio / Hh.probs_ratio; (c) measured against the float32 oracle per
case (Hh.lse_bound).  DESIGN.md section 6 has the measured errors beside them."""
import functools

import numpy as np
import pytest

import helpers as Hh
import test_gpu_parity as TP
from oracle import ltg_oracle as O

pytestmark = pytest.mark.gpu

SEED = Hh.HOT_SEED
assert SEED == TP.SEED


@functools.lru_cache(maxsize=2)
def _forward_reference(I, B, profile):
    """the inputs of a forward case and the oracle's middle layers (the same for both decoder precisions)"""
    X, P, mask, eps = Hh.hot_forward_inputs(I, B, profile)
    F = O.vae_forward(P, X.toarray(), mask, Hh.HOT_KEEP, eps, 1.0, 1.0, np.float64)
    return X, P, {k: F[k] for k in ("h1", "mu", "logvar", "z", "h2", "KL_rows")}


def _stage_a(got, F, tag):
    """h1, mulv, z, h2 at test_forward_parity's bounds; kl_rows to 1e-4 of the largest row (the rows are in the hundreds)"""
    fig = {"h1": Hh.rel_err(got["h1"], F["h1"]) / 2e-5}
    if "mu" in F:
        fig["mulv"] = Hh.rel_err(got["mulv"], np.concatenate([F["mu"], F["logvar"]], 1)) / 1e-4
        fig["z"] = Hh.rel_err(got["z"], F["z"]) / 1e-4
        fig["kl"] = float(np.abs(got["kl_rows"] - F["KL_rows"]).max() / (1e-4 * np.abs(F["KL_rows"]).max()))
    fig["h2"] = Hh.rel_err(got["h2"], F["h2"]) / 1e-4
    return fig


def _stages_bcd(precision, got, probs, P):
    """(b) logits from the device's h2, (c) lse from the device's logits, (d) probabilities from the device's logits and lse"""
    bf = precision == "bf16"
    h2 = O.bf16_round(got["h2"]) if bf else got["h2"]
    W = O.bf16_round(P["Wp1"]) if bf else P["Wp1"]
    fig = {"logits": Hh.logits_ratio(got["logits"], h2, W, P["bp1"])[0]}
    r, row, err, bound, gap = Hh.lse_ratio(got["lse"], got["logits"])
    fig.update(lse=r, lse_err=err, lse_bound=bound, lse_gap=gap)
    r, at, small_ok = Hh.probs_ratio(probs, got["logits"], got["lse"])
    fig.update(probs=r, probs_small_ok=small_ok)
    return fig


def _assert_figures(fig, tag):
    """every figure is error / bound; printed before the first assertion"""
    print("hot forward %s: " % (tag,) + " ".join("%s %.3g" % kv for kv in fig.items()))
    assert fig.pop("probs_small_ok"), (tag, "a probability below 2^-100 is negative or above 2^-99")
    for k in ("h1", "mulv", "z", "h2", "kl", "logits", "lse", "probs"):
        if k in fig:
            assert fig[k] <= 1.0, (tag, k, fig)


FWD = sorted((I, B, profile, precision, knob) for I, B, precision, knob, profiles in Hh.HOT_FWD for profile in profiles)


@pytest.mark.parametrize("I,B,profile,precision,knob", FWD,
                         ids=["%d-%d-%s-%s%s" % (I, B, pf, pr, "-bit%d" % (k.bit_length() - 1) if k else "") for I, B, pf, pr, k in FWD])
def test_hot_forward_stage_by_stage(I, B, profile, precision, knob):
    """I = 1 000: small slab; bit 18: the generic kernels; 4 096: the largest small slab; 6 000: middle-layer fast path without streaming;
    8 200: the first streaming form with a ragged tail (150 rows: eight batch tiles); 25 032: 7 segments of 4 096; bit 17: the second
    streaming form forced; 65 544: the second form chosen by the library."""
    import torch
    X, P, F = _forward_reference(I, B, profile)
    eng = TP._engine(I, precision)
    eng.cfg.tuning = knob
    eng.set_generator(Hh.gen_to_engine(P))
    acts = eng.new_acts(B)
    batch = TP._upload_batch(eng, X)
    probs = torch.empty(B, I, dtype=torch.float32, device=eng.device)
    eng.forward(batch, acts, keep_prob=Hh.HOT_KEEP, is_training=1.0, rng_step=Hh.HOT_FWD_STEP, probs_out=probs)
    torch.cuda.synchronize()
    got = {k: getattr(acts, k).cpu().numpy() for k in ("h1", "mulv", "z", "h2", "logits", "lse", "kl_rows")}
    fig = _stage_a(got, F, profile)
    fig.update(_stages_bcd(precision, got, probs.cpu().numpy(), P))
    _assert_figures(fig, (I, B, profile, precision, knob))


def test_hot_forward_over_a_span_of_batches():
    """ltg_fwd_opts.rows_per_step at 8 200 items x (100, 100, 50) rows (is_training = 0, as the trainer issues it): batch k draws its
    dropout with counter rng_step + k and its local row numbers; the stages as above, (a) batch by batch"""
    import torch
    I, rows, profile, step = Hh.HOT_SPAN
    R = sum(rows)
    _, X, P = Hh.hot_problem(I, R, profile, 3 * I + R)
    eng = TP._engine(I, "bf16")
    eng.set_generator(Hh.gen_to_engine(P))
    acts = eng.new_acts(R)
    batch = TP._upload_batch(eng, X)
    probs = torch.empty(R, I, dtype=torch.float32, device=eng.device)
    eng.forward(batch, acts, keep_prob=Hh.HOT_KEEP, is_training=0.0, rng_step=step, probs_out=probs, rows_per_step=rows[0])
    torch.cuda.synchronize()
    got = {k: getattr(acts, k).cpu().numpy() for k in ("h1", "h2", "logits", "lse")}
    fig, r0 = {}, 0
    for k, n in enumerate(rows):
        mask = Hh.dropout_mask_dense(SEED, step + k, n, I, Hh.HOT_KEEP)
        F = O.vae_forward(P, X[r0:r0 + n].toarray(), mask, Hh.HOT_KEEP, np.zeros((n, eng.Z)), 0.0, 1.0, np.float64)
        for key, v in _stage_a({"h1": got["h1"][r0:r0 + n], "h2": got["h2"][r0:r0 + n]}, {"h1": F["h1"], "h2": F["h2"]}, k).items():
            fig[key] = max(fig.get(key, 0.0), v)
        r0 += n
    fig.update(_stages_bcd("bf16", got, probs.cpu().numpy(), P))
    _assert_figures(fig, (I, rows, profile))


# ---- ltg_rowstats_combine on injected partials: all three forms of ltg_rank_terms (R = 1, R <= 8, R > 8)
def _combine_reference(part):
    """(lse in fp64, its bound) of partials [R][B][5] = (max, sum exp, ., ., .): 2 ulp of the lse (its own rounding and logf's) plus stage
    (c)'s bound -- 8 x the gap between this merge evaluated at float32 and at float64, never below 2 ulp"""
    m, s = part[:, :, 0].astype(np.float64), part[:, :, 1].astype(np.float64)
    M = m.max(0)
    want = M + np.log((s * np.exp(m - M)).sum(0))
    m32, s32 = part[:, :, 0], part[:, :, 1]
    M32 = m32.max(0)
    with np.errstate(under="ignore"):
        l32 = M32 + np.log((s32 * np.exp(m32 - M32)).sum(0, dtype=np.float32))
    assert l32.dtype == np.float32
    gap = float(np.abs(l32 - want).max())
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return want, 2.0 * ulp + np.maximum(8.0 * gap, 2.0 * ulp)


@pytest.mark.parametrize("B", [1, 64, 257])
@pytest.mark.parametrize("R", [1, 2, 8, 9])
def test_rowstats_combine_on_injected_partials(R, B):
    """the ranks' maxima differ by 0, 60 and 160 (at 160 a rank's whole sum underflows against the maximum: exp(-160) = 0 in fp32), the
    largest on the first rank, on the last and in the middle; a third rank half way down where there is one"""
    import torch
    eng = TP._engine(1000, "bf16")
    rng = np.random.default_rng(100 * R + B)
    worst = 0.0
    for diff in (0.0, 60.0, 160.0):
        for top in sorted({0, R - 1, R // 2}):
            part = np.zeros((R, B, 5), np.float32)
            m0 = rng.uniform(-40.0, 120.0, B)
            part[:, :, 0] = m0 - diff
            if R > 2:
                part[(top + 1) % R, :, 0] = m0 - diff / 2
            part[top, :, 0] = m0
            part[:, :, 1] = rng.uniform(1.0, 4096.0, (R, B))          # a segment's sum of exp(x - max): 1 .. its item count
            part[:, :, 2] = rng.normal(0, 50, (R, B))
            part[:, :, 3] = part[:, :, 1] * rng.uniform(0, 1e-2, (R, B))
            part[:, :, 4] = rng.integers(1, 40, (R, B))
            lse = torch.full((B,), float("nan"), dtype=torch.float32, device=eng.device)
            eng.rowstats_combine(torch.from_numpy(part).to(eng.device), R, B, lse)
            torch.cuda.synchronize()
            want, bound = _combine_reference(part)
            got = lse.cpu().numpy().astype(np.float64)
            assert np.all(np.isfinite(got)), (diff, top)
            ratio = float((np.abs(got - want) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (R, B, diff, top, ratio)
    print("rowstats_combine R=%d B=%d: worst error / bound %.3g" % (R, B, worst))


# ---- G step: test_g_step_parity's case and bounds with hot generator and discriminator
G_HOT = [c + (p,) for c in Hh.HOT_G for p in Hh._TWO]
# The one cold case that passes test_g_step_parity's bf16 bounds (first moments 2e-3, second 4e-3 of the tensor's largest): dlogits are rounded
# to bf16 before the two products that consume them, and with a dead tile and rows spanning 200 the values near a rounding boundary move the
# sums by more than that -- in the ORACLE too: float32 against float64 on this case's inputs (quant = True, CPU, the reference alone) differ by
# 3.88e-3 on the first moments (bp1) and 4.20e-3 on the second; the device is 2.36e-3 off the fp64 oracle (W_p1).  So the Xavier regime's
# bound, not the kernel: 4 x the oracle's own gap for this case.
G_HOT_TOL = {("bf16", 8200, 100, "step", False, "dead-tile"): (4 * 3.88e-3, 4 * 4.20e-3)}


@pytest.mark.parametrize("precision,I,B,path,warm,profile", G_HOT,
                         ids=["%s-%d-%d-%s%s-%s" % (pr, I, B, path, "-warm" if w else "", pf) for pr, I, B, path, w, pf in G_HOT])
def test_hot_g_step(precision, I, B, path, warm, profile):
    """every fourth user's fake pairs include item I - 3 (the spike), an item of the dead tile and item 5: P_b and sum_p then hold a
    probability near 1 and ones that are 0 in fp32"""
    P = Hh.hot_problem(I, B, profile, 11 * I + B)[2]
    D = Hh.hot_discriminator(O.init_discriminator(I, *TP.G_D, seed=5))
    fig = {}
    try:
        TP._g_step_case(precision, I, B, path, warm, hs=TP.G_D, P=P, D=D, pairs=Hh.hot_fake_pairs, tol=G_HOT_TOL.get((precision, I, B, path, warm, profile)),
                        figures=fig)
    finally:
        if fig:
            print("hot G step %s %d %d %s %s: worst first / second moment rel err %.2e / %.2e" % (
                precision, I, B, path, profile, max(v[0] for v in fig.values()), max(v[1] for v in fig.values())))


# ---- D step and forward-only tower with the hot discriminator
D_HOT = [(900, 950, TP.CONFIG_D), (33, 7, TP.CONFIG_D), (700, 650, (99, 150, 250, 300)), (700, 650, (132, 150, 250, 300))]


def _hot_d(hs, I=500, seed=3):
    return Hh.hot_discriminator(O.init_discriminator(I, *hs, seed=seed))


@pytest.mark.parametrize("d_arith", ["fp32", "bf16x6"])
@pytest.mark.parametrize("nr,nf,hs", D_HOT, ids=TP._d_case_ids(D_HOT))
def test_hot_d_step(nr, nf, hs, d_arith):
    """config.ini's sizes; (99, ...): the generic kernels; (132, ...): the fast path past the one-kernel tower's h0 limit -- test_d_step_parity's bounds"""
    TP._d_step_case(nr, nf, warm=False, d_arith=d_arith, hs=hs, D=_hot_d(hs))


def test_hot_d_step_from_warm_moments():
    TP._d_step_case(900, 950, warm=True, d_arith="bf16x6", hs=TP.CONFIG_D, D=_hot_d(TP.CONFIG_D))


@pytest.mark.parametrize("d_arith", ["bf16x6", "fp32"])
@pytest.mark.parametrize("hs,segs", [((100, 150, 250, 300), (1, 63, 64, 65, 700)), ((12, 20, 28, 16), (5, 130))])
def test_hot_forward_only_tower(hs, segs, d_arith):
    """ltg_fake_tower_batched through the one-kernel tower (bf16x6) and the three-launch tower (fp32): y of every slot against O.d_tower,
    segment by segment, at test_forward_only_tower_matches_oracle's 2e-6 for either arithmetic"""
    import torch
    from ltgan.engine import Pairs
    I, keep = 400, 0.7
    rng = np.random.default_rng(sum(segs) + hs[0])
    D = _hot_d(hs, I, seed=11)
    n = sum(segs)
    pop, nic = rng.integers(0, I, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    hole = rng.random(n) < 0.04
    pop[hole] = -1
    nic[hole] = -1
    row0 = np.concatenate([[0], np.cumsum(segs)[:-1]]).astype(np.int32)
    seg_of = np.repeat(np.arange(len(segs), dtype=np.int32), segs)
    steps = (1000 + 7 * np.arange(len(segs))).astype(np.int64)
    eng = TP._engine(I, "fp32", hs=hs, lr=1e-3, d_arith=d_arith)
    emb, darr = Hh.disc_to_engine(D)
    eng.set_discriminator(emb, darr)
    t = lambda a: torch.from_numpy(a).to(eng.device)
    y = torch.full((n,), -1.0, dtype=torch.float32, device=eng.device)
    eng.fake_tower_batched(Pairs(t(pop), t(nic)), t(seg_of), t(row0), t(steps), y, keep)
    torch.cuda.synchronize()
    got = y.cpu().numpy().astype(np.float64)
    worst = 0.0
    for sidx, (r0, ns) in enumerate(zip(row0, segs)):
        sl = slice(r0, r0 + ns)
        dm = Hh.d_masks(SEED, int(steps[sidx]), ns, hs[1:], keep)
        v = pop[sl] >= 0
        T = O.d_tower(D, np.where(v, pop[sl], 0), np.where(v, nic[sl], 0), dm, keep)
        worst = max(worst, float(np.max(np.abs(got[sl] - np.where(v, T["y"], 0.0)))))
        assert np.all(got[sl][~v] == 0.0)
    print("hot forward-only tower %s d_arith %s: worst |y - oracle| %.2e over %d slots" % (hs, d_arith, worst, n))
    assert worst < 2e-6, worst
