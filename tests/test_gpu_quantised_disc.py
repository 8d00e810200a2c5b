"""The bf16 and fp8 discriminator (ltg_config.d_precision) against the fp64 oracle fed the SAME quantised operands (O.d_tower(dq) /
O.d_tower_backward(dq)), on every route the library picks for these modes: the operand-format fp8 step (ltg_fp8bwd.h: k8_gather_t,
fk8t_d_l1, k8_d_out, k8_d_bwd1 / bwd2, k8_d_adam) at the row counts where its 128-row padding and 1 024-row split-K chunks change; the
staged and non-staged fp8 forwards with the generic mode-2 backward; k_d_*<MODE = 1 | 2> on every tile variant; the forward-only tower of
phase G; the Adam sweeps from warm moments; a trained model's range and the e4m3 clamp.

Bounds.  D step: loss 1e-4; first moments in the energy and the max norm at the project's figures for the mode and size class (bf16 2e-3,
fp8 2e-2, fp8 with h0 >= 512 or h3 > 512 6e-2: quantised_ref.m_tol), second moments twice that, theta through _check_adam_move.  Where a
case is listed in D_WIDEN its bound is 4 x the jitter floor of THAT case instead (tests/quantised_ref.py: the noise model; computed in the
test, printed beside the device's figure) -- never a device figure.  Forward-only tower: max |y - oracle| and the median of the same within
4 x the floor of the case, each; tests/test_quantised_disc_cpu.py lists the floors and holds the float32 oracle to the same bounds.

Floors (max / median |dy|, the worst of three draws): fp8 2.7e-5 / 3.9e-7 (12 x 20 x 28 x 16) .. 5.8e-3 / 1.7e-5 (512 x 256 x 256 x 640), 3.7e-3 /
7.3e-5 at BASELINE's 2048 x 1024 x 512 x 256, 1.8e-2 / 1.3e-5 with a trained model's range; bf16 3.6e-7 / 1.1e-8 .. 2.3e-4 / 4.8e-7, 7.3e-4 /
2.9e-7 trained.  One MI355X measured 0.001 .. 0.7 of the floor in the maximum and at most 0.3 of it in the median -- except at the smallest
bf16 size, where float32's own rounding of y (1.5e-8) is 1.3 x the floor of 1.1e-8: the tightest bound of the file, 4.4e-8.  DESIGN.md
section 6 has the table."""
import functools

import numpy as np
import pytest

import helpers as Hh
import quantised_ref as Q
import test_gpu_parity as TP
from oracle import ltg_oracle as O

pytestmark = pytest.mark.gpu

SEED = Q.SEED
assert SEED == TP.SEED

OPFMT, BASE = (256, 128, 128, 128), (2048, 1024, 512, 256)            # the smallest size d_fp8_opfmt takes; BASELINE config 5
# (dq, layer sizes, nr, nf).  Operand format: NP = 128 with one real row / with five; n = 128 (no padding); n = 129; n = 1 024 (exactly one
# chunk); n = 1 025 (NP = 1 152: the second chunk holds one real row in 128); three chunks with the real | fake boundary inside a tile
D_Q = [("fp8", OPFMT, nr, nf) for nr, nf in ((1, 0), (0, 5), (64, 64), (100, 29), (600, 424), (600, 425), (1100, 1000))] + \
    [("fp8", BASE, 600, 425)] + \
    [("fp8", hs, nr, nf) for hs in ((512, 256, 256, 640), (192, 64, 128, 128), (256, 128, 128, 100)) for nr, nf in ((33, 7), (600, 425))] + \
    [(dq, hs, nr, nf) for hs in ((520, 300, 260, 132), (514, 300, 250, 130), (100, 151, 250, 300), (4, 1, 3, 4), (1, 1, 1, 1))
     for nr, nf in ((33, 7), (700, 650)) for dq in ("bf16", "fp8")] + \
    [("bf16", (100, 150, 250, 300), 900, 950)]                        # bwd1 promoted to 64-tiles: t32 = 1 794 > 1 024
# Cases held, in the norm named, to 4 x their own jitter floor instead of the class figure (the other norm keeps the class figure).
# ONE pair row: dw1 | db1 is the outer product of that row's e4m3 embedding with its 128 dpre1 values, so ONE dpre1 value that rounds the
# other way (6 %) is the whole max-norm error: the device is 3.6e-2 off there (exactly one e4m3 step of one element; 1.0e-2 in the energy
# norm, inside the class figure), the noise model's three draws reach 3.6e-2 as well -- floor 3.6e-2, bound 1.4e-1.
D_WIDEN = {("fp8", OPFMT, 1, 0): ("max",)}
D_HOT = [("bf16", (100, 150, 250, 300), 700, 650), ("fp8", OPFMT, 600, 425), ("fp8", BASE, 260, 250)]


def _q_ids(cases):
    return ["%s-%s" % (c[0], i) for c, i in zip(cases, TP._d_case_ids([(nr, nf, hs) for _, hs, nr, nf in cases]))]


def _pairs(dev, pop, nic):
    import torch
    from ltgan.engine import Pairs
    if len(pop) == 0:
        z = torch.zeros(1, dtype=torch.int32, device=dev)
        return Pairs(z, z.clone(), n=0)
    return Pairs(torch.from_numpy(pop).to(dev), torch.from_numpy(nic).to(dev))


def _prepared(c, dq, m=None, v=None, t0=2):
    eng = TP._engine(c["I"], "fp32", hs=c["hs"], lr=1e-3, d_precision=dq)
    emb, darr = Hh.disc_to_engine(c["D"])
    kw = {} if m is None else dict(m=[m[k] for k in O.D_KEYS], v=[v[k] for k in O.D_KEYS])
    eng.set_discriminator(emb, darr, **kw)
    eng.adam_t = t0
    return eng, _pairs(eng.device, c["rp"], c["rn"]), _pairs(eng.device, c["fp"], c["fn"])


def _state(eng):
    return [[t.cpu().numpy().copy() for t in ts] for ts in (eng.d_p, eng.d_m, eng.d_v)]


def _q_step_case(dq, hs, nr, nf, hot=False, widen=()):
    """the quantised twin of test_gpu_parity._d_step_case: one cold D step at shared step t = 3, holes at 5 %, keep = 0.7, every bias
    non-zero: loss, m, v and the theta move.  widen: the norms ("energy", "max") held to 4 x this case's jitter floor instead of the class
    figure (D_WIDEN).  Returns (case, oracle parts) for the statements a caller adds."""
    import torch
    c = Q.d_case(nr, nf, hs, hot=hot)
    D = c["D"]
    want_loss, g, _, _, parts = Q.d_oracle(c, dq, parts=True)
    ad = O.SharedAdam(1e-3)
    ad.t = 2
    D64 = {k: np.asarray(v, np.float64) for k, v in D.items()}
    ad.apply(D64, g, O.D_KEYS)
    eng, real, fake = _prepared(c, dq)
    if dq == "fp8" and hs in (OPFMT, BASE):
        assert eng.d_fp8 is not None                       # the operand-format route has its shadows
    loss = float(eng.d_step(real, fake, c["keep"], rng_step=c["step"]).cpu().numpy()[0])
    torch.cuda.synchronize()
    d_p, d_m, d_v = _state(eng)
    floor = Q.d_floor(c, dq, g)
    tol = Q.m_tol(dq, hs)
    bad = []
    lerr = abs(loss - want_loss) / max(1.0, abs(want_loss))
    print("quantised D step %s %s (%d, %d)%s: loss rel err %.2e" % (dq, hs, nr, nf, " hot" if hot else "", lerr))
    if not lerr < 1e-4:
        bad.append(("loss", loss, want_loss))
    for i, k in enumerate(O.D_KEYS):
        m_got, m_want = d_m[i].reshape(-1).astype(np.float64), ad.m[k].reshape(-1)
        v_got, v_want = d_v[i].reshape(-1).astype(np.float64), ad.v[k].reshape(-1)
        fig = (Q.energy(m_got, m_want), Hh.rel_err(m_got, m_want), Q.energy(v_got, v_want), Hh.rel_err(v_got, v_want))
        te = Q.FACTOR * floor[k][0] if "energy" in widen else tol
        tm = Q.FACTOR * floor[k][1] if "max" in widen else tol
        print("    %s: m energy / max %.2e / %.2e, v %.2e / %.2e; class figure %.0e, 4 x jitter floor energy / max %.2e / %.2e%s" % (
            (k,) + fig + (tol, Q.FACTOR * floor[k][0], Q.FACTOR * floor[k][1], " (the bound in the %s norm)" % " and ".join(widen) if widen else "")))
        for name, got, lim in (("m energy", fig[0], te), ("m max", fig[1], tm), ("v energy", fig[2], 2 * te), ("v max", fig[3], 2 * tm)):
            if not got < lim:
                bad.append((k, name, got, lim))
    assert not bad, bad
    for i, k in enumerate(O.D_KEYS):
        p0 = np.asarray(D[k], np.float64).reshape(-1)
        TP._check_adam_move(d_p[i].reshape(-1) - p0, D64[k].reshape(-1) - p0, ad.m[k].reshape(-1), ad.lr_t(3), ("theta", k))
    return c, parts


@pytest.mark.parametrize("dq,hs,nr,nf", D_Q, ids=_q_ids(D_Q))
def test_quantised_d_step_matches_oracle(dq, hs, nr, nf):
    _q_step_case(dq, hs, nr, nf, widen=D_WIDEN.get((dq, hs, nr, nf), ()))


# ---------------------------------------------------------------------------------------------------------------- Adam sweeps, warm
ADAM_CASES = [("fp8", OPFMT), ("fp8", BASE), ("fp8", (192, 64, 128, 128)), ("bf16", (100, 150, 250, 300))]


@functools.lru_cache(maxsize=1)
def _e4m3():
    return Q.e4m3_table()


@pytest.mark.parametrize("dq,hs", ADAM_CASES, ids=["%s-%s" % (dq, Q.case_id(hs)) for dq, hs in ADAM_CASES])
def test_quantised_adam_sweeps_from_warm_moments(dq, hs):
    """k8_d_adam (operand format: the weight tiles through adam1, the flat tail through adam_update), k_d_adam with the shadow write-back
    (192 x 64 x 128 x 128) and the bf16 mode's sweep, from injected non-zero moments at shared step t = 212 and with NO gradient noise: the
    device's own gradient vector (ltg_d_grad over the whole batch) goes to ltg_d_apply and, in fp64, to O.SharedAdam -- theta', m', v'
    element-wise at _check_warm_adam's bounds.  The same state from ltg_d_step on an identically prepared engine, at the bounds of
    test_d_step_cut_at_the_gradient_exchange_equals_the_step (which claims bit equality at no size).  Every operand-format shadow equals
    e4m3(2^8 theta') of the theta the device wrote, computed by the oracle's rounding model on the host and compared through a table of
    the 256 e4m3 bytes: value for value, transposition included (the sign of a zero byte is the one thing the values do not show)."""
    import torch
    nr, nf = 130, 61
    c = Q.d_case(nr, nf, hs)
    D, n = c["D"], nr + nf
    a, real, fake = _prepared(c, dq)
    g = torch.empty(a.d_grad_floats(), dtype=torch.float32, device=a.device)
    a.d_grad(real, fake, 0, n, g, keep_prob=c["keep"], rng_step=c["step"])
    torch.cuda.synchronize()
    gh = g.cpu().numpy().astype(np.float64)
    gd, off = {}, 0
    for k in O.D_KEYS:
        sz = np.asarray(D[k]).size
        gd[k] = gh[off:off + sz].reshape(np.asarray(D[k]).shape)
        off += sz
    want_loss = Q.d_oracle(c, dq)[0]
    assert abs(gh[off] - want_loss) < 1e-4 * max(1.0, abs(want_loss))          # the loss in slot P
    assert all(np.abs(gd[k]).max() > 0 for k in O.D_KEYS)
    m0, v0 = TP._warm_moments({k: np.asarray(D[k]) for k in O.D_KEYS}, gd, seed=nr + 3)
    t0 = 211
    ad = O.SharedAdam(1e-3)
    ad.t = t0
    for k in O.D_KEYS:
        ad.m[k], ad.v[k] = m0[k].astype(np.float64), v0[k].astype(np.float64)
    D64 = {k: np.asarray(v, np.float64) for k, v in D.items()}
    ad.apply(D64, gd, O.D_KEYS)
    emb, darr = Hh.disc_to_engine(D)
    a.set_discriminator(emb, darr, m=[m0[k] for k in O.D_KEYS], v=[v0[k] for k in O.D_KEYS])
    a.adam_t = t0
    la = float(a.d_apply(g)[0].item())
    torch.cuda.synchronize()
    assert a.adam_t == t0 + 1
    sa = _state(a)
    worst = 0.0
    for i, k in enumerate(O.D_KEYS):
        sh = np.asarray(D[k]).shape
        worst = max(worst, TP._check_warm_adam(sa[0][i].reshape(sh), np.asarray(D[k]), D64[k], sa[1][i].reshape(sh), ad.m[k], sa[2][i].reshape(sh), ad.v[k],
                                               1e-4, (dq, hs, k), t0 + 1))
    print("quantised Adam sweep %s %s: worst relative error of a theta move from warm moments %.2e" % (dq, hs, worst))
    # ---- the whole step from the same state
    b, real_b, fake_b = _prepared(c, dq, m0, v0, t0)
    lb = float(b.d_step(real_b, fake_b, c["keep"], rng_step=c["step"])[0].item())
    torch.cuda.synchronize()
    assert b.adam_t == t0 + 1 and abs(la - lb) < 2e-6 * abs(la)
    sb = _state(b)
    for i, k in enumerate(O.D_KEYS):
        assert Hh.rel_err(sb[1][i], sa[1][i]) < 2e-5 and Hh.rel_err(sb[2][i], sa[2][i]) < 2e-5, ("m / v", k)
        assert np.abs(sa[0][i].astype(np.float64) - sb[0][i]).max() < 0.02 * 1e-3, ("theta", k)          # 2 % of one Adam move
    # ---- the e4m3 shadows follow the weights the device wrote
    h0, h1, h2, h3 = hs
    if dq == "fp8" and all(x % 64 == 0 for x in hs):
        assert a.d_fp8 is not None and len(a.d_fp8) == 5
        for which, eng, st in (("apply", a, sa), ("step", b, sb)):
            q8 = lambda x: O.fp8_e4m3_round(np.asarray(x, np.float64) * float(1 << O.FP8_S["w"]))
            w1, w2, w3 = st[0][0].reshape(h0, h1), st[0][2].reshape(h0, h2), st[0][4].reshape(h1 + h2, h3)
            want = {"emb": q8(D["emb"]), "w1t": q8(w1).T, "w2t": q8(w2).T, "w3t": q8(w3).T, "w3": q8(w3)}
            for name, t8 in zip(("emb", "w1t", "w2t", "w3t", "w3"), eng.d_fp8):
                got = _e4m3()[t8.cpu().numpy()].reshape(want[name].shape)
                assert np.all(np.isfinite(got)), (which, name)
                miss = np.argwhere(got != want[name])
                assert miss.size == 0, (which, name, len(miss), miss[:4].tolist(), got[tuple(miss[0])], want[name][tuple(miss[0])])
            assert float((want["w1t"] != 0).mean()) > 0.9
    else:
        assert a.d_fp8 is None


# ---------------------------------------------------------------------------------------------------------------- forward-only tower
def _tower_call(eng, pop, nic, seg_of, row0, steps, keep):
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)
    y = torch.full((len(pop),), -1.0, dtype=torch.float32, device=eng.device)
    eng.fake_tower_batched(_pairs(eng.device, pop, nic), t(seg_of), t(row0), t(steps), y, keep)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _tower_engine(c, dq, I=400):
    eng = TP._engine(I, "fp32", hs=c["hs"], lr=1e-3, d_precision=dq)
    emb, darr = Hh.disc_to_engine(c["D"])
    eng.set_discriminator(emb, darr)
    return eng


def _tower_case(hs, segs, dq, hot=False, emb_scale=1.0):
    c = Q.tower_case(hs, segs, hot=hot, emb_scale=emb_scale)
    eng = _tower_engine(c, dq)
    got = _tower_call(eng, c["pop"], c["nic"], c["seg_of"], c["row0"], c["steps"], Q.KEEP)
    y, valid = Q.tower_oracle(c, dq)
    fmax, fmed = Q.tower_floor(c, dq, y, valid)
    emax, emed = Q.y_figures(got, y, valid)
    y32 = Q.tower_oracle(c, None)[0]
    print("quantised forward-only tower %s %s%s: |y - oracle| max / median %.2e / %.2e over %d slots; 4 x floor %.2e / %.2e; oracle's distance from the fp32 tower %.2e" % (
        hs, dq, " hot" if hot else "", emax, emed, c["n"], Q.FACTOR * fmax, Q.FACTOR * fmed, float(np.abs(y - y32)[valid].max())))
    assert np.all(got[~valid] == 0.0)                      # a hole gives exactly 0
    assert emax <= Q.FACTOR * fmax and emed <= Q.FACTOR * fmed, (emax, Q.FACTOR * fmax, emed, Q.FACTOR * fmed)
    # segment independence: the same segments one call each, bit for bit
    for sidx, (r0, ns) in enumerate(zip(c["row0"], c["segs"])):
        sl = slice(r0, r0 + ns)
        one = _tower_call(eng, c["pop"][sl], c["nic"][sl], np.zeros(ns, np.int32), np.zeros(1, np.int32), c["steps"][sidx:sidx + 1], Q.KEEP)
        assert np.array_equal(one.view(np.uint32), got[sl].view(np.uint32)), ("segment", sidx)
    return c, y, valid


TOWER_Q = [(hs, segs, dq) for hs, segs in Q.TOWER_CASES for dq in ("bf16", "fp8")]


@pytest.mark.parametrize("hs,segs,dq", TOWER_Q, ids=["%s-%s" % (Q.case_id(hs), dq) for hs, segs, dq in TOWER_Q])
def test_quantised_forward_only_tower_matches_oracle(hs, segs, dq):
    """ltg_fake_tower_batched with d_precision bf16 / fp8 (disc_forward(with_bwd = false): fk8s_d_l1 / l2, fk8_d_l1 / l2 or k_d_l1 / l2<MODE>
    with k_d_out<false>): y of every slot against O.d_tower(dq), segment by segment with the segment's own dropout counter"""
    _tower_case(hs, segs, dq)


@pytest.mark.parametrize("hs,segs,dq", TOWER_Q, ids=["%s-%s" % (Q.case_id(hs), dq) for hs, segs, dq in TOWER_Q])
def test_quantised_tower_is_position_independent(hs, segs, dq):
    """keep = 1: the same (pop, niche) pair in every slot of n = 1, 63, 64, 65, 129 rows gives ONE bit pattern of y, in every slot and at
    every n -- an element's accumulation order depends neither on its tile row nor on how ragged the last tile is"""
    c = Q.tower_case(hs, segs)
    eng = _tower_engine(c, dq)
    seen = set()
    for n in (1, 63, 64, 65, 129):
        y = _tower_call(eng, np.full(n, 3, np.int32), np.full(n, 7, np.int32), np.zeros(n, np.int32), np.zeros(1, np.int32), np.array([1000], np.int64), 1.0)
        seen |= set(y.view(np.uint32).tolist())
        assert len(seen) == 1, (n, sorted(seen))
    y1 = np.array(sorted(seen), np.uint32).view(np.float32)[0]
    want = O.d_tower(c["D"], np.array([3]), np.array([7]), [np.ones((1, w)) for w in hs[1:]], 1.0, dq=dq)["y"][0]
    assert 0.0 < y1 < 1.0 and abs(float(y1) - want) < 2e-2


def test_fp8_tower_at_the_clamp():
    """embeddings x 10: 0.2 x 10 x 2^8 > 448, so ltg_f2fp8 saturates; the oracle clamps alike, the bounds of the noise model still apply"""
    c = Q.tower_case(OPFMT, (129,), emb_scale=10.0)
    e = np.asarray(c["D"]["emb"], np.float64)[np.concatenate([c["pop"][c["pop"] >= 0], c["nic"][c["nic"] >= 0]])] * float(1 << O.FP8_S["emb"])
    assert np.abs(e).max() > 448.0, "the oracle's scaled operand does not reach the clamp"
    _tower_case(OPFMT, (129,), "fp8", emb_scale=10.0)


G_Q = [("bf16", (100, 150, 250, 300)), ("fp8", (100, 150, 250, 300)), ("fp8", BASE)]


@pytest.mark.parametrize("dq,hs", G_Q, ids=["%s-%s" % (dq, Q.case_id(hs)) for dq, hs in G_Q])
def test_g_step_with_a_quantised_discriminator(dq, hs):
    """test_g_step_parity's 1000-100-step case with a bf16 decoder and a quantised fake tower: sum_y (loss[4]) against O.d_tower(dq) within
    n x the median bound + the max bound; the generator-side assertions exactly as without (sum_y is all the G step takes from the tower)"""
    TP._g_step_case("bf16", 1000, 100, "step", warm=False, hs=hs, d_precision=dq)


# ---------------------------------------------------------------------------------------------------------------- trained range
def _fp8_range_report(c, parts, tag):
    """No scaled operand of the oracle reaches the clamp, and fewer than 1 % of the non-zero dpre1 2^7 values are lost to the e4m3 subnormal
    step (|x| < 2^-10: they convert to zero; a dropped unit or a hole is an exact zero, no value): the case tests arithmetic, not saturation.
    Prints, per operand class, the share of non-zero values that convert to zero, and for dpre1 the share inside (0, 2^-9) as well -- values
    in [2^-10, 2^-9) convert to ONE step, so they keep a sign and a magnitude.  Measured (host, the oracle alone): 256 x 128 x 128 x 128
    (600, 425) 0.01 % lost, 0.02 % inside (0, 2^-9); 2048 x 1024 x 512 x 256 (260, 250) 0.93 % lost, 1.54 % inside (0, 2^-9) (1.03 % of ALL
    entries, zeros included) -- at BASELINE's size the stricter reading of "below the subnormal step" does not hold at 1 %; and 38 % of the
    non-zero dpre3 2^8 values convert to zero there (saturated tanh in the fc layer), which no bound of this file depends on."""
    ops = Q.scaled_operands(c, parts)
    top = {k: max(float(np.abs(a).max()) for a in v) for k, v in ops.items()}
    cat = {k: np.concatenate([np.abs(a).reshape(-1) for a in v]) for k, v in ops.items()}
    nz = {k: v[v > 0] for k, v in cat.items()}
    flushed = {k: float((v < 2.0 ** -10).mean()) for k, v in nz.items()}
    print("%s: largest scaled operand %s; share of non-zero entries flushed to zero %s; dpre1 2^7 entries in (0, 2^-9): %.4f of the non-zero, %.4f of all" % (
        tag, " ".join("%s %.1f" % kv for kv in top.items()), " ".join("%s %.4f" % kv for kv in flushed.items()), float((nz["g1"] < 2.0 ** -9).mean()),
        float((nz["g1"] < 2.0 ** -9).sum() / cat["g1"].size)))
    assert all(v < 448.0 for v in top.values()), top
    assert flushed["g1"] < 0.01, flushed


@pytest.mark.parametrize("dq,hs,nr,nf", D_HOT, ids=_q_ids(D_HOT))
def test_hot_quantised_d_step(dq, hs, nr, nf):
    """Hh.hot_discriminator (emb, w1 .. w4 x 2) through the quantised D step at the same bounds and the same jitter rule"""
    c, parts = _q_step_case(dq, hs, nr, nf, hot=True, widen=D_WIDEN.get((dq, hs, nr, nf, "hot"), ()))
    _, _, y, valid = Q.d_oracle(c, dq)
    y32 = Q.d_oracle(c, None)[2]
    print("hot quantised D step %s %s: oracle's y differs from the fp32 tower's by max / median %.2e / %.2e" % ((dq, hs) + Q.y_figures(y, y32, valid)))
    if dq == "fp8":
        _fp8_range_report(c, parts, "hot fp8 D step %s (%d, %d)" % (hs, nr, nf))


HOT_TOWER = [(hs, segs, dq) for hs, segs in Q.TOWER_HOT for dq in ("bf16", "fp8")]


@pytest.mark.parametrize("hs,segs,dq", HOT_TOWER, ids=["%s-%s" % (Q.case_id(hs), dq) for hs, segs, dq in HOT_TOWER])
def test_hot_quantised_forward_only_tower(hs, segs, dq):
    c, y, valid = _tower_case(hs, segs, dq, hot=True)
    if dq == "fp8":
        e = np.abs(np.asarray(c["D"]["emb"], np.float64)).max() * float(1 << O.FP8_S["emb"])
        w = max(np.abs(np.asarray(c["D"][k], np.float64)).max() for k in ("w1", "w2", "w3")) * float(1 << O.FP8_S["w"])
        assert e < 448.0 and w < 448.0 and 1.0 / Q.KEEP * float(1 << O.FP8_S["act"]) < 448.0          # (|tanh| / keep < 1.43: 91 at scale act)
