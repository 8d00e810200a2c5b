"""Posterior-aware scores on the GPU (tests/posterior_ref.py is the reference; its `bound` is the only tolerance of the products):
ltg_posterior_h2 with injected noise and with the counter RNG, ltg_posterior_scores fed the device's own image (every S, ragged item and
row counts, with and without the bf16 shadow, both cfg precisions, sentinels around the outputs), slabs against the whole call bit for
bit, degenerate posteriors, the S forwards + torch accumulation this replaces, ltg_posterior_entries, Recommender(posterior=) against the
entry points called by hand and with rules and attachments, the item-sharded recommender (tests/dist_posterior_worker.py) and both CLIs
on Askubuntu_Sample in fresh child processes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import posterior_ref as R
import serving_harness
from serving_harness import DEV, _bits, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu
SHARDED = "test_gpu_posterior::test_sharded_recommender_with_posterior"
assert 29701 not in {port for _, port in serving_harness.PORTS.values()}, "the rendezvous port of the sharded test is taken"
serving_harness.PORTS[SHARDED] = ("dist_posterior_worker.py", 29701)
SEED = 98765


@functools.lru_cache(maxsize=None)
def _fx(n, I, S):
    """the shared fixture, computed once per shape; a test that changes an array copies it first"""
    return R.fixture(n, I, S)


class _Dev:
    """cfg + generator state of the columns lo .. hi of a fixture on the device, through the C ABI alone"""

    def __init__(self, fx, lo=0, hi=None, shadow=False, prec=0, seed=SEED):
        import torch
        from ltgan import _cabi as cabi
        self.lib, self.cabi = cabi.load(), cabi
        I = fx["I"]
        hi = I if hi is None else hi
        sl = (lo, hi) != (0, I)
        self.n_items = hi - lo
        self.cfg = cabi.ltg_config(hi - lo, R.H, R.Z, I, 100, 150, 250, 300, prec, 0, lo if sl else 0, I if sl else 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, seed)
        self.t = dict(p2=_t(fx["W_p0"]), p6=_t(fx["b_p0"]), p3=_t(fx["W_p1t"][lo:hi]), p7=_t(fx["b_p1"][lo:hi]))
        self.gen = cabi.ltg_gen_state()
        for i, name in ((2, "p2"), (6, "p6"), (3, "p3"), (7, "p7")):
            self.gen.p[i] = self.t[name].data_ptr()
        self.st = torch.cuda.current_stream().cuda_stream
        if shadow:
            self.t["shadow"] = torch.full((hi - lo, 608), 0x5555, dtype=torch.int16, device=DEV)
            self.gen.wp1t_bf16 = self.t["shadow"].data_ptr()
            assert self.lib.ltg_refresh_shadow(C.byref(self.cfg), C.byref(self.gen), self.st) == 0

    def h2(self, mulv, S, eps=None, row_lo=0, draw=0, want_z=True):
        """-> (image tensor [n * S, 608] int16 on the device, z host [n * S, Z] or None)"""
        import torch
        n = mulv.shape[0]
        mv = _t(np.ascontiguousarray(mulv, np.float32))
        ed = _t(np.ascontiguousarray(eps, np.float32)) if eps is not None else None
        img = torch.full((n * S, 608), 0x5555, dtype=torch.int16, device=DEV)          # (the pad columns must be WRITTEN)
        z = torch.full((n * S, R.Z), 7.0, dtype=torch.float32, device=DEV) if want_z else None
        rc = self.lib.ltg_posterior_h2(C.byref(self.cfg), C.byref(self.gen), mv.data_ptr(), n, row_lo, S, draw, ed.data_ptr() if ed is not None else None,
                                       img.data_ptr(), z.data_ptr() if z is not None else None, self.st)
        assert rc == 0
        torch.cuda.synchronize()
        return img, (z.cpu().numpy() if z is not None else None)

    def scores(self, img, n, S, beta, spread=True):
        """-> host (score [n, I], spread [n, I] or None); the outputs sit inside sentinel-filled buffers that must come back untouched"""
        import torch
        I, pad = self.n_items, 64
        bufs = [torch.full((pad + n * I + pad,), 7.0, dtype=torch.float32, device=DEV) for _ in range(2 if spread else 1)]
        ptr = [b.data_ptr() + 4 * pad for b in bufs]
        rc = self.lib.ltg_posterior_scores(C.byref(self.cfg), C.byref(self.gen), img.data_ptr(), n, S, float(beta), ptr[0], ptr[1] if spread else None,
                                           self.st)
        assert rc == 0
        torch.cuda.synchronize()
        out = []
        for b in bufs:
            h = b.cpu().numpy()
            assert (h[:pad] == 7.0).all() and (h[pad + n * I:] == 7.0).all(), "a cell outside [n, I] was written"
            out.append(h[pad:pad + n * I].reshape(n, I))
        return out[0], (out[1] if spread else None)

    def entries(self, img, S, ids):
        import torch
        n, k = ids.shape
        idd = _t(np.ascontiguousarray(ids, np.int32))
        m = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
        s = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
        assert self.lib.ltg_posterior_entries(C.byref(self.cfg), C.byref(self.gen), img.data_ptr(), n, S, idd.data_ptr(), k, m.data_ptr(), s.data_ptr(),
                                              self.st) == 0
        torch.cuda.synchronize()
        return m.cpu().numpy(), s.cpu().numpy()


def _img_host(img):
    """the device image -> (values [rows, 600] float32, the pad columns' bits)"""
    h = img.cpu().numpy()
    return R.bf16_bits_to_float(h[:, : R.H]), h[:, R.H:]


def _ref(img_vals, fx, S, beta, lo=0, hi=None):
    hi = fx["I"] if hi is None else hi
    W, b = fx["W_bf16"][lo:hi], fx["b_p1"][lo:hi]
    return R.scores(img_vals, W, b, S, beta), R.bound(img_vals, W, b, S)


def _within(got, want, tol, what):
    d = np.abs(got.astype(np.float64) - want)
    worst = float((d / tol).max())
    print("%s: largest |got - ref| / tol = %.4f (largest difference %.3g, smallest tol %.3g)" % (what, worst, float(d.max()), float(tol.min())))
    assert (d <= tol).all(), (what, worst)


# ---------------------------------------------------------------------------------------------- 1. h2 with injected noise
@pytest.mark.parametrize("n,S", [(1, 1), (5, 4), (37, 8), (5, 16), (37, 32)])
def test_h2_with_injected_noise(n, S):
    fx = _fx(n, 1000, S)
    dev = _Dev(fx)
    img, z = dev.h2(fx["mulv"], S, eps=fx["eps"])
    vals, pad = _img_host(img)
    _, h, z_ref = R.h2_image(fx["mulv"], fx["eps"], fx["W_p0"], fx["b_p0"])
    d = np.abs(vals.astype(np.float64) - h)
    print("n %d, S %d: largest (|image - h| - 2^-8 |h|) %.3g, largest |z - ref| %.3g" % (n, S, float((d - 2.0 ** -8 * np.abs(h)).max()),
                                                                                       float(np.abs(z - z_ref).max())))
    assert (d <= 2.0 ** -8 * np.abs(h) + 1e-6).all()
    assert (pad == 0).all() and pad.shape == (n * S, 8)
    mu = np.repeat(fx["mulv"][:, None, : R.Z].astype(np.float64), S, 1)
    sde = np.exp(0.5 * fx["mulv"][:, None, R.Z:].astype(np.float64)) * fx["eps"]
    assert (np.abs(z - z_ref) <= 4 * 2.0 ** -24 * (np.abs(mu) + np.abs(sde)).reshape(n * S, R.Z)).all()


# ---------------------------------------------------------------------------------------------- 2. the counter RNG
def test_h2_counter_rng():
    from oracle import ltg_oracle as O
    n, S = 64, 16
    fx = _fx(5, 1000, 4)
    dev = _Dev(fx)
    zero = np.zeros((n, 2 * R.Z), np.float32)                                # mu = 0, logvar = 0: z = e
    img, z = dev.h2(zero, S, draw=3)
    idx = np.arange(n * S * R.Z, dtype=np.uint64)
    want = O.rng_normal(SEED, R.STREAM_POSTERIOR_EPS, 3, idx).reshape(n * S, R.Z)
    print("largest |z - oracle normal| %.3g, largest |e| %.3g" % (float(np.abs(z - want).max()), float(np.abs(want).max())))
    assert np.abs(want).max() <= 5.8 and (np.abs(z - want) <= 1e-5).all()
    N = z.size
    assert N == 64 * 16 * 200 and abs(float(z.mean(dtype=np.float64))) <= 5 / np.sqrt(N)
    assert abs(float(z.astype(np.float64).var()) - 1.0) <= 5 * np.sqrt(2.0 / N)
    # the rows of a call are keyed by their GLOBAL row: [0, 37) == [0, 20) + [20, 37) with row_lo = 20
    mv = _fx(37, 1000, 16)["mulv"]
    whole, zw = dev.h2(mv, S, draw=3)
    a, za = dev.h2(mv[:20], S, draw=3)
    b, zb = dev.h2(mv[20:], S, draw=3, row_lo=20)
    assert np.array_equal(whole.cpu().numpy(), np.concatenate([a.cpu().numpy(), b.cpu().numpy()]))
    assert np.array_equal(_bits(zw), _bits(np.concatenate([za, zb])))
    other, _ = dev.h2(mv, S, draw=4)
    assert not np.array_equal(other.cpu().numpy(), whole.cpu().numpy())
    again, _ = dev.h2(mv, S, draw=3)
    assert np.array_equal(again.cpu().numpy(), whole.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 3. the scores
@pytest.mark.parametrize("I", [1000, 1003])
@pytest.mark.parametrize("n,S", [(1, 1), (37, 1), (5, 4), (37, 4), (1, 8), (37, 8), (5, 16), (37, 16), (1, 32), (5, 32), (37, 32)])
def test_scores_against_the_reference(n, S, I):
    fx = _fx(n, I, S)
    dev = _Dev(fx)
    img, _ = dev.h2(fx["mulv"], S, eps=fx["eps"], want_z=False)
    vals, _ = _img_host(img)                                                 # the device's own image: the reference's operands
    (_, mean, std), tol = _ref(vals, fx, S, 0.0)
    got_mean, got_std = dev.scores(img, n, S, 0.0)
    _within(got_mean, mean, tol, "mean n %d S %d I %d" % (n, S, I))
    _within(got_std, std, tol, "std")
    if S == 1:
        assert (got_std == 0.0).all()
    betas = (1.5, -1.0) if S > 1 else ()
    for beta in betas:
        got, sp = dev.scores(img, n, S, beta)
        _within(got, mean + beta * std, 3 * tol, "score beta %g" % beta)
        assert np.array_equal(_bits(sp), _bits(got_std))
    # the shadow and the cfg's precision change no bit
    beta = 1.5 if S > 1 else 0.0
    base, base_sp = dev.scores(img, n, S, beta)
    for kw in (dict(shadow=True), dict(prec=1), dict(shadow=True, prec=1)):
        other = _Dev(fx, **kw)
        got, sp = other.scores(img, n, S, beta)
        assert np.array_equal(_bits(got), _bits(base)) and np.array_equal(_bits(sp), _bits(base_sp)), kw
    only, none = dev.scores(img, n, S, beta, spread=False)                   # spread_out is optional
    assert none is None and np.array_equal(_bits(only), _bits(base))


# ---------------------------------------------------------------------------------------------- 4. slabs
@pytest.mark.parametrize("S", [4, 16, 32])
def test_slabs_equal_the_whole_call(S):
    n, I, cut = 37, 1003, 517
    fx = _fx(n, I, S)
    dev = _Dev(fx)
    img, _ = dev.h2(fx["mulv"], S, eps=fx["eps"], want_z=False)
    whole, whole_sp = dev.scores(img, n, S, 1.5)
    again, again_sp = dev.scores(img, n, S, 1.5)
    assert np.array_equal(_bits(whole), _bits(again)) and np.array_equal(_bits(whole_sp), _bits(again_sp))
    for shadow in (False, True):
        parts = [_Dev(fx, lo=a, hi=b, shadow=shadow).scores(img, n, S, 1.5) for a, b in ((0, cut), (cut, I))]
        assert np.array_equal(_bits(np.concatenate([p[0] for p in parts], 1)), _bits(whole))
        assert np.array_equal(_bits(np.concatenate([p[1] for p in parts], 1)), _bits(whole_sp))


# ---------------------------------------------------------------------------------------------- 5. degenerate posteriors
def _engine_with(fx, precision="bf16"):
    from ltgan.engine import Engine
    eng = Engine(fx["I"], h_sizes=(16, 24, 40, 32), lr=1e-3, precision=precision, seed=SEED)
    eng.set_generator([np.array(a) for a in fx["gen"]])
    return eng


def _batch(eng, n, I, seed=5):
    import helpers as Hh
    from ltgan.engine import CsrRows
    X = Hh.random_history(np.random.default_rng(seed), n, I, mean_nnz=12)
    return X, CsrRows(_t(X.indptr.astype(np.int32)), _t(X.indices.astype(np.int32)), 0, n)


@pytest.mark.parametrize("S", [4, 8, 16, 32])
def test_degenerate_posterior(S):
    import torch
    n, I = 37, 1003
    fx = _fx(n, I, S)
    eng = _engine_with(fx)
    _, batch = _batch(eng, n, I)
    acts = eng.new_acts(n)
    eng.forward(batch, acts, keep_prob=1.0, is_training=0.0, rng_step=1)      # z = mu: the plain bf16 logits
    torch.cuda.synchronize()
    plain = acts.logits.cpu().numpy()
    mulv = acts.mulv.cpu().numpy().copy()
    mulv[:, R.Z:] = -200.0
    dev = _Dev(fx)
    img, _ = dev.h2(mulv, S, eps=fx["eps"], want_z=False)
    img1, _ = dev.h2(mulv, 1, eps=fx["eps"][:, :1], want_z=False)
    one, _ = dev.scores(img1, n, 1, 0.0)
    for beta in (0.0, 1.5, -1.0):
        got, sp = dev.scores(img, n, S, beta)
        assert (sp == 0.0).all() and np.array_equal(_bits(got), _bits(one)), beta
    vals, _ = _img_host(img1)
    tol = R.bound(vals, fx["W_bf16"], fx["b_p1"], 1)
    _within(one, plain.astype(np.float64), tol, "S = 1 at logvar -200 against ltg_vae_forward, S %d" % S)


# ---------------------------------------------------------------------------------------------- 6. the composition this replaces
@pytest.mark.parametrize("S", [4, 16])
def test_against_s_forwards_and_torch_accumulation(S):
    import torch
    n, I = 37, 1003
    fx = _fx(n, I, S)
    eng = _engine_with(fx)
    _, batch = _batch(eng, n, I)
    acts = eng.new_acts(n)
    eps = _t(fx["eps"])
    ls = []
    for s in range(S):
        eng.forward(batch, acts, keep_prob=1.0, is_training=1.0, rng_step=1, eps=eps[:, s].contiguous())
        ls.append(acts.logits.double().clone())
    l = torch.stack(ls, 1)
    mean = l.mean(1)
    std = ((l - mean[:, None]) ** 2).mean(1).sqrt()
    image = eng.posterior_image(n, S)
    score = torch.full((n, I), 7.0, dtype=torch.float32, device=DEV)
    spread = torch.full((n, I), 7.0, dtype=torch.float32, device=DEV)
    eng.posterior_h2(acts.mulv, n, 0, S, 0, image, eps=eps)
    eng.posterior_scores(image, n, S, 0.0, score, spread)
    torch.cuda.synchronize()
    vals, _ = _img_host(image)
    W, b = fx["W_bf16"], fx["b_p1"]
    tol = R.bound(vals, W, b, S) + 2.0 ** -8 * R.magnitude(vals, W, b, S)     # + the image's bf16 rounding carried through the reference
    _within(score.cpu().numpy(), mean.cpu().numpy(), tol, "mean against %d forwards" % S)
    _within(spread.cpu().numpy(), std.cpu().numpy(), tol, "std against %d forwards" % S)
    eng.posterior_scores(image, n, S, 1.5, score)
    torch.cuda.synchronize()
    _within(score.cpu().numpy(), (mean + 1.5 * std).cpu().numpy(), 3 * tol, "score against %d forwards" % S)


# ---------------------------------------------------------------------------------------------- 7. the entries
@pytest.mark.parametrize("S", [1, 4, 16, 32])
def test_entries_equal_the_scores_cells(S):
    n, I, k, cut = 37, 1003, 23, 517
    fx = _fx(n, I, S)
    dev = _Dev(fx)
    img, _ = dev.h2(fx["mulv"], S, eps=fx["eps"], want_z=False)
    mean, std = dev.scores(img, n, S, 0.0)
    rng = np.random.default_rng(S)
    ids = np.stack([rng.choice(I, k, replace=False) for _ in range(n)]).astype(np.int32)
    ids[:, -3:] = -1                                                         # padding
    ids[0, 0], ids[1, 0], ids[2, 0] = 0, I - 1, cut
    real = ids >= 0
    vals, _ = _img_host(img)
    tol = np.take_along_axis(R.bound(vals, fx["W_bf16"], fx["b_p1"], S), np.where(real, ids, 0).astype(np.int64), 1)
    cell = lambda a: np.take_along_axis(a, np.where(real, ids, 0).astype(np.int64), 1)
    for shadow in (False, True):
        m, s = _Dev(fx, shadow=shadow).entries(img, S, ids)
        assert (m[~real] == 0.0).all() and (s[~real] == 0.0).all()
        assert (np.abs(m.astype(np.float64) - cell(mean))[real] <= tol[real]).all() and (np.abs(s.astype(np.float64) - cell(std))[real] <= tol[real]).all()
        if S == 1:
            assert (s == 0.0).all()
    # slabs: an entry outside the slab gives 0.0, so the slabs' tables add up to the whole call's
    whole = dev.entries(img, S, ids)
    parts = [_Dev(fx, lo=a, hi=b).entries(img, S, ids) for a, b in ((0, cut), (cut, I))]
    for j in range(2):
        own = [(ids >= a) & (ids < b) for a, b in ((0, cut), (cut, I))]
        assert (parts[0][j][~own[0]] == 0.0).all() and (parts[1][j][~own[1]] == 0.0).all()
        assert np.array_equal(parts[0][j] + parts[1][j], whole[j])


# ---------------------------------------------------------------------------------------------- 8. the host layer
def _by_hand(eng, rec, post, ev, lo, hi, k):
    """the lists of users lo .. hi from the entry points and ltg_topk, on a fresh forward -> host (ids, scores, mean, std, lse)"""
    import torch
    n, S = hi - lo, post.samples
    tr, _ = ev.rows(lo, hi)
    acts = eng.new_acts(n)
    eng.forward(tr, acts, keep_prob=1.0, is_training=0.0, rng_step=77 + lo)
    image = eng.posterior_image(n, S)
    eng.posterior_h2(acts.mulv, n, lo, S, post.draw, image)
    eng.posterior_scores(image, n, S, post.beta, acts.logits)
    lse = torch.empty(n, dtype=torch.float32, device=DEV)
    eng.row_lse(acts.logits, n, lse)
    s = torch.empty(n, k, dtype=torch.float32, device=DEV)
    i = torch.empty(n, k, dtype=torch.int32, device=DEV)
    eng.topk(acts, tr, k, s, i)
    m, d = torch.empty_like(s), torch.empty_like(s)
    eng.posterior_entries(image, S, i, m, d)
    torch.cuda.synchronize()
    return i.cpu().numpy(), s.cpu().numpy(), m.cpu().numpy(), d.cpu().numpy(), lse.cpu().numpy(), acts.logits.cpu().numpy(), image


def test_recommender_with_posterior(monkeypatch):
    import torch
    import helpers as Hh
    from ltgan import serving
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Explore, ExposureCap, LongTailReport, MinSlots, Posterior, Recommender
    I, n, k, chunk, S = 1003, 200, 50, 128, 8
    rng = np.random.default_rng(12)
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=chunk).run(rng_step=77, keep_prob=1.0)
    again_ids, again_sc = Recommender(eng, ev, k=k, chunk=chunk, posterior=None).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(again_ids, plain_ids) and np.array_equal(_bits(again_sc), _bits(plain_sc))
    monkeypatch.setattr(serving, "POSTERIOR_IMAGE_BYTES", 48 * S * 608 * 2)   # row blocks of 48 users: below the chunk
    post = Posterior(samples=S, beta=1.0, draw=2, stats=True)
    rec = Recommender(eng, ev, k=k, chunk=chunk, posterior=post)
    assert post.block == 48
    ids, sc = rec.run(rng_step=77, keep_prob=1.0)
    mean, std = post.table()
    ref_rows = []
    for lo, hi in ((0, 128), (128, 200)):
        h_i, h_s, h_m, h_d, h_lse, h_logits, image = _by_hand(eng, rec, post, ev, lo, hi, k)
        assert np.array_equal(ids[lo:hi], h_i) and np.array_equal(_bits(sc[lo:hi]), _bits(h_s))
        assert np.array_equal(_bits(mean[lo:hi]), _bits(h_m)) and np.array_equal(_bits(std[lo:hi]), _bits(h_d))
        # every served entry's reference score reaches the reference's k-th score up to 2 tol (near-ties may swap)
        vals, _ = _img_host(image)
        W, b = R.bf16_round(eng.g_p[3].cpu().numpy()), eng.g_p[7].cpu().numpy()
        (ref_sc, _, _), tol = R.scores(vals, W, b, S, 1.0), 3 * R.bound(vals, W, b, S)
        Xc = X.tocsr()
        for r in range(hi - lo):
            elig = np.ones(I, bool)
            elig[Xc.indices[Xc.indptr[lo + r]:Xc.indptr[lo + r + 1]]] = False
            kth = np.sort(ref_sc[r][elig])[-k]
            assert elig[h_i[r]].all() and (ref_sc[r][h_i[r]] >= kth - 2 * tol[r].max()).all(), lo + r     # (the entry's tol + the k-th item's)
        ref_rows.append(h_lse)
    assert np.array_equal(_bits(rec.acts.lse[:72].cpu().numpy()), _bits(ref_rows[1]))     # the last chunk's lse is that of the scores
    assert (std > 0).all() and not np.array_equal(ids, plain_ids)
    st = post.stats()
    moved = sum(int((~np.isin(ids[u], plain_ids[u])).sum()) for u in range(n))
    assert st["entries"] == n * k and st["moved_share"] == moved / (n * k) and 0.0 < st["moved_share"] < 1.0
    assert abs(st["mean_std"] - float(std.astype(np.float64).mean())) < 1e-9
    print("UCB at beta 1: mean entry std %.4f, moved share %.4f" % (st["mean_std"], st["moved_share"]))
    # the chunking and the row blocks change nothing; another draw does
    monkeypatch.setattr(serving, "POSTERIOR_IMAGE_BYTES", 256 << 20)
    p2 = Posterior(samples=S, beta=1.0, draw=2)
    ids2, sc2 = Recommender(eng, ev, k=k, chunk=77, posterior=p2).run(rng_step=77, keep_prob=1.0)
    assert p2.block == 77 and np.array_equal(ids2, ids) and np.array_equal(_bits(sc2), _bits(sc)) and np.array_equal(_bits(p2.table()[1]), _bits(std))
    ids3, _ = Recommender(eng, ev, k=k, chunk=chunk, posterior=Posterior(samples=S, beta=1.0, draw=3)).run(rng_step=77, keep_prob=1.0)
    assert not np.array_equal(ids3, ids)
    # LCB and the posterior mean, one Thompson draw
    for kw in (dict(samples=S, beta=-1.0), dict(samples=S, beta=0.0), dict(samples=1, beta=0.0)):
        p = Posterior(**kw)
        i_k, s_k = Recommender(eng, ev, k=k, chunk=chunk, posterior=p).run(rng_step=77, keep_prob=1.0)
        m_k, d_k = p.table()
        assert i_k.min() >= 0 and (np.diff(s_k, axis=1) <= 0).all()
        want = (np.float32(kw["beta"]) * d_k.astype(np.float64) + m_k)
        assert np.abs(s_k - want).max() <= 1e-4                              # (the entries' K order differs from the scores': fp32 rounding)
        assert (d_k == 0).all() if kw["samples"] == 1 else (d_k > 0).all()
    # with a rule, an exploration policy, a rule that reads the lse, and the report: it runs, and the lists obey their own rule
    rep = LongTailReport(labels, 3, k_ndcg=k, k_r1=20, k_r2=k, k_exp=k)
    slots = [0, 0, 20]
    ids_r, _ = Recommender(eng, ev, k=k, chunk=chunk, posterior=Posterior(samples=S), rule=MinSlots(labels, 3, slots), report=rep).run(
        rng_step=77, keep_prob=1.0)
    assert ((labels[ids_r] == 2).sum(1) >= 20).all()
    assert np.array_equal(rep.table()[1], np.bincount(ids_r.ravel(), minlength=I))
    exp = Explore(0.8, fixed=5, draw=1)
    p_e = Posterior(samples=S, beta=0.5, stats=True)
    ids_e, _ = Recommender(eng, ev, k=k, chunk=chunk, posterior=p_e, explore=exp).run(rng_step=77, keep_prob=1.0)
    srt = np.sort(ids_e, 1)
    assert (srt[:, 1:] != srt[:, :-1]).all() and (exp.table()[:, :5] == 0).all() and (exp.table()[:, 5:] < 0).all()
    head, _ = Recommender(eng, ev, k=5, chunk=chunk, posterior=Posterior(samples=S, beta=0.5)).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids_e[:, :5], head)                                # the fixed head is the posterior's top-5
    cap = ExposureCap(30)
    ids_c, _ = Recommender(eng, ev, k=k, chunk=chunk, posterior=Posterior(samples=S), cap=cap).run(rng_step=77, keep_prob=1.0)
    assert cap.needs_lse and np.bincount(ids_c[ids_c >= 0].ravel(), minlength=I).max() <= 30
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2])
def test_sharded_recommender_with_posterior(world):
    run_ranks("dist_posterior_worker.py", ["1001", "230"], world, "POSTERIOR_SHARDED_OK world=%d" % world, port_of=SHARDED)


def test_clis_on_askubuntu(tmp_path):
    import torch
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    from ltgan import recommend as rc
    from ltgan.dataset import EvalData
    from ltgan.trainer import Posterior, Recommender
    post = Posterior(samples=16, beta=1.0, draw=0, stats=True)
    ids, sc = Recommender(eng, EvalData(tr, te, eng.device), k=100, posterior=post).run(rng_step=rc.RNG_STEP, keep_prob=1.0)
    mean, std = post.table()
    out = run_cli("recommend.py", [ds, ck, "--posterior", "1.0", "--keep-prob", "1.0", "--uncertainty", "unc.tsv", "--out", "post.tsv", "--npz",
                                   "post.npz"], cwd)
    print(out[-1])
    st = post.stats()
    assert out[-1] == "posterior@100: beta 1, samples 16, draw 0, mean entry std %.6f, moved share %.6f" % (st["mean_std"], st["moved_share"])
    assert out[-2].startswith("users: %d\tniche_share@100: " % tr.shape[0])
    z = np.load(os.path.join(cwd, "post.npz"))
    assert np.array_equal(z["ids"], ids) and np.array_equal(_bits(z["scores"]), _bits(sc))
    assert np.array_equal(_bits(z["post_mean"]), _bits(mean)) and np.array_equal(_bits(z["post_std"]), _bits(std))
    rows = [line.split("\t") for line in open(os.path.join(cwd, "unc.tsv")).read().splitlines()]
    assert [int(u) for u, _ in rows] == list(range(uid0, uid0 + tr.shape[0]))
    for u, (_, items) in enumerate(rows):
        f = [x.split(":") for x in items.split(",")]
        assert [int(x[0]) for x in f] == ids[u].tolist()
        assert [x[1] for x in f] == ["%.6g" % float(v) for v in mean[u]] and [x[2] for x in f] == ["%.6g" % float(v) for v in std[u]]
        assert all(float(x[2]) >= 0 for x in f)
    assert (std >= 0).all() and st["mean_std"] > 0
    out = run_cli("longtail.py", [ds, ck, "--posterior", "1.0"], cwd)
    print("\n".join(out[-4:]))
    assert out[-1].startswith("posterior@100: beta 1, samples 16, draw 0, mean entry std ") and ", moved share " in out[-1]
    grp = [l.split("\t") for l in out if l.startswith("posterior_std\t")]
    assert [g[1] for g in grp] == ["popular", "niche"] and sum(int(g[2]) for g in grp) == tr.shape[0] * 100
    assert all(float(g[3]) > 0 for g in grp if int(g[2]) > 0)
    assert any(l.startswith("all\t") and len(l.split("\t")) == 9 for l in out)
    torch.cuda.synchronize()
