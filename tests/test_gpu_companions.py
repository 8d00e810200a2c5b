"""Niche companions on the GPU (ltg_pair_pack / ltg_pair_companions): the side images against the fp64 reference within a
bound derived from the layer lengths and the weights' absolute sums, the scores against the fp64 oracle of the device's own images within
tol = (8 + h3) 2^-24 (sum |w4| + |b4|), the lists against numpy's order bit for bit on the device's own score table (ties by id, padding),
ragged candidate parts merged with ltg_topk_merge against one call bit for bit, a query alone against the same query in a chunk, run-to-run
identity, the discriminator's own forward-only tower, the refusals, and the host layer: PairCompanions, companions.py and the item-sharded
ShardedPairCompanions (tests/dist_companions_worker.py).  The reference is tests/companions_ref.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import companions_ref as CR
import helpers as Hh
import test_companions_cpu as TC
from oracle import ltg_oracle as O
from serving_harness import askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                      # fp32 unit roundoff
SMALL, CONFIG = (16, 24, 40, 37), (100, 150, 250, 300)     # h3 = 37 is a multiple of nothing (ld = 40: three padding columns); config.ini's sizes
F = 4000                            # rows of the embedding table
N_Q, N_C = 130, 3001


class Disc:
    """an oracle discriminator dict on the device, as the C ABI takes it"""

    def __init__(self, D):
        import torch
        from ltgan import _cabi as cabi
        self.cabi, self.lib, self.D = cabi, cabi.load(), D
        hs = (D["w1"].shape[0], D["w1"].shape[1], D["w2"].shape[1], D["w3"].shape[1])
        self.hs, self.feat = hs, D["emb"].shape[0]
        self.cfg = cabi.ltg_config(self.feat, 600, 200, self.feat, *hs, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))).cuda()
        self.t = [dev(D["emb"])] + [dev(D[k]) for k in O.D_KEYS]
        self.disc = cabi.ltg_disc_state()
        self.disc.emb = self.t[0].data_ptr()
        for i in range(8):
            self.disc.p[i] = self.t[1 + i].data_ptr()
        self.ld = self.lib.ltg_pair_ld(C.byref(self.cfg))
        assert self.ld == (hs[3] + 3) // 4 * 4
        self.tol = (8 + hs[3]) * U * (float(np.abs(np.asarray(D["w4"], np.float64)).sum()) + abs(float(np.asarray(D["b4"]).reshape(-1)[0])))

    def pack(self, side, ids):
        import torch
        ids_d = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
        out = torch.full((len(ids), self.ld), 7.0, dtype=torch.float32, device="cuda")      # (the padding columns must be WRITTEN)
        rc = self.lib.ltg_pair_pack(C.byref(self.cfg), C.byref(self.disc), self.cabi.LTG_PAIR_SIDE[side], ids_d.data_ptr(), len(ids), out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        return out

    def companions(self, q_img, q_gid, c_img, c_gid, k):
        """device images, host id arrays -> host (scores [n_q, k], ids [n_q, k])"""
        import torch
        n, m = int(q_img.shape[0]), int(c_img.shape[0])
        qg = torch.from_numpy(np.ascontiguousarray(q_gid, dtype=np.int32)).cuda()
        cg = torch.from_numpy(np.ascontiguousarray(c_gid, dtype=np.int32)).cuda()
        need = self.lib.ltg_pair_companions_ws_bytes(C.byref(self.cfg), n, m, k)
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        s = torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
        i = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
        rc = self.lib.ltg_pair_companions(C.byref(self.cfg), C.byref(self.disc), q_img.data_ptr(), qg.data_ptr(), n, c_img.data_ptr(), cg.data_ptr(), m,
                                          k, s.data_ptr(), i.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        return s.cpu().numpy(), i.cpu().numpy()

    def score_table(self, q_img, c_img):
        """the DEVICE's scores of every pair [n_q, n_c] float32: candidates in parts of 256 with k = 256 and nothing excluded, so every part's
        list is the whole part (a pair's bits do not depend on the part: test_position_independence)"""
        n, m = int(q_img.shape[0]), int(c_img.shape[0])
        out = np.empty((n, m), np.float32)
        none = np.full(n, -1, np.int32)
        for lo in range(0, m, 256):
            hi = min(m, lo + 256)
            s, i = self.companions(q_img, none, c_img[lo:hi].contiguous(), np.arange(lo, hi, dtype=np.int32), 256)
            assert np.all(np.sort(i[:, :hi - lo], 1) == np.arange(lo, hi)) and np.all(i[:, hi - lo:] == -1)
            out[np.arange(n)[:, None], i[:, :hi - lo]] = s[:, :hi - lo]
        return out


def _engine_discriminator(eng):
    """the engine's discriminator as an oracle dict (w4 as the oracle's [h3, 1])"""
    D = dict(zip(O.D_KEYS, [p.cpu().numpy() for p in eng.d_p]), emb=eng.d_emb.cpu().numpy())
    D["w4"] = D["w4"].reshape(-1, 1)
    return D


def _eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _discriminator(hs, hot):
    """the reference's initialiser with non-zero biases; hot: x 2 as tests/helpers.hot_discriminator (tests/test_gpu_hot_range.py: scores to +-8,
    a few per cent of the fc layer's tanh above 0.99 -- a trained model's range)"""
    rng = np.random.default_rng(hs[3] + hot)
    D = O.init_discriminator(F, *hs, seed=11)
    for key in ("b1", "b2", "b3", "b4"):
        D[key] = rng.normal(0, 0.1, np.shape(D[key])).astype(np.float32)
    return Hh.hot_discriminator(D) if hot else {k: np.asarray(v, np.float32) for k, v in D.items()}


@functools.lru_cache(maxsize=None)
def _problem(hs, hot):
    """one discriminator, 130 popular queries, 3 001 niche candidates (ascending; the first 40 queries are candidates too), their device
    images and the fp64 oracle of those images -- computed once, shared by the tests, never written"""
    rng = np.random.default_rng(17)
    dv = Disc(_discriminator(hs, hot))
    c = np.sort(rng.choice(F, N_C, replace=False)).astype(np.int32)
    q = np.concatenate([rng.choice(c, 40, replace=False), rng.choice(np.setdiff1d(np.arange(F), c), N_Q - 40, replace=False)]).astype(np.int32)
    rng.shuffle(q)
    q_img, c_img = dv.pack("popular", q), dv.pack("niche", c)
    S = CR.score_ref(q_img.cpu().numpy(), c_img.cpu().numpy(), dv.D["w4"], dv.D["b4"])
    S.setflags(write=False)
    return dv, q, c, q_img, c_img, S


# ---------------------------------------------------------------------------------------------- 1. the side images
def _pack_bound(D, side, ids):
    """|x_dev - x| per (id, column), first order in u = 2^-24, from the layer lengths and the weights' absolute sums:
    branch pre-activation: an fmaf chain of h0 terms and the bias add        (h0 + 1) u (|e| |w| + |b|)
    its tanh: 1-Lipschitz, tanhf within 2 ulp of a value below 1              + 4 u
    fc half: that error through |w3|, an fmaf chain of hb terms, the bias     dt |w3| + (hb + 1) u (sum_i |w3[i][j]| + |b3[j]|)     (|t| <= 1)
    E = expf(2 x) within 1 ulp (relative 2^-23), read back as 0.5 log E       + u"""
    f = lambda a: np.abs(np.asarray(a, np.float64))
    h1 = D["w1"].shape[1]
    wb, bb, w3 = (D["w1"], D["b1"], D["w3"][:h1]) if side == "popular" else (D["w2"], D["b2"], D["w3"][h1:])
    b3 = np.zeros(D["w3"].shape[1]) if side == "popular" else f(D["b3"])
    h0, hb = wb.shape
    dt = (h0 + 1) * U * (f(D["emb"])[ids] @ f(wb) + f(bb)) + 4 * U
    return dt @ f(w3) + (hb + 1) * U * (f(w3).sum(0) + b3) + U


@pytest.mark.parametrize("side", ["popular", "niche"])
@pytest.mark.parametrize("hs,hot", [(SMALL, False), (CONFIG, False), (CONFIG, True)])
def test_pack_against_the_reference_within_the_derived_bound(hs, hot, side, capsys):
    rng = np.random.default_rng(3)
    dv = Disc(_discriminator(hs, hot))
    ids = rng.integers(0, F, N_C).astype(np.int32)
    ids[:3] = (0, F - 1, 0)                                        # the table's ends, a repeated id
    img = dv.pack(side, ids).cpu().numpy()
    h3 = hs[3]
    assert np.all(np.isfinite(img)) and np.all(img > 0)
    assert np.all(img[:, h3:] == 1.0), "padding columns are written as E(0) = 1"
    x = CR.pack_ref(dv.D, side, ids)
    assert np.abs(x).max() < CR.CLAMP
    err = np.abs(0.5 * np.log(img[:, :h3].astype(np.float64)) - x)
    bound = _pack_bound(dv.D, side, ids)
    with capsys.disabled():
        print("\n[companions] pack %s %s hot=%d: |x| <= %.2f, largest |x_dev - x| %.3e, smallest bound %.3e, largest error / bound %.3f" % (
            hs, side, hot, np.abs(x).max(), err.max(), bound.min(), (err / bound).max()))
    assert np.all(err <= bound), (float((err / bound).max()),)
    assert _eq(img[0], img[2])
    # an id's row has the same bits alone, at another place of a short list, and inside the 3 001
    for pos in (0, 1, 7, 8, 1500, N_C - 1):
        assert _eq(dv.pack(side, ids[pos:pos + 1]).cpu().numpy()[0], img[pos]), pos
    assert _eq(dv.pack(side, ids[[5, 1500, 9]]).cpu().numpy(), img[[5, 1500, 9]])


def test_pack_clamps_the_pre_activation():
    """w3 x 1 000: |x| reaches hundreds; every E is finite and positive, the saturated ones are expf(+-80) -- one value each"""
    D = _discriminator(SMALL, False)
    D["w3"] = D["w3"] * np.float32(1000.0)
    dv = Disc(D)
    ids = np.arange(0, 600, dtype=np.int32)
    for side in ("popular", "niche"):
        x = CR.pack_ref(D, side, ids)
        img = dv.pack(side, ids).cpu().numpy()[:, :SMALL[3]]
        hi, lo = x > CR.CLAMP + 1, x < -CR.CLAMP - 1
        assert hi.sum() > 100 and lo.sum() > 100 and np.all(np.isfinite(img)) and np.all(img > 0)
        for sel, want in ((hi, np.exp(80.0)), (lo, np.exp(-80.0))):
            v = np.unique(img[sel])
            assert v.size == 1 and abs(float(v[0]) / want - 1.0) <= 2.0 ** -22, (side, v)
        mid = np.abs(x) < CR.CLAMP - 1
        assert np.abs(0.5 * np.log(img[mid].astype(np.float64)) - x[mid]).max() < 1e-2
    # two saturated images multiply to inf or 0, never to inf x 0: the scores stay finite
    q, c = dv.pack("popular", ids[:17]), dv.pack("niche", ids)
    s, i = dv.companions(q, np.full(17, -1, np.int32), c, ids, 20)
    assert np.all(np.isfinite(s)) and np.all(i >= 0)
    S = CR.score_ref(q.cpu().numpy(), c.cpu().numpy(), D["w4"], D["b4"])
    assert np.abs(s - S[np.arange(17)[:, None], i]).max() <= dv.tol


def test_padding_columns_are_inert():
    """h3 = 37, ld = 40: whatever the three padding columns of either image hold -- NaN, inf, 0, garbage -- every score keeps its bits"""
    import torch
    dv, q, c, q_img, c_img, _ = _problem(SMALL, False)
    want = dv.companions(q_img, q, c_img, c, 20)
    for fill in (float("nan"), float("inf"), 0.0, -3e30):
        q2, c2 = q_img.clone(), c_img.clone()
        q2[:, SMALL[3]:] = fill
        c2[:, SMALL[3]:] = 1.0 if fill == 0.0 else fill
        got = dv.companions(q2, q, c2, c, 20)
        assert np.array_equal(got[1], want[1]) and _eq(got[0], want[0]), fill
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. scores and lists, real-valued
def _check_lists(got_s, got_i, S, q_gid, c_gid, k, tol):
    """every returned score within tol of the oracle at the returned id; every returned id's oracle score >= the k-th best oracle score
    among the eligible - 2 tol; ids distinct, eligible, never the query; ordered by (device score desc, id asc); padded at the end.
    -> the largest |score - oracle|"""
    ok = CR.eligible(q_gid, c_gid)
    worst = 0.0
    for r in range(len(q_gid)):
        ids = got_i[r]
        n = int((ids >= 0).sum())
        assert n == min(k, int(ok[r].sum())), (r, n)
        assert np.all(ids[n:] == -1) and np.all(np.isneginf(got_s[r, n:]))
        if n == 0:
            continue
        loc = np.searchsorted(c_gid, ids[:n])
        assert np.array_equal(c_gid[loc], ids[:n]) and np.unique(ids[:n]).size == n and np.all(ok[r, loc]) and not np.any(ids[:n] == q_gid[r]), r
        sc = got_s[r, :n]
        assert np.all((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (ids[:n][:-1] < ids[:n][1:]))), r
        err = np.abs(sc.astype(np.float64) - S[r, loc])
        worst = max(worst, float(err.max()))
        assert err.max() <= tol, (r, float(err.max()), tol)
        kth = np.sort(S[r, ok[r]])[::-1][n - 1]
        assert np.all(S[r, loc] >= kth - 2 * tol), r
    return worst


@pytest.mark.parametrize("k", [1, 20, 256])
@pytest.mark.parametrize("n_q", [1, 17, 130])
@pytest.mark.parametrize("hs,hot", [(SMALL, False), (CONFIG, False), (SMALL, True), (CONFIG, True)],
                         ids=["h3-37", "config", "h3-37-trained-range", "config-trained-range"])
def test_scores_and_lists_against_the_oracle_of_the_device_images(hs, hot, n_q, k, capsys):
    """tol = (8 + h3) 2^-24 (sum |w4| + |b4|): one 1-ulp expf per side, the product, the 1 + E, a 1-ulp v_rcp_f32 and the fma (<= 4 x 2^-24 per
    tanh, twice for the two sides' images), and a length-h3 fp32 sum.  Measured on an MI355X: at most 1.35e-6 against tol
    4.07e-4 (config.ini's sizes), 4.54e-6 against 8.10e-4 at a trained model's range, 4.2e-7 against 1.54e-5 at h3 = 37."""
    dv, q, c, q_img, c_img, S = _problem(hs, hot)
    got_s, got_i = dv.companions(q_img[:n_q].contiguous(), q[:n_q], c_img, c, k)
    with capsys.disabled():
        print("\n[companions] %s hot=%d n_q=%d k=%d: |score| <= %.2f, tol %.3e" % (hs, hot, n_q, k, np.abs(S).max(), dv.tol), end="")
    worst = _check_lists(got_s, got_i, S[:n_q], q[:n_q], c, k, dv.tol)
    with capsys.disabled():
        print(", largest |score - fp64 oracle| %.3e" % worst)
    if n_q == N_Q:
        assert np.any(got_i[:, 0] >= 0) and np.any(np.isin(q, c))           # (self-exclusion is exercised: 40 queries are candidates)


def test_niche_queries_over_popular_candidates_are_the_transposed_scores():
    """the kernel does not care which side is which: score(q, c) has the same bits either way round"""
    dv, q, c, q_img, c_img, _ = _problem(SMALL, False)
    A = dv.score_table(q_img[:40].contiguous(), c_img[:300].contiguous())
    B = dv.score_table(c_img[:300].contiguous(), q_img[:40].contiguous())
    assert _eq(A, B.T.copy())


# ---------------------------------------------------------------------------------------------- 3. order, bit for bit
@pytest.mark.parametrize("k", [1, 20, 256])
def test_zero_output_layer_gives_the_lowest_eligible_ids(k):
    """w4 = 0: every score is b4, bit for bit, and the lists are the k lowest eligible ids"""
    D = _discriminator(SMALL, False)
    D["w4"] = np.zeros_like(D["w4"])
    dv = Disc(D)
    _, q, c, _, _, _ = _problem(SMALL, False)
    q = q.copy()
    q[0] = c[0]                                                    # a query that is the lowest candidate starts at the next one
    got_s, got_i = dv.companions(dv.pack("popular", q), q, dv.pack("niche", c), c, k)
    b4 = np.float32(np.asarray(D["b4"]).reshape(-1)[0])
    want_s, want_i = CR.lists_ref(np.full((N_Q, N_C), b4, np.float32), q, c, k)
    assert np.array_equal(got_i, want_i) and _eq(got_s, want_s)
    assert want_i[0, 0] == c[1] and np.all(want_i[~np.isin(q, c), 0] == c[0])


@pytest.mark.parametrize("hs", [SMALL, CONFIG])
def test_duplicate_rows_tie_bitwise_and_break_by_id(hs):
    """candidate images with rows duplicated at scattered ids: equal bits against every query, broken by id -- the lists are numpy's order
    over the device's own score table, bit for bit, for every k; more duplicates of one row than k"""
    rng = np.random.default_rng(hs[0])
    dv = _problem(hs, False)[0]
    n_c = 1500
    emb_row = rng.integers(0, F, n_c).astype(np.int32)
    a, b = emb_row[5], emb_row[6]
    emb_row[rng.choice(n_c, 100, replace=False)] = b               # 100 copies of one row, then 400 of another, scattered
    emb_row[rng.choice(n_c, 400, replace=False)] = a
    c_gid = np.sort(rng.choice(100000, n_c, replace=False)).astype(np.int32)
    q_row = rng.integers(0, F, 50).astype(np.int32)
    q_gid = np.concatenate([c_gid[rng.choice(n_c, 25, replace=False)], np.full(25, -1)]).astype(np.int32)
    q_img, c_img = dv.pack("popular", q_row), dv.pack("niche", emb_row)
    S = dv.score_table(q_img, c_img)
    same = np.nonzero(emb_row == a)[0]
    assert same.size >= 400 and np.all(S[:, same].view(np.uint32) == S[:, same[:1]].view(np.uint32))
    for k in (1, 20, 256):
        got_s, got_i = dv.companions(q_img, q_gid, c_img, c_gid, k)
        want_s, want_i = CR.lists_ref(S, q_gid, c_gid, k)
        assert np.array_equal(got_i, want_i) and _eq(got_s, want_s), k


def test_fewer_eligible_than_k_pads():
    dv, q, c, q_img, c_img, S = _problem(SMALL, False)
    sel = np.array([3, 500, 501, 1999, 3000])
    qs = np.concatenate([np.nonzero(np.isin(q, c))[0][:2], np.nonzero(~np.isin(q, c))[0][:2]])
    q_gid = q[qs].copy()
    q_gid[0] = c[500]                                              # a query that excludes one of the five
    for k in (1, 5, 20, 256):
        got_s, got_i = dv.companions(q_img[qs].contiguous(), q_gid, c_img[sel].contiguous(), c[sel], k)
        n = (got_i >= 0).sum(1)
        assert n.tolist() == [min(k, 4)] + [min(k, 5 - int(g in c[sel])) for g in q_gid[1:]]
        _check_lists(got_s, got_i, S[qs][:, sel], q_gid, c[sel], k, dv.tol)
    # no candidates at all: all-padding lists
    import torch
    got_s, got_i = dv.companions(q_img[:7].contiguous(), q[:7], torch.empty(0, dv.ld, dtype=torch.float32, device="cuda"), np.zeros(0, np.int32), 20)
    assert np.all(got_i == -1) and np.all(np.isneginf(got_s))


# ---------------------------------------------------------------------------------------------- 4. position independence
@pytest.mark.parametrize("hs", [SMALL, CONFIG])
def test_position_independence(hs):
    """the candidates in ragged parts (1, 127, 1 024, the rest), each run alone and joined by ltg_topk_merge, against one call; a query run
    alone against the same query inside the chunk of 130; two runs -- all bit for bit"""
    import torch
    dv, q, c, q_img, c_img, _ = _problem(hs, False)
    lib = dv.lib
    edges = [0, 1, 128, 1152, N_C]
    for k in (20, 256):
        want_s, want_i = dv.companions(q_img, q, c_img, c, k)
        again = dv.companions(q_img, q, c_img, c, k)
        assert np.array_equal(again[1], want_i) and _eq(again[0], want_s), "two runs differ"
        ps, pi = [], []
        for a, b in zip(edges[:-1], edges[1:]):
            s, i = dv.companions(q_img, q, c_img[a:b].contiguous(), c[a:b], k)
            assert np.all((i == -1) | ((i >= c[a]) & (i <= c[b - 1])))
            ps.append(s)
            pi.append(i)
        ps, pi = torch.from_numpy(np.stack(ps)).cuda(), torch.from_numpy(np.stack(pi)).cuda()
        so = torch.empty(N_Q, k, dtype=torch.float32, device="cuda")
        io = torch.empty(N_Q, k, dtype=torch.int32, device="cuda")
        rc = lib.ltg_topk_merge(len(edges) - 1, N_Q, k, ps.data_ptr(), pi.data_ptr(), k, so.data_ptr(), io.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(io.cpu().numpy(), want_i) and _eq(so.cpu().numpy(), want_s), ("parts", k)
        for r in (0, 1, 31, 32, 77, N_Q - 1):
            s, i = dv.companions(q_img[r:r + 1].contiguous(), q[r:r + 1], c_img, c, k)
            assert np.array_equal(i[0], want_i[r]) and _eq(s[0], want_s[r]), ("alone", k, r)
        s, i = dv.companions(q_img[40:57].contiguous(), q[40:57], c_img, c, k)
        assert np.array_equal(i, want_i[40:57]) and _eq(s, want_s[40:57]), ("chunk of 17", k)


# ---------------------------------------------------------------------------------------------- 5. it is the discriminator
def _moved_engine(hs, I=2000):
    """an Engine whose discriminator has been moved by a few D steps (and the generator by a G step, which must leave D alone)"""
    import torch
    from ltgan.engine import CsrRows, Engine, Pairs
    rng = np.random.default_rng(1)
    eng = Engine(I, h_sizes=hs, lr=1e-2, precision="bf16", seed=1234, d_seed=5)
    dev = eng.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pairs = lambda n: Pairs(t(rng.integers(0, I, n).astype(np.int32)), t(rng.integers(0, I, n).astype(np.int32)))
    for st in range(3):
        eng.d_step(pairs(300), pairs(280), 0.7, rng_step=10 + st)
    B = 16
    X = Hh.random_history(rng, B, I, mean_nnz=9)
    slot, uptr, rowidx, pos, nu = Hh.csc_view(X)
    batch = CsrRows(t(X.indptr.astype(np.int32)), t(X.indices.astype(np.int32)), 0, B, slot=t(slot), uptr=t(uptr), rowidx=t(rowidx), csr_pos=t(pos),
                    n_unique=nu)
    rows = np.repeat(np.arange(B, dtype=np.int32), 2)
    fake = Pairs(t(rng.integers(0, I, 2 * B).astype(np.int32)), t(rng.integers(0, I, 2 * B).astype(np.int32)), t(rows))
    eng.g_step(batch, fake, eng.new_acts(B), torch.tensor([2 * B], dtype=torch.int32, device=dev), anneal=0.1, rng_step=3, d_rng_step=4)
    eng.d_step(pairs(300), pairs(280), 0.7, rng_step=20)
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("hs", [SMALL, CONFIG])
def test_it_is_the_discriminator(hs, capsys):
    """sigmoid(score) of the returned (query, id) pairs against ltg_fake_tower_batched at d_keep_prob = 1 (everything kept) on an engine moved
    by D and G steps: tol / 4 (sigmoid's slope) + the tower's own forward tolerance, 2e-6 (test_forward_only_tower_matches_oracle); and
    against the oracle's tower on the engine's weights"""
    import torch
    from ltgan.engine import Pairs
    eng = _moved_engine(hs)
    I, k = eng.I, 20
    D = _engine_discriminator(eng)
    assert all(np.abs(D[key]).max() > 0 for key in ("b1", "b2", "b3", "b4")), "the D steps moved the biases"
    tol = (8 + hs[3]) * U * (float(np.abs(D["w4"].astype(np.float64)).sum()) + abs(float(D["b4"].reshape(-1)[0])))
    rng = np.random.default_rng(2)
    q = rng.choice(I, 64, replace=False).astype(np.int32)
    c = np.sort(rng.choice(I, 1500, replace=False)).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    s = torch.empty(64, k, dtype=torch.float32, device=eng.device)
    i = torch.empty(64, k, dtype=torch.int32, device=eng.device)
    eng.pair_companions(eng.pair_pack("popular", t(q)), t(q), eng.pair_pack("niche", t(c)), t(c), k, s, i)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy()
    assert np.all(i >= 0)
    pop, nic = np.repeat(q, k).astype(np.int32), i.reshape(-1).astype(np.int32)
    n = pop.size
    y = torch.full((n,), -1.0, dtype=torch.float32, device=eng.device)
    eng.fake_tower_batched(Pairs(t(pop), t(nic)), t(np.zeros(n, np.int32)), t(np.zeros(1, np.int32)), t(np.array([77], np.int64)), y, 1.0)
    torch.cuda.synchronize()
    y = y.cpu().numpy().astype(np.float64)
    mine = 1.0 / (1.0 + np.exp(-s.reshape(-1)))
    ones = [np.ones((n, w)) for w in hs[1:]]
    T = O.d_tower(D, pop, nic, ones, 1.0)
    with capsys.disabled():
        print("\n[companions] %s: |sigmoid(score) - tower| %.3e (bound %.3e), |score - oracle| %.3e (tol %.3e), |tower - oracle| %.3e" % (
            hs, np.abs(mine - y).max(), tol / 4 + 2e-6, np.abs(s.reshape(-1) - T["s"]).max(), tol, np.abs(y - T["y"]).max()))
    assert np.abs(mine - y).max() <= tol / 4 + 2e-6
    # the oracle on the WEIGHTS: the kernel's tol plus what the two fp32 images add -- tanh is 1-Lipschitz, so |w4| . (pack bounds)
    images = float(np.abs(D["w4"].astype(np.float64)).reshape(-1) @ (_pack_bound(D, "popular", q).max(0) + _pack_bound(D, "niche", c).max(0)))
    assert np.abs(s.reshape(-1) - T["s"]).max() <= tol + images


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing():
    """every LTG_EINVAL / LTG_EWORKSPACE case (tests/test_companions_cpu.check_refusals) on device buffers that must keep their sentinel"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    buf = torch.full((1 << 16,), 1234.5, dtype=torch.float32, device="cuda")
    TC.check_refusals(cabi, lib, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 1234.5).all()) and torch.cuda.current_stream().query()


# ---------------------------------------------------------------------------------------------- 7. host layer
def test_pair_companions_class_equals_the_calls_and_the_reference():
    import torch
    from ltgan.engine import Engine
    from ltgan.trainer import PairCompanions
    I = 3000
    eng = Engine(I, h_sizes=SMALL, lr=1e-3, precision="bf16", seed=3, d_seed=9)
    D = _engine_discriminator(eng)
    dv = Disc(D)
    rng = np.random.default_rng(4)
    niche = np.sort(rng.choice(I, 900, replace=False)).astype(np.int32)
    popular = np.setdiff1d(np.arange(I), niche).astype(np.int32)
    for side, q, c, k in (("popular", popular[:333], niche, 20), ("niche", niche[::7], popular, 256), ("popular", np.array([5, 5, 2999, 0], np.int32), niche[:7], 20)):
        pc = PairCompanions(eng, k=k, queries=side, chunk=100)           # several chunks, the last short
        ids, scores = pc.run(q, c)
        assert ids.shape == scores.shape == (len(q), k) and ids.dtype == np.int32 and scores.dtype == np.float32
        other = "niche" if side == "popular" else "popular"
        q_img, c_img = dv.pack(side, q), dv.pack(other, c)
        want_s, want_i = dv.companions(q_img, q, c_img, c, k)
        assert np.array_equal(ids, want_i) and _eq(scores, want_s), (side, k)
        _check_lists(scores, ids, CR.score_ref(q_img.cpu().numpy(), c_img.cpu().numpy(), D["w4"], D["b4"]), q, c, k, dv.tol)
    e_ids, e_scores = PairCompanions(eng, k=5).run(np.zeros(0, np.int32), niche)
    assert e_ids.shape == e_scores.shape == (0, 5)
    with pytest.raises(ValueError, match="ascending"):
        PairCompanions(eng).run(popular[:3], niche[::-1])
    with pytest.raises(ValueError, match="outside"):
        PairCompanions(eng).run(np.array([I], np.int32), niche)
    with pytest.raises(ValueError, match="outside"):
        PairCompanions(eng).run(popular[:3], np.array([-1, 4], np.int32))
    with pytest.raises(ValueError):
        PairCompanions(eng, k=257)
    with pytest.raises(ValueError):
        PairCompanions(eng, queries="all")
    torch.cuda.synchronize()


def test_companions_cli_equals_the_class(tmp_path):
    import torch
    from ltgan import companions as CP
    from ltgan import data_processing as dp
    from ltgan.trainer import PairCompanions
    ds, cwd, n_items, eng, ck, _, _, _ = askubuntu_run(tmp_path, split=None)
    show2id, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(ds, "item2id.txt"), os.path.join(ds, "item_list.txt"),
                                                     os.path.join(ds, "niche_items.txt"), n_items)
    valid = dp.load_valid_item_ids(os.path.join(ds, "item_list.txt"), show2id)
    side, q, cand = CP.split_sides("popular", niche, valid, n_items)
    assert side == "popular" and q.size and cand.size and not np.intersect1d(q, cand).size
    want_i, want_s = PairCompanions(eng, k=10).run(q, cand)
    torch.cuda.synchronize()

    def summary(out):
        last = [l for l in out if l.startswith("items: ")][-1]
        return dict(x.split(": ") for x in last.split("\t"))

    f = summary(run_cli("companions.py", [ds, ck, "--k", "10", "--out", "c.tsv", "--npz", "c.npz"], cwd))
    z = np.load(os.path.join(cwd, "c.npz"))
    assert np.array_equal(z["items"], q) and np.array_equal(z["ids"], want_i) and _eq(z["scores"], want_s)
    rows = open(os.path.join(cwd, "c.tsv")).read().splitlines()
    assert len(rows) == q.size
    for n, line in enumerate(rows):
        sid, rest = line.split("\t")
        ent = [e.split(":") for e in rest.split(",")] if rest else []
        assert int(sid) == q[n] and [int(e[0]) for e in ent] == [i for i in want_i[n].tolist() if i >= 0]
        assert all(len(e[1]) == 8 and abs(float(e[1]) - 1.0 / (1.0 + np.exp(-float(s)))) <= 5.1e-7 for e, s in zip(ent, want_s[n]))
    m = CP.companions_summary(want_i, want_s, cand.size)
    assert int(f["items"]) == q.size and abs(float(f["coverage@10"]) - m["coverage"]) < 1e-6 and abs(float(f["mean_prob@1"]) - m["mean_prob"]) < 1e-6
    assert 0.0 < float(f["coverage@10"]) <= 1.0 and 0.0 < float(f["mean_prob@1"]) < 1.0
    # two ranks (gloo, one GPU), candidates sharded by item slab: the same table bit for bit
    out2 = run_cli("companions.py", [ds, ck, "--k", "10", "--out", "c2.tsv", "--npz", "c2.npz"], cwd, world=2, limit=900)
    z2 = np.load(os.path.join(cwd, "c2.npz"))
    assert np.array_equal(z2["ids"], want_i) and _eq(z2["scores"], want_s)
    assert open(os.path.join(cwd, "c2.tsv")).read() == open(os.path.join(cwd, "c.tsv")).read()
    assert summary(out2) == f


@pytest.mark.parametrize("world", [2])
def test_sharded_pair_companions(world):
    run_ranks("dist_companions_worker.py", ["5003"], world, "COMPANIONS_SHARDED_OK world=%d" % world)
