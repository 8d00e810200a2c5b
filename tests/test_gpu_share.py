"""Share-targeted top-K lists on the GPU: ltg_topk_share against the reference of tests/share_ref.py -- ids, score bits and the whole
state block (the definition is integer comparisons of 64-bit words and one fp32 subtraction, so it is held bit for bit) -- on synthetic
Zipf lists at a row shorter than a wave, k = 1, quantised scores whose threshold cost is shared by more than a thousand steps, 1 024-entry
rows, k off the wave size, 150 000 words and a 3 000 x 100 split; the targets at and beyond the ends, lists longer than k, empty and short
lists, entries behind the padding and a -0.0 cost; the properties of the device output that need no reference; the comparison with
ltg_topk_quota at the same promoted total; Recommender(share=) against the entry point called by hand, with a LongTailReport reading the
final lists; the item-sharded recommender (tests/dist_share_worker.py) and both CLIs on Askubuntu_Sample in fresh child processes."""
import ctypes
import os
import re

import numpy as np
import pytest

import share_ref as S
from serving_harness import DEV, _bits, _t, askubuntu_run, run_cli, run_ranks

pytestmark = pytest.mark.gpu

#        n,    I,    k,    c,  share, quant
SHAPES = [(64, 40, 5, 40, 0.3, None),                     # a row shorter than a wave
          (200, 300, 1, 300, 0.3, None),                  # k = 1
          (777, 129, 10, 129, 0.4, 0.5),                  # 1 337 words share the threshold's cost, 237 costs are zero: the low 32 bits decide
          (64, 2200, 1024, 2200, 0.55, None),             # the longest row
          (130, 70, 33, 70, 0.6, None),                   # k off the wave size
          (1500, 300, 100, 200, 0.4, None),               # 150 000 words over many workgroups
          (3000, 1000, 100, 400, 0.3, None)]              # the largest case


_CASES = {}


def case(t):
    """the lists of shape t, their target and the reference at that target, built once and left unchanged"""
    if t not in _CASES:
        n, I, k, c, share, quant = SHAPES[t]
        ps, pi, rs, ri, _ = S.share_case(n, I, k, c, quant=quant)
        want = int(np.ceil(np.float64(share) * n * k))
        _CASES[t] = (ps, pi, rs, ri, k, want, S.share_lists(ps, pi, rs, ri, k, want))
    return _CASES[t]


def share_dev(ps, pi, rs, ri, k, want, poison=True):
    """one ltg_topk_share through the C ABI on host arrays -> host (scores, ids, state [8])"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, m_in = pi.shape
    st = torch.cuda.current_stream().cuda_stream
    d = [_t(np.asarray(ps, np.float32)), _t(np.asarray(pi, np.int32)), _t(np.asarray(rs, np.float32)), _t(np.asarray(ri, np.int32))]
    need = lib.ltg_share_ws_bytes(n, k)
    assert need > 0
    ws = torch.full((need,), 0xA5 if poison else 0, dtype=torch.uint8, device=DEV)        # nothing relies on a zeroed workspace
    state = torch.full((cabi.LTG_SHARE_STATE,), -9, dtype=torch.int32, device=DEV)
    so = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
    io = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    assert lib.ltg_topk_share(n, m_in, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), k, int(want), so.data_ptr(),
                              io.data_ptr(), state.data_ptr(), ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), io.cpu().numpy(), state.cpu().numpy()


def check_against_reference(ps, pi, rs, ri, k, want, what, ref=None):
    wS, wI, wst, ex = ref if ref is not None else S.share_lists(ps, pi, rs, ri, k, want)
    gS, gI, st = share_dev(ps, pi, rs, ri, k, want)
    print("%s: want %d, state %s (reference %s), steps per row %d distinct values" % (what, want, st.tolist(), wst.tolist(), len(np.unique(ex["t"]))))
    assert np.array_equal(st, wst), (what, st, wst)
    bad = np.nonzero((gI != wI).any(1))[0]
    assert bad.size == 0, (what, bad[:5], gI[bad[:1]], wI[bad[:1]])
    assert np.array_equal(_bits(gS), _bits(wS)), what
    return gS, gI, st


def promoted_count(ids, pi):
    """how many entries of the table come from the promoted lists"""
    return sum(int(np.isin(ids[u][ids[u] >= 0], pi[u][:S.list_len(pi[u])]).sum()) for u in range(len(ids)))


# ---------------------------------------------------------------------------------------------- 1. parity with the reference
@pytest.mark.parametrize("t", range(len(SHAPES)))
def test_parity_with_the_reference(t):
    ps, pi, rs, ri, k, want, ref = case(t)
    st, ex = ref[2], ref[3]
    # the case counts: on the reference the threshold binds, at least a quarter of the rows change, t_u takes at least two values
    assert 0 < st[2] < st[1] and st[3] * 4 >= len(pi) and len(np.unique(ex["t"])) >= 2, (SHAPES[t], st)
    check_against_reference(ps, pi, rs, ri, k, want, SHAPES[t], ref)


def test_the_quantised_case_decides_in_the_low_bits():
    ps, pi, rs, ri, k, want, ref = case(2)
    st, ex = ref[2], ref[3]
    costs = np.concatenate(ex["words"]) >> np.uint64(32)
    at_thr = int((costs == np.uint64(np.uint32(st[4]))).sum())
    taken_at_thr = int(st[2]) - int((costs < np.uint64(np.uint32(st[4]))).sum())
    assert at_thr == 1337 and int((costs == 0).sum()) == 237 and 0 < taken_at_thr < at_thr


# ---------------------------------------------------------------------------------------------- 2. edge cases against the reference
def test_targets_at_and_beyond_the_ends():
    ps, pi, rs, ri, k, _, _ = case(4)
    pS, pI, pst, _ = S.share_lists(ps, pi, rs, ri, k, 0)
    A, N = int(pst[0]), int(pst[1])
    for want in (0, 1, A):                               # a target the plain lists meet: the plain lists, bit for bit
        gS, gI, st = check_against_reference(ps, pi, rs, ri, k, want, "want %d <= A" % want)
        assert np.array_equal(gI, pI) and np.array_equal(_bits(gS), _bits(pS)) and st[2:5].tolist() == [0, 0, 0]
    full = None
    for want in (A + N, A + N + 1, 2 ** 31 + 5, 2 ** 62):  # every row at its limit, the threshold does not bind
        gS, gI, st = check_against_reference(ps, pi, rs, ri, k, want, "want %d >= A + N" % want)
        assert st[2] == N
        full = (gS, gI, st) if full is None else full
        assert np.array_equal(gI, full[1]) and np.array_equal(_bits(gS), _bits(full[0])) and np.array_equal(st, full[2])
    check_against_reference(ps, pi, rs, ri, k, A + 1, "one step")
    check_against_reference(ps, pi, rs, ri, k, A + N - 1, "all steps but one")


def test_lists_longer_than_k():
    for n, I, k, c, m_in, share in ((130, 70, 7, 70, 40, 0.5), (300, 400, 20, 400, 150, 0.35), (64, 1500, 100, 1500, 1024, 0.4)):
        ps, pi, rs, ri, _ = S.share_case(n, I, k, c, m_in=m_in)
        assert pi.shape == (n, m_in)
        want = int(np.ceil(share * n * k))
        _, _, st = check_against_reference(ps, pi, rs, ri, k, want, "m_in %d > k %d" % (m_in, k))
        assert 0 < st[2] < st[1]


def test_empty_and_short_lists_and_entries_behind_the_padding():
    n, I, k, c = 150, 90, 12, 90
    ps, pi, rs, ri, _ = S.share_case(n, I, k, c, m_in=20)
    ps, pi, rs, ri = ps.copy(), pi.copy(), rs.copy(), ri.copy()
    rng = np.random.default_rng(0)
    pi[0:10, :], ps[0:10, :] = -1, -np.inf               # no promoted list
    ri[5:15, :], rs[5:15, :] = -1, -np.inf               # no rest list; rows 5 .. 9: both empty
    for u in range(20, 60):                              # np + nr < k
        cp, cr = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        pi[u, cp:], ps[u, cp:], ri[u, cr:], rs[u, cr:] = -1, -np.inf, -1, -np.inf
    for u in range(40, 100):                             # entries behind the padding: ids and finite scores that must be ignored
        for ids, sc in ((pi, ps), (ri, rs)):
            cut = S.list_len(ids[u])
            if cut < 19:
                ids[u, cut] = -1 - int(rng.integers(0, 3))
                ids[u, cut + 1:] = rng.integers(0, I, 19 - cut)
                sc[u, cut:] = rng.standard_normal(20 - cut).astype(np.float32) + 5
    _, _, full, _ = S.share_lists(ps, pi, rs, ri, k, 2 ** 40)
    A, N = int(full[0]), int(full[1])
    for want in (0, A + N // 3, A + N, A + N + 7):
        gS, gI, st = check_against_reference(ps, pi, rs, ri, k, want, "short lists, want %d" % want)
        assert (gI[5:10] == -1).all() and np.isneginf(gS[5:10]).all()                   # both lists empty: an empty row
    assert 0 < N // 3 < N


def test_a_minus_zero_cost_sorts_first():
    """rest = -0.0 against promoted = +0.0: the fp32 difference is -0.0, whose bits would sort after every other cost"""
    ps = np.array([[0.0, -9.0], [1.0, -9.0]], np.float32)
    pi = np.array([[1, -1], [1, -1]], np.int32)
    rs = np.array([[-0.0, -9.0], [1.5, -9.0]], np.float32)
    ri = np.array([[0, -1], [0, -1]], np.int32)
    gS, gI, st = check_against_reference(ps, pi, rs, ri, 1, 1, "-0.0")
    assert gI[:, 0].tolist() == [1, 0] and st.tolist() == [0, 2, 1, 1, 0, 2, 0, 0]
    assert _bits(gS[:, 0]).tolist() == _bits(np.array([0.0, 1.5], np.float32)).tolist()
    gS, gI, st = check_against_reference(ps, pi, rs, ri, 1, 2, "-0.0, both")
    assert gI[:, 0].tolist() == [1, 1] and st[4] == int(np.float32(0.5).view(np.int32))


# ---------------------------------------------------------------------------------------------- 3. the device output on its own
@pytest.mark.parametrize("t", range(len(SHAPES)))
def test_properties_of_the_device_output(t):
    ps, pi, rs, ri, k, want, _ = case(t)
    n = len(pi)
    gS, gI, st = share_dev(ps, pi, rs, ri, k, want)
    A, N = int(st[0]), int(st[1])
    assert want >= A and promoted_count(gI, pi) == min(want, A + N) == A + st[2]
    for u in range(n):                                   # ltg_topk's order, distinct ids, every score the original bits
        got = gI[u][gI[u] >= 0]
        assert len(got) == min(k, S.list_len(pi[u]) + S.list_len(ri[u])) and len(set(got.tolist())) == len(got), u
        assert (gI[u, len(got):] == -1).all() and np.isneginf(gS[u, len(got):]).all(), u
        w = S.order_words(gS[u, :len(got)], got)
        assert (w[1:] < w[:-1]).all(), u
        src = {int(g): s for ids, sc in ((pi[u], ps[u]), (ri[u], rs[u])) for g, s in zip(ids[:S.list_len(ids)], _bits(sc))}
        assert [src[int(g)] for g in got] == _bits(gS[u, :len(got)]).tolist(), u
    for kw in (dict(), dict(poison=False)):              # twice, and with a zeroed workspace: the same bits
        gS2, gI2, st2 = share_dev(ps, pi, rs, ri, k, want, **kw)
        assert np.array_equal(gI2, gI) and np.array_equal(_bits(gS2), _bits(gS)) and np.array_equal(st2, st), kw


# ---------------------------------------------------------------------------------------------- 4. against MinSlots at the same total
@pytest.mark.parametrize("t,M", [(0, 2), (4, 20), (5, 30)])
def test_cheaper_than_min_slots_at_the_same_promoted_total(t, M):
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    ps, pi, rs, ri, k, _, _ = case(t)
    n = len(pi)
    pS, pI, pst, ex = S.share_lists(ps, pi, rs, ri, k, 0)                # the plain lists: the merge, cut to k
    st = torch.cuda.current_stream().cuda_stream
    d = [_t(pS), _t(pI), _t(ps), _t(pi)]
    qo_s = torch.empty(n, k, dtype=torch.float32, device=DEV)
    qo_i = torch.empty(n, k, dtype=torch.int32, device=DEV)
    quota = (ctypes.c_int32 * 1)(M)
    assert lib.ltg_topk_quota(n, k, d[0].data_ptr(), d[1].data_ptr(), 1, k, d[2].data_ptr(), d[3].data_ptr(), quota, k, qo_s.data_ptr(),
                              qo_i.data_ptr(), st) == 0
    torch.cuda.synchronize()
    q_ids = qo_i.cpu().numpy()
    p_u = np.array([int(np.isin(q_ids[u][q_ids[u] >= 0], pi[u][:S.list_len(pi[u])]).sum()) for u in range(n)])
    t_min = p_u - ex["a"]                                # the steps MinSlots makes every row take
    assert (t_min >= 0).all() and (t_min <= [len(w) for w in ex["words"]]).all() and t_min.sum() > 0
    T = int(p_u.sum())
    gS, gI, gst = share_dev(ps, pi, rs, ri, k, T)
    assert promoted_count(gI, pi) == T == gst[0] + gst[2]
    _, _, _, ex_t = S.share_lists(ps, pi, rs, ri, k, T)
    ours, theirs = S.step_cost(ex_t["words"], ex_t["t"]), S.step_cost(ex["words"], t_min)
    print("shape %s quota %d: promoted %d, step cost %.6g (share) vs %.6g (min slots)" % (SHAPES[t], M, T, float(ours), float(theirs)))
    assert ours <= theirs and not np.array_equal(ex_t["t"], t_min)


# ---------------------------------------------------------------------------------------------- 5. the host layer
@pytest.mark.parametrize("I", [1001, 1537])
def test_recommender_with_share(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import Calibrate, Diversify, ExposureCap, LongTailReport, MinSlots, Recommender, ShareTarget
    rng = np.random.default_rng(I)
    n, k = 300, 100
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    # test_recommender_with_cap's output bias of log Zipf popularity: the plain lists pile onto a head, and the users still differ
    acts0 = eng.new_acts(n)
    eng.forward(ev.rows(0, n)[0], acts0, keep_prob=1.0, is_training=0.0, rng_step=77)
    sigma = float(acts0.logits[:n].std(dim=0).mean())
    bias = (-sigma * np.log(np.arange(1, I + 1)))[rng.permutation(I)].astype(np.float32)
    eng.g_p[7].copy_(_t(bias))
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=1.0)
    hits = np.bincount(plain_ids[plain_ids >= 0], minlength=I)
    labels = np.where(hits <= np.median(hits), 1, rng.choice([0, 2], I)).astype(np.uint8)      # group 1 = the tail; label 2 is in no group
    # share = 0: the plain table bit for bit, and the sizes of the problem
    zero = ShareTarget(labels, 2, [1], 0.0)
    ids0, sc0 = Recommender(eng, ev, k=k, chunk=128, share=zero).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids0, plain_ids) and np.array_equal(_bits(sc0), _bits(plain_sc))
    z = zero.stats()
    assert z["taken"] == 0 and z["rows_changed"] == 0 and z["price"] == 0.0 and z["reached"] and z["share"] == z["plain_share"]
    A = int(round(z["plain_share"] * n * k))
    assert A == int(np.isin(plain_ids, np.nonzero(labels == 1)[0]).sum()) and z["available"] > 100
    share = (A + z["available"] // 3) / (n * k)          # a target a third of the way from the plain share to the limit: it binds
    tgt = ShareTarget(labels, 2, [1], share)
    rep = LongTailReport(labels, 2)
    ids, sc = Recommender(eng, ev, k=k, chunk=128, share=tgt, report=rep).run(rng_step=77, keep_prob=1.0)
    # by hand: per chunk the forward and two ltg_topk_groups lists (the last chunk is short), then the entry point
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
    p_s, p_i, r_s, r_i, w_s, w_i = new(n, k), new(n, k, dt=torch.int32), new(n, k), new(n, k, dt=torch.int32), new(n, k), new(n, k, dt=torch.int32)
    acts, lab_d = eng.new_acts(128), _t(labels)
    for lo in range(0, n, 128):
        hi = min(n, lo + 128)
        tr, _ = ev.rows(lo, hi)
        eng.forward(tr, acts, keep_prob=1.0, is_training=0.0, rng_step=77 + lo)
        eng.topk_groups(acts, tr, k, lab_d, 0b10, p_s[lo:hi], p_i[lo:hi])
        eng.topk_groups(acts, tr, k, lab_d, 0x1FF & ~0b10, r_s[lo:hi], r_i[lo:hi])
    want = int(np.ceil(np.float64(share) * n * k))
    state, ws = new(8, dt=torch.int32), new(eng.share_ws_bytes(n, k), dt=torch.uint8)
    eng.topk_share(p_s, p_i, r_s, r_i, k, want, w_s, w_i, state, ws)
    torch.cuda.synchronize()
    assert tgt.want == want and np.array_equal(ids, w_i.cpu().numpy()) and np.array_equal(_bits(sc), _bits(w_s.cpu().numpy()))
    assert torch.equal(tgt.state, state) and torch.equal(tgt.pro_i, p_i) and torch.equal(tgt.rest_s.view(torch.int32), r_s.view(torch.int32))
    # ... and the reference on the gathered lists
    wS, wI, wst, ex = S.share_lists(p_s.cpu().numpy(), p_i.cpu().numpy(), r_s.cpu().numpy(), r_i.cpu().numpy(), k, want)
    assert np.array_equal(ids, wI) and np.array_equal(_bits(sc), _bits(wS)) and np.array_equal(state.cpu().numpy(), wst)
    st = tgt.stats()
    print("I %d: %s" % (I, st))
    assert 0 < st["taken"] < st["available"] and st["reached"] and st["rows_changed"] == int((ex["t"] > 0).sum()) > 0
    assert st["plain_share"] == wst[0] / wst[5] and st["share"] == (wst[0] + wst[2]) / wst[5] >= share > st["plain_share"]
    assert st["target"] == share and st["price"] == float(np.array([wst[4]], np.int32).view(np.float32)[0]) > 0
    assert int(np.isin(ids, np.nonzero(labels == 1)[0]).sum()) == want and not np.array_equal(ids, plain_ids)
    # the report read the final lists: ltg_topk_metrics over them, chunk by chunk, and its item_hits is their bincount
    rep2 = LongTailReport(labels, 2)
    rep2.bind(eng, n, k)
    ids_d = _t(ids)
    for lo in range(0, n, 128):
        hi = min(n, lo + 128)
        rep2.add(eng, ids_d[lo:hi], ev.rows(lo, hi)[1], lo)
    (o1, h1), (o2, h2) = rep.table(), rep2.table()
    assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(h1, h2) and np.array_equal(h1, np.bincount(ids[ids >= 0], minlength=I))
    # a target out of reach: every row at its limit, and the stats say so
    far = ShareTarget(labels, 2, [1], 1.0)
    ids1, _ = Recommender(eng, ev, k=k, chunk=128, share=far).run(rng_step=77, keep_prob=1.0)
    f = far.stats()
    assert f["taken"] == f["available"] == z["available"] and f["reached"] == (A + f["available"] >= n * k)
    good = ShareTarget(labels, 2, [1], share)
    for kw in (dict(diversify=Diversify(0.3)), dict(rule=MinSlots(labels, 3, [0, 5, 5])), dict(calibrate=Calibrate(labels, 2, 0.5)),
               dict(cap=ExposureCap(60))):
        with pytest.raises(ValueError):
            Recommender(eng, ev, k=k, chunk=128, share=good, **kw)
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=0, chunk=128, share=good)
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recommender_with_share(world):
    run_ranks("dist_share_worker.py", ["1001", "230"], world, "SHARE_SHARDED_OK world=%d" % world)


def test_clis_on_askubuntu(tmp_path):
    import torch
    from ltgan import longtail as lt
    ds, cwd, n_items, _, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    n_users = tr.shape[0]
    labels, names = lt.build_groups(ds, "niche", 2, n_items)
    assert names[1] == "niche"

    def share_line(line):
        m = re.fullmatch(r"share@100: (\S+) (\d\.\d{6}) -> (\d\.\d{6}) \(target (\d\.\d{6})\), (\d+) rows changed, price (\S+)", line)
        assert m, line
        return (m.group(1),) + tuple(float(x) for x in m.groups()[1:4]) + (int(m.group(5)), float(m.group(6)))

    def tsv_share(path):
        lines = open(path).read().splitlines()
        assert len(lines) == n_users
        slots = niche = 0
        for n, line in enumerate(lines):
            u, _, items = line.partition("\t")
            items = [int(x) for x in items.split(",")] if items else []
            assert int(u) == uid0 + n and len(items) == len(set(items)) <= 100 and (not items or (min(items) >= 0 and max(items) < n_items))
            slots += len(items)
            niche += int((labels[items] == 1).sum())
        return niche / slots

    out = run_cli("recommend.py", [ds, ck, "--share", "niche:0", "--out", "plain.tsv"], cwd)     # the plain lists: where the share stands
    print(out[-1])
    name, before, after, target, changed, price = share_line(out[-1])
    assert (name, after, target, changed, price) == ("niche", before, 0.0, 0, 0.0)
    assert "%.6f" % tsv_share(os.path.join(cwd, "plain.tsv")) == "%.6f" % before
    goal = min(1.0, round(before + 0.1, 3))              # ten points more of every slot for the niche items
    out = run_cli("recommend.py", [ds, ck, "--share", "niche:%.3f" % goal, "--out", "share.tsv"], cwd)
    assert out[-2].startswith("users: %d\tniche_share@100: " % n_users)
    print(out[-1])
    name, before2, after, target, changed, price = share_line(out[-1])
    assert name == "niche" and before2 == before and target == goal
    reached = "%.6f" % tsv_share(os.path.join(cwd, "share.tsv"))
    assert reached == "%.6f" % after                     # the line reports what the TSV holds
    assert after >= target and changed > 0 and price > 0   # the niche items of this catalogue can fill the target: it is reached
    out = run_cli("longtail.py", [ds, ck, "--share", "niche:%.3f" % goal, "--groups", "niche"], cwd)
    print(out[-1])
    assert share_line(out[-1]) == (name, before, after, target, changed, price)           # the same lists, whichever CLI serves them
    assert out[-2].startswith("all\t") and len(out[-2].split("\t")) == 9
    assert out[-3].startswith("niche\t") and out[-3].split("\t")[6] == "%.6f" % after     # the report read the final lists
    torch.cuda.synchronize()
