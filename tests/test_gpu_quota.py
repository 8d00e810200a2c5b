"""Minimum slots per item group on the GPU, ids and score bits exactly against numpy (tests/quota_ref.py: lexsort over the admitted
items; the greedy walk over the full row): ltg_topk_groups on the injected rows of test_gpu_topk, ltg_topk_quota on reference lists,
Recommender(rule=) on the logits of a real forward with a LongTailReport reading the ruled lists, the item-sharded recommender
(tests/dist_quota_worker.py) and both CLIs on Askubuntu_Sample in fresh child processes.  Nothing is recomputed, so there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import quota_ref as Q
from serving_harness import DEV, _t, askubuntu_run, run_cli, run_ranks
from topk_ref import _csr, _eq, _reference, _rows, _topk_dev

pytestmark = pytest.mark.gpu


def _groups_dev(logits, indptr, indices, k, labels, mask, item_lo=0):
    """ltg_topk_groups on a [rows, I] device tensor through the C ABI; labels: device uint8 of the whole catalogue"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, I = logits.shape
    cfg = cabi.ltg_config(I, 600, 200, I, 100, 150, 250, 300, 0, 0, item_lo, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    tr = None
    if indptr is not None:
        tr = cabi.ltg_batch(n, 0, indptr.data_ptr(), indices.data_ptr() if indices.numel() else indptr.data_ptr())
    s = torch.full((n, k), 7.0, dtype=torch.float32, device=logits.device)
    i = torch.full((n, k), -7, dtype=torch.int32, device=logits.device)
    rc = lib.ltg_topk_groups(C.byref(cfg), logits.data_ptr(), C.byref(tr) if tr is not None else None, n, k, labels.data_ptr(),
                             labels.numel(), mask, s.data_ptr(), i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _quota_dev(sa, ia, sg, ig, quota, k):
    """ltg_topk_quota through the C ABI on host arrays -> host arrays"""
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    n, k_in = ia.shape
    n_lists, _, m_in = ig.shape
    d = [_t(sa.astype(np.float32)), _t(ia.astype(np.int32)), _t(sg.astype(np.float32)), _t(ig.astype(np.int32))]
    so = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
    io = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    q = (C.c_int32 * n_lists)(*[int(x) for x in quota])
    rc = lib.ltg_topk_quota(n, k_in, d[0].data_ptr(), d[1].data_ptr(), n_lists, m_in, d[2].data_ptr(), d[3].data_ptr(), q, k, so.data_ptr(),
                            io.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return so.cpu().numpy(), io.cpu().numpy()


def _labels(rng, n, G, absent):
    """labels random in 0 .. G (G = in no group), a few far beyond (9, 255: bit 8), none equal to `absent`"""
    lab = rng.integers(0, G + 1, n).astype(np.uint8)
    stray = rng.random(n) < 0.03
    lab[stray] = rng.choice(np.array([9, 255], np.uint8), int(stray.sum()))
    lab[lab == absent] = (absent + 1) % (G + 1)
    return lab


def _filtered(orders, L, labels, mask, k, item_lo=0):
    """the reference lists from the rows' full rankings (computed once per catalogue size)"""
    bit = np.minimum(labels, 8).astype(np.int64)
    return Q.lists(L, None, lambda r: orders[r][((mask >> bit[orders[r] + item_lo]) & 1) == 1], k, item_lo)


@pytest.mark.parametrize("I", [1000, 1001, 25024, 200000])
def test_topk_groups_matches_lexsort_of_the_admitted_items(I):
    rng = np.random.default_rng(I + 1)
    L, folds = _rows(rng, I, 1024)
    Ld = _t(L)
    ptr, idx = _csr(folds, DEV)
    orders = [Q.ranked(L[r], folds[r]) for r in range(L.shape[0])]
    for G in (2, 4, 8):
        absent = 7 if G < 8 else 5                                     # a label no item carries: its list is all padding
        labels = _labels(rng, I, G, absent)
        lab_d = _t(labels)
        masks = [1 << g for g in range(G) if g != absent] + [(1 << 0) | (1 << (G - 1)), 0x100, 1 << absent, 0x1FF]
        for k in (1, 100, 1024):
            plain = _topk_dev(Ld, ptr, idx, k)
            for mask in masks:
                S, ID = _groups_dev(Ld, ptr, idx, k, lab_d, mask)
                wS, wID = _filtered(orders, L, labels, mask, k)
                assert np.array_equal(ID, wID), (I, G, k, hex(mask), np.nonzero((ID != wID).any(1))[0])
                assert _eq(S, wS), (I, G, k, hex(mask))
                if mask == 0x1FF:                                      # ltg_topk on the same rows, bit for bit
                    assert np.array_equal(ID, plain[1]) and _eq(S, plain[0])
                if mask == 1 << absent:
                    assert (ID == -1).all() and np.isneginf(S).all()
                if mask == 0x100:
                    assert (ID >= 0).any() and (labels[ID[ID >= 0]] >= 8).all()
            S, ID = _groups_dev(Ld, ptr, idx, k, lab_d, masks[0])
            S2, ID2 = _groups_dev(Ld, ptr, idx, k, lab_d, masks[0])    # twice in a row: the same bits
            assert np.array_equal(ID2, ID) and _eq(S2, S)
            Sn, IDn = _groups_dev(Ld, None, None, k, lab_d, masks[0])  # tr = None: only the labels exclude
            wS, wID = Q.masked_lists(L[:4], None, labels, masks[0], k)
            assert np.array_equal(IDn[:4], wID) and _eq(Sn[:4], wS)


def test_topk_groups_on_a_ragged_slab_reads_the_labels_at_item_lo():
    I_glob, a, b = 25024, 12345, 12345 + 6001                          # item_lo and the slab's size: neither a multiple of 4
    rng = np.random.default_rng(7)
    L, folds = _rows(rng, b - a, 100)
    labels = _labels(rng, I_glob, 4, 7)
    Ld, lab_d = _t(L), _t(labels)
    ptr, idx = _csr(folds, DEV)
    orders = [Q.ranked(L[r], folds[r], a) for r in range(L.shape[0])]
    for k in (1, 100, 1024):
        for mask in (1, 4, 0x110, 0x1FF):
            S, ID = _groups_dev(Ld, ptr, idx, k, lab_d, mask, item_lo=a)
            wS, wID = _filtered(orders, L, labels, mask, k, item_lo=a)
            assert np.array_equal(ID, wID) and _eq(S, wS), (k, hex(mask))
        wS, wID = _reference(L, folds, k, item_lo=a)
        assert np.array_equal(ID, wID) and _eq(S, wS)                  # 0x1FF == the plain reference


def _quota_case(L, folds, labels, groups, quota, k, k_in, m_in):
    """reference input lists for the reserved groups -> ltg_topk_quota's output, and the greedy walk over the full rows"""
    sa, ia = Q.masked_lists(L, folds, labels, 0x1FF, k_in)
    g = [Q.masked_lists(L, folds, labels, 1 << grp, m_in) for grp in groups]
    S, ID = _quota_dev(sa, ia, np.stack([x[0] for x in g]), np.stack([x[1] for x in g]), quota, k)
    full = [0] * 8
    for grp, q in zip(groups, quota):
        full[grp] = q
    wS, wID = Q.greedy_lists(L, folds, labels, full, k)
    assert np.array_equal(ID, wID), (groups, quota, k, k_in, m_in, np.nonzero((ID != wID).any(1))[0])
    assert _eq(S, wS), (groups, quota, k, k_in, m_in)
    return ID, sa, ia, g


@pytest.mark.parametrize("I", [1000, 3001])
def test_topk_quota_matches_the_greedy_walk(I):
    rng = np.random.default_rng(I)
    L, folds = _rows(rng, I, 100)                                     # incl. the all-equal row, 50 eligible items, none at all
    labels = rng.integers(0, 9, I).astype(np.uint8)                    # 8 groups and "no group"
    labels[np.nonzero(labels == 3)[0][25:]] = 4                        # group 3 is small: 25 items, fewer than its quota below
    n3 = [int((labels[Q.ranked(L[r], folds[r])] == 3).sum()) for r in range(L.shape[0])]
    assert 0 < max(n3) < 40
    # all quotas 0: the plain list's first k
    ID, sa, ia, _ = _quota_case(L, folds, labels, [1], [0], 100, 100, 1)
    assert np.array_equal(ID, ia)
    ID, sa, ia, _ = _quota_case(L, folds, labels, list(range(8)), [0] * 8, 60, 100, 5)               # k_in > k, n_lists 8
    assert np.array_equal(ID, ia[:, :60])
    # one quota == k: that group's list
    ID, _, _, g = _quota_case(L, folds, labels, [2], [100], 100, 100, 100)
    full = (g[0][1] >= 0).all(1)
    assert full.any() and np.array_equal(ID[full], g[0][1][full])
    # a group with fewer eligible items than its quota hands the rest to the free slots; m_in larger than the quota
    ID, _, _, _ = _quota_case(L, folds, labels, [3, 0], [40, 10], 100, 128, 64)
    assert ((ID >= 0).sum(1) == np.minimum(100, [len(Q.ranked(L[r], folds[r])) for r in range(L.shape[0])])).all()
    # the all-equal row (row 1): the tie runs across every quota boundary, lower ids win inside a group
    row = ID[1]
    assert (np.diff(row) > 0).all() and np.array_equal(row[labels[row] == 3], Q.ranked(L[1], folds[1])[labels[Q.ranked(L[1], folds[1])] == 3][:40])
    # eight reserved lists, quotas summing to k exactly; and k = k_in = 1024
    _quota_case(L, folds, labels, list(range(8)), [12, 13, 12, 13, 12, 13, 12, 13], 100, 100, 13)
    _quota_case(L, folds, labels, [7, 1, 4], [300, 1, 200], 1000, 1024, 300)
    if I > 1024:
        _quota_case(L, folds, labels, [0, 5], [1024, 0], 1024, 1024, 1024)
    _quota_case(L, folds, labels, [6], [1], 1, 1, 1)                   # k = 1


def _n_eligible(X, labels, g):
    """per user: the items of group g that are not fold-in items"""
    sel = (labels == g)
    return int(sel.sum()) - np.asarray(X[:, np.nonzero(sel)[0]].getnnz(axis=1)).ravel()


@pytest.mark.parametrize("I", [1000, 25024])
def test_recommender_with_rule_on_forward_logits(I):
    import torch
    import helpers as Hh
    from ltgan.dataset import EvalData
    from ltgan.engine import Engine
    from ltgan.trainer import LongTailReport, MinSlots, Recommender
    rng = np.random.default_rng(2)
    n, k = 300, 100
    X = Hh.random_history(rng, n, I, mean_nnz=15)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=9)
    ev = EvalData(X, X, eng.device)
    labels = rng.integers(0, 4, I).astype(np.uint8)                    # groups 0..2, label 3 in no group
    slots = [0, 25, 10]
    for g in (1, 2):
        assert _n_eligible(X, labels, g).min() >= slots[g]             # every user can be served: the inequality below is not vacuous
    plain_ids, plain_sc = Recommender(eng, ev, k=k, chunk=128).run(rng_step=77, keep_prob=1.0)
    for kp in (0.75, 1.0):
        rep = LongTailReport(rng.integers(0, 2, I).astype(np.uint8), 2)        # rule and report are independent: other labels
        rec = Recommender(eng, ev, k=k, chunk=128, rule=MinSlots(labels, 3, slots), report=rep)
        ids, sc = rec.run(rng_step=77, keep_prob=kp)
        L = rec.acts.logits[: n - 256].cpu().numpy()                   # the short last chunk's logits: rows 256 .. 299
        folds = [X.indices[X.indptr[r]:X.indptr[r + 1]] for r in range(256, n)]
        wS, wID = Q.greedy_lists(L, folds, labels, slots, k)
        assert np.array_equal(ids[256:], wID) and _eq(sc[256:], wS), kp
        assert np.array_equal(rep.table()[1], np.bincount(ids.ravel(), minlength=I))     # the report read the ruled lists
        ids2, sc2 = Recommender(eng, ev, k=k, chunk=128, rule=MinSlots(labels, 3, slots)).run(rng_step=77, keep_prob=kp)
        assert np.array_equal(ids2, ids) and _eq(sc2, sc)              # run to run, and the report changes nothing
        for g in (1, 2):
            assert ((labels[ids] == g).sum(1) >= slots[g]).all()
    assert not np.array_equal(ids, plain_ids)                          # (keep_prob 1.0) the rule moved something
    # all-zero slots: rule=None bit for bit
    ids0, sc0 = Recommender(eng, ev, k=k, chunk=128, rule=MinSlots(labels, 3, [0, 0, 0])).run(rng_step=77, keep_prob=1.0)
    assert np.array_equal(ids0, plain_ids) and _eq(sc0, plain_sc)
    # with a report on the rule's own labels: item_hits summed over group g >= n_users * slots[g]
    rep = LongTailReport(labels, 3)
    Recommender(eng, ev, k=k, chunk=128, rule=MinSlots(labels, 3, slots), report=rep).run(rng_step=77)
    hits = rep.table()[1]
    assert hits.sum() == n * k
    for g in (1, 2):
        assert hits[labels == g].sum() >= n * slots[g], (g, hits[labels == g].sum())
    with pytest.raises(ValueError):
        Recommender(eng, ev, k=30, chunk=128, rule=MinSlots(labels, 3, slots))      # 35 slots in a list of 30
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recommender_with_rule(world):
    run_ranks("dist_quota_worker.py", ["custom:1001", "230"], world, "QUOTA_SHARDED_OK world=%d" % world)


def test_clis_on_askubuntu(tmp_path):
    import torch
    from ltgan import longtail as lt
    from ltgan.dataset import EvalData
    from ltgan.trainer import LongTailReport, Recommender
    ds, cwd, n_items, eng, ck, tr, te, uid0 = askubuntu_run(tmp_path)
    labels, names = lt.build_groups(ds, "pop", 4, n_items)
    assert names[3] == "pop3" and _n_eligible(tr.tocsr(), labels, 3).min() >= 30        # the minimum this test relies on
    out = run_cli("recommend.py", [ds, ck, "--groups", "pop:4", "--min-slots", "pop3:30", "--out", "ruled.tsv"], cwd)
    assert out[-1].startswith("users: %d\tniche_share@100: " % tr.shape[0])
    lines = open(os.path.join(cwd, "ruled.tsv")).read().splitlines()
    assert len(lines) == tr.shape[0]
    least = 100
    for n, line in enumerate(lines):
        u, items = line.split("\t")
        items = np.array([int(x) for x in items.split(",")])
        assert int(u) == uid0 + n and len(items) == 100 == len(set(items.tolist())) and items.min() >= 0 and items.max() < n_items
        least = min(least, int((labels[items] == 3).sum()))
    print("fewest pop3 items in a list: %d" % least)
    assert least >= 30
    # longtail.py: the pop3 row's share@100 under the rule; without --min-slots today's lines, those of Recommender(report=) without a rule
    ruled = run_cli("longtail.py", [ds, ck, "--groups", "pop:4", "--min-slots", "pop3:30"], cwd)[-6:]
    pop3 = [l.split("\t") for l in ruled if l.startswith("pop3\t")][0]
    print("pop3 under the rule: %s" % pop3)
    assert len(pop3) == 8 and float(pop3[6]) >= 0.30
    assert len(ruled[0].split("\t")) == 3 and ruled[-1].startswith("all\t") and len(ruled[-1].split("\t")) == 9
    plain = run_cli("longtail.py", [ds, ck, "--groups", "pop:4"], cwd)[-6:]
    rep = LongTailReport(labels, 4, k_exp=100)
    Recommender(eng, EvalData(tr, te, eng.device), k=rep.k, report=rep).run(rng_step=2 * 10 ** 9)
    want = lt.report_lines(lt.aggregate(*rep.table(), labels, names, 100))
    assert plain == want, (plain, want)
    torch.cuda.synchronize()
