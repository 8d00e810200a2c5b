"""Worker of tests/test_serving_cpu.py (CPU tensors, no GPU): SlabLists, MinSlots.apply, Diversify.apply and the one chunk walk of
Recommender / ShardedRecommender driven with a fake engine that implements topk / topk_groups / topk_merge with torch ops, stubs the rest
and records every call; the collectives of torch.distributed are recorded into the same log.  Under torch.distributed.run (gloo, world
size 2) main() checks the item-sharded side; unsharded() needs no process group and is also called by the test file in-process.

150 items: item_slab gives slabs of 128 and 22, the uneven last slab.  Logits: a row-wise permutation of arange(150) as float32, every
score distinct and exact.  8 users in chunks of 5: a full chunk and a short last one of 3 rows, on buffers bound for 5 rows."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_ITEMS, N_USERS, ROWS, STEP = 150, 8, 5, 1000
LABELS = (np.arange(N_ITEMS) % 3).astype(np.uint8)          # three item groups; every slab holds items of each
LOG = []                                                    # every engine call and every collective, in order


def full_logits():
    g = torch.Generator().manual_seed(7)
    return torch.stack([torch.randperm(N_ITEMS, generator=g) for _ in range(N_USERS)]).float()


def reference(logits, L, mask=None):
    """torch.topk on the full-catalogue logits, only the items whose group the mask admits -> (scores, int32 ids)"""
    x = logits.clone()
    if mask is not None:
        admit = torch.from_numpy(((mask >> LABELS.astype(np.int64)) & 1).astype(bool))
        x[:, ~admit] = -float("inf")
    v, i = torch.topk(x, L, dim=1)
    return v, i.int()


class _Rows:
    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi


class FakeEval:
    n = N_USERS

    def rows(self, lo, hi):
        return _Rows(lo, hi), _Rows(lo, hi)


class _Acts:
    def __init__(self, rows, n_items):
        self.logits = torch.zeros(rows, n_items)
        self.h1 = torch.zeros(rows, 4)


class FakeEngine:
    """the Engine calls the serving layer makes, on CPU tensors; `dst` keeps where topk / topk_groups / topk_merge were told to write"""
    device = "cpu"

    def __init__(self, lo=0, hi=N_ITEMS, rank=0, world=1):
        self.item_lo, self.item_hi, self.I, self.I_global = lo, hi, hi - lo, N_ITEMS
        self.rank, self.world = rank, world
        self.full = full_logits()
        self.dst = []

    def new_acts(self, rows):
        return _Acts(rows, self.I)

    def _fill(self, tr, acts):
        acts.logits[: tr.hi - tr.lo] = self.full[tr.lo:tr.hi, self.item_lo:self.item_hi]

    def forward(self, tr, acts, keep_prob=0.75, is_training=0.0, rng_step=0):
        LOG.append(("forward", rng_step))
        self._fill(tr, acts)

    def fwd_opts(self, keep_prob=0.75, is_training=0.0, rng_step=0):
        LOG.append(("fwd_opts", rng_step))
        return rng_step

    def g_fwd_enc(self, tr, acts, fo):
        LOG.append(("g_fwd_enc",))
        acts.h1.fill_(-1.0)
        acts.h1[: tr.hi - tr.lo] = float(self.rank + 1)      # this slab's part of the pre-activation

    def g_fwd_rest(self, tr, fake, acts, fo, rowpart):
        LOG.append(("g_fwd_rest",))
        n = tr.hi - tr.lo
        assert fake is None and rowpart.numel() >= 5 * n
        assert torch.all(acts.h1[:n] == float(sum(range(1, self.world + 1)))) and torch.all(acts.h1[n:] == -1.0)   # all-reduced, these rows only
        self._fill(tr, acts)

    def _topk(self, acts, L, labels, mask, score_out, id_out):
        n = int(score_out.shape[0])
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, L) and score_out.is_contiguous() and id_out.is_contiguous()
        x = acts.logits[:n].clone()
        if mask is not None:
            lab = labels[self.item_lo:self.item_hi].long()
            x[:, ((mask >> lab) & 1) == 0] = -float("inf")
        v, i = torch.topk(x, L, dim=1)
        score_out.copy_(v)
        id_out.copy_(torch.where(v > -float("inf"), i + self.item_lo, torch.full_like(i, -1)).int())
        self.dst.append((score_out.data_ptr(), id_out.data_ptr()))

    def topk(self, acts, tr, k, score_out, id_out):
        LOG.append(("topk", k))
        self._topk(acts, k, None, None, score_out, id_out)

    def topk_groups(self, acts, tr, k, labels, group_mask, score_out, id_out):
        LOG.append(("topk_groups", k, group_mask))
        self._topk(acts, k, labels, group_mask, score_out, id_out)

    def topk_merge(self, score_in, id_in, k, score_out, id_out):
        parts, n, k_in = (int(x) for x in score_in.shape)
        LOG.append(("topk_merge", parts, k_in, k))
        assert score_in.is_contiguous() and id_in.is_contiguous() and tuple(id_in.shape) == (parts, n, k_in)
        assert tuple(score_out.shape) == tuple(id_out.shape) == (n, k) and score_out.is_contiguous() and id_out.is_contiguous()
        v, j = torch.topk(score_in.permute(1, 0, 2).reshape(n, parts * k_in), k, dim=1)
        score_out.copy_(v)
        id_out.copy_(id_in.permute(1, 0, 2).reshape(n, parts * k_in).gather(1, j))
        self.dst.append((score_out.data_ptr(), id_out.data_ptr()))

    def topk_quota(self, score_all, id_all, score_grp, id_grp, quota, score_out, id_out):
        LOG.append(("topk_quota", tuple(quota)))
        score_out.copy_(score_all[:, : score_out.shape[1]])
        id_out.copy_(id_all[:, : id_out.shape[1]])

    def topk_diversify(self, image, image_lo, score_in, id_in, lam, k, score_out, id_out, stat_out=None):
        LOG.append(("topk_diversify", int(score_in.shape[1]), k))
        assert tuple(image.shape) == (N_ITEMS, 608) and bool(torch.all(image == 1)) and tuple(stat_out.shape) == (score_in.shape[0], 2)
        score_out.copy_(score_in[:, :k])
        id_out.copy_(id_in[:, :k])

    def topk_metrics(self, ids, te, labels, n_groups, out, item_hits, **cut):
        LOG.append(("topk_metrics",))

    def item_pack(self, space="decoder", metric="cosine", out=None):
        LOG.append(("item_pack",))
        if out is None:
            out = torch.empty(self.I, 608, dtype=torch.int16)
        assert tuple(out.shape) == (self.I, 608)
        return out.fill_(1)


def record_collectives():
    def wrap(name, which):
        real = getattr(dist, name)

        def fn(*a, **k):
            LOG.append((name, str(a[which].dtype).replace("torch.", "")))
            return real(*a, **k)
        setattr(dist, name, fn)
    wrap("all_gather", 1)
    wrap("all_reduce", 0)


def taken():
    out = list(LOG)
    del LOG[:]
    return out


def equal_lists(got_s, got_i, want):
    return torch.equal(got_s, want[0]) and torch.equal(got_i, want[1])


def modes():
    """-> {name: keyword arguments of a Recommender}: k = 7 with the rule (reserved lists of m = 4), k = 4 diversified out of 7 candidates"""
    from ltgan.trainer import Diversify, MinSlots
    return {"plain": lambda: dict(k=7),
            "rule": lambda: dict(k=7, rule=MinSlots(LABELS, 3, [2, 0, 4])),
            "rule0": lambda: dict(k=7, rule=MinSlots(LABELS, 3, [0, 0, 0])),
            "diversify": lambda: dict(k=4, diversify=Diversify(0.5, candidates=7))}


def report():
    from ltgan.trainer import LongTailReport
    return LongTailReport(LABELS, 3, k_ndcg=4, k_r1=2, k_r2=3, k_exp=4)


def check_tables(name, rec, full):
    """what run() left behind: the table (the stubs of quota / diversify keep the head of the plain list / of the candidates), and the
    merged lists of the short last chunk where the rule and the re-ranking read them"""
    want = reference(full, rec.k)
    assert equal_lists(rec.scores, rec.ids, want), name
    last = full[ROWS:]
    if name.startswith("rule"):
        assert equal_lists(*rec.rule.plain(N_USERS - ROWS, 7), reference(last, 7)), name
    if name == "rule":
        g_s, g_i = rec.rule.reserved(N_USERS - ROWS)
        for j, g in enumerate((0, 2)):
            assert equal_lists(g_s[j], g_i[j], reference(last, 4, 1 << g)), (name, g)
    if name == "diversify":
        assert equal_lists(*rec.diversify.candidates_of(N_USERS - ROWS), reference(last, 7)), name
        assert tuple(rec.diversify.image.shape) == (N_ITEMS, 608) and bool(torch.all(rec.diversify.image == 1))


# ---- the expected sequences, written out from the code before SlabLists: Recommender.run / MinSlots.apply / Diversify.apply (unsharded) and
# ShardedRecommender.run / ._ruled / ._diversified (item shards, R ranks) -- per chunk whose first row is `lo`, then the report's launch if any
UNSHARDED = {
    "plain": lambda lo: [("forward", STEP + lo), ("topk", 7)],
    "rule": lambda lo: [("forward", STEP + lo), ("topk", 7), ("topk_groups", 4, 1), ("topk_groups", 4, 4), ("topk_quota", (2, 4))],
    "rule0": lambda lo: [("forward", STEP + lo), ("topk", 7)],
    "diversify": lambda lo: [("forward", STEP + lo), ("topk", 7), ("topk_diversify", 7, 4)],
}
UNSHARDED_ONCE = {"plain": [], "rule": [], "rule0": [], "diversify": [("item_pack",)]}

SHARDED_FORWARD = lambda lo: [("fwd_opts", STEP + lo), ("g_fwd_enc",), ("all_reduce", "float32"), ("g_fwd_rest",)]      # noqa: E731
SHARDED = {
    "plain": lambda lo, R: SHARDED_FORWARD(lo) + [("topk", 7), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7)],
    "rule": lambda lo, R: SHARDED_FORWARD(lo) + [("topk", 7), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7),
                                                 ("topk_groups", 4, 1), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 4, 4),
                                                 ("topk_groups", 4, 4), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 4, 4),
                                                 ("topk_quota", (2, 4))],
    "rule0": lambda lo, R: SHARDED_FORWARD(lo) + [("topk", 7), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7)],
    "diversify": lambda lo, R: SHARDED_FORWARD(lo) + [("topk", 7), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7),
                                                      ("topk_diversify", 7, 4)],
}
SHARDED_ONCE = {"plain": [], "rule": [], "rule0": [], "diversify": [("item_pack",), ("all_reduce", "int32")]}


def unsharded():
    """parts == 1: every list is written straight into its destination, no gather buffer exists, and the calls are the direct ones"""
    from ltgan.serving import SlabLists
    from ltgan.trainer import Recommender
    del LOG[:]
    eng = FakeEngine()
    full = eng.full
    lists = SlabLists(eng, rows=ROWS, longest=7)
    assert lists.parts == 1 and lists.loc_s is lists.loc_i is lists.part_s is lists.part_i is None
    acts, labels = eng.new_acts(ROWS), torch.from_numpy(LABELS)
    for lo, hi in ((0, ROWS), (ROWS, N_USERS)):
        n = hi - lo
        eng.forward(_Rows(lo, hi), acts, rng_step=STEP + lo)
        for L, mask in ((7, None), (4, 1 << 2), (7, 1 << 0), (4, None)):
            s, i = torch.empty(n, L), torch.empty(n, L, dtype=torch.int32)
            lists.topk(acts, None, n, L, s, i, labels, mask)
            assert equal_lists(s, i, reference(full[lo:hi], L, mask)), (lo, L, mask)
            assert eng.dst[-1] == (s.data_ptr(), i.data_ptr())            # the engine wrote the outputs themselves
    assert not [c for c in taken() if c[0] in ("topk_merge", "all_gather", "all_reduce")]
    for name, kw in modes().items():
        for rep in (None, report()):
            eng = FakeEngine()
            rec = Recommender(eng, FakeEval(), chunk=ROWS, report=rep, **kw())
            assert rec.lists.part_s is None and rec.lists.loc_s is None and rec.chunk == ROWS
            taken()
            rec.run(rng_step=STEP)
            tail = [("topk_metrics",)] if rep is not None else []
            assert taken() == UNSHARDED_ONCE[name] + UNSHARDED[name](0) + tail + UNSHARDED[name](ROWS) + tail, (name, rep is not None)
            check_tables(name, rec, full)
            if name == "plain":                                          # straight into the table, chunk by chunk
                assert eng.dst == [(rec.scores[lo:].data_ptr(), rec.ids[lo:].data_ptr()) for lo in (0, ROWS)]
            if name == "rule":                                           # ... and into the rule's own arrays
                g_s, g_i = rec.rule.reserved(N_USERS - ROWS)
                assert eng.dst[-3:] == [(t.data_ptr(), u.data_ptr()) for t, u in (rec.rule.plain(N_USERS - ROWS, 7), (g_s[0], g_i[0]), (g_s[1], g_i[1]))]


def main():
    from ltgan.serving import SlabLists
    from ltgan.sharded import ShardedRecommender, item_slab
    dist.init_process_group("gloo")
    rank, R = dist.get_rank(), dist.get_world_size()
    record_collectives()
    lo_i, hi_i = item_slab(N_ITEMS, rank, R)
    assert R == 2 and (lo_i, hi_i) == ((0, 128), (128, 150))[rank]
    eng = FakeEngine(lo_i, hi_i, rank, R)
    full = eng.full
    # ---- SlabLists on its own: lists of 7 and of 4 entries alternate on ONE set of buffers, full chunk and short last chunk
    lists = SlabLists(eng, rows=ROWS, longest=7, parts=R)
    assert lists.loc_s.numel() == lists.loc_i.numel() == ROWS * 7 and lists.part_s.numel() == lists.part_i.numel() == R * ROWS * 7
    acts, labels = eng.new_acts(ROWS), torch.from_numpy(LABELS)
    for lo, hi in ((0, ROWS), (ROWS, N_USERS)):
        n = hi - lo
        eng.forward(_Rows(lo, hi), acts, rng_step=STEP + lo)
        taken()
        for L, mask in ((7, None), (4, 1 << 2), (7, 1 << 0), (4, None)):
            s, i = torch.empty(n, L), torch.empty(n, L, dtype=torch.int32)
            lists.topk(acts, None, n, L, s, i, labels, mask)
            assert equal_lists(s, i, reference(full[lo:hi], L, mask)), (rank, lo, L, mask)
            first = ("topk", L) if mask is None else ("topk_groups", L, mask)
            assert taken() == [first, ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, L, L)]
        # merge() alone (ShardedItemNeighbors: the local lists come from another kernel), from where local() says they go
        s, i = torch.empty(n, 4), torch.empty(n, 4, dtype=torch.int32)
        ls, li = lists.local(n, 4, s, i)
        assert ls.data_ptr() == lists.loc_s.data_ptr() and ls.is_contiguous() and tuple(ls.shape) == (n, 4)
        eng.topk(acts, None, 4, ls, li)
        lists.merge(ls, li, s, i)
        assert equal_lists(s, i, reference(full[lo:hi], 4))
        assert taken() == [("topk", 4), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 4, 4)]
    # ---- the chunk walk over item shards: every mode, without and with a report
    for name, kw in modes().items():
        for rep in (None, report()):
            eng = FakeEngine(lo_i, hi_i, rank, R)
            rec = ShardedRecommender(eng, FakeEval(), chunk=ROWS, report=rep, **kw())
            assert rec.chunk == ROWS and rec.lists.parts == R and rec.lists.part_s.numel() == R * ROWS * 7
            assert not hasattr(rec.rule, "part_s") and not hasattr(rec.diversify, "part_s")
            taken()
            rec.run(rng_step=STEP)
            tail = [("topk_metrics",)] if rep is not None else []
            assert taken() == SHARDED_ONCE[name] + SHARDED[name](0, R) + tail + SHARDED[name](ROWS, R) + tail, (rank, name, rep is not None)
            check_tables(name, rec, full)
    unsharded()                                                          # (with the collectives recorded: there are none)
    dist.barrier()
    if rank == 0:
        print("SERVING_CPU_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
