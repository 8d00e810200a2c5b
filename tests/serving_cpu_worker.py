"""Worker of tests/test_serving_cpu.py (CPU tensors, no GPU): SlabLists, every serve-time rule (minimum slots, diversified, calibrated,
capped, share-targeted, floored), the audience, the report and the explanations on the one chunk walk of Recommender / ShardedRecommender,
driven with a fake engine that implements topk / topk_groups / topk_merge with torch ops, stubs the rest and records every call; the
collectives of torch.distributed are recorded into the same log.  Under torch.distributed.run (gloo, world
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
        self.lse = torch.zeros(rows)


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
        acts.lse.fill_(-1.0)
        acts.lse[: tr.hi - tr.lo] = torch.arange(tr.lo, tr.hi).float()      # "lse" of a row = its row number in the split

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
        acts.lse.fill_(-1.0)                                  # a slab's forward leaves no full-row lse: rowstats_combine writes it
        part = rowpart[: 5 * n].view(n, 5).zero_()
        part[:, 0] = torch.arange(tr.lo, tr.hi).float()       # this slab's row partial

    def rowstats_combine(self, rowpart_all, n_ranks, n_rows, lse_out):
        LOG.append(("rowstats_combine", n_ranks, n_rows))
        assert n_ranks == self.world and rowpart_all.numel() == n_ranks * n_rows * 5
        lse_out[:n_rows] = rowpart_all.view(n_ranks, n_rows, 5)[:, :, 0].sum(0) / n_ranks      # every slab's partial arrived

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

    def hist_groups(self, tr, labels, n_groups, count_out, hist_lo=None):
        LOG.append(("hist_groups", n_groups))
        assert hist_lo == (self.item_lo if self.world > 1 else 0) and tuple(count_out.shape) == (tr.hi - tr.lo, n_groups + 1)
        count_out.fill_(1)                                    # every slab counts 1 everywhere: all-reduced, `world`

    def topk_calibrate(self, score_grp, id_grp, list_class, n_groups, hist, lam, k, score_out, id_out, stat_out=None):
        LOG.append(("topk_calibrate", tuple(list_class), k))
        assert bool(torch.all(hist == self.world)) and tuple(stat_out.shape) == (score_grp.shape[1], 2)
        score_out.copy_(score_grp[0][:, :k])
        id_out.copy_(id_grp[0][:, :k])

    def cap_ws_bytes(self, n_rows, c_in, n_items=None):
        LOG.append(("cap_ws_bytes", n_rows, c_in, n_items))
        return 64

    def cap_index(self, cand_i, n_items, state, ws):
        LOG.append(("cap_index", int(cand_i.shape[1]), n_items))
        state.zero_()

    def cap_rounds(self, cand_s, cand_i, lse, cap, k, n_rounds, state, ws):
        LOG.append(("cap_rounds", lse is not None, k, n_rounds))
        state[1] += n_rounds                                  # state[4] stays 0: no round raised a threshold, converged

    def cap_finish(self, cand_s, cand_i, n_items, k, score_out, id_out, state, ws):
        LOG.append(("cap_finish", k))
        score_out.copy_(cand_s[:, :k])
        id_out.copy_(cand_i[:, :k])

    def share_ws_bytes(self, n_rows, k):
        LOG.append(("share_ws_bytes", n_rows, k))
        return 64

    def topk_share(self, score_pro, id_pro, score_rest, id_rest, k, want, score_out, id_out, state, ws):
        LOG.append(("topk_share", k, want))
        score_out.copy_(score_rest[:, :k])
        id_out.copy_(id_rest[:, :k])

    def floor_ws_bytes(self, n_rows, c_in, n_items=None):
        LOG.append(("floor_ws_bytes", n_rows, c_in, n_items))
        return 64

    def floor_index(self, cand_i, n_items, state, ws):
        LOG.append(("floor_index", int(cand_i.shape[1]), n_items))
        state.zero_()

    def floor_rounds(self, cand_s, cand_i, lse, need, k, reserve, n_rounds, state, ws):
        LOG.append(("floor_rounds", lse is not None, k, reserve, n_rounds))
        state[1] += n_rounds                                  # state[4] stays 0: no round lowered a limit, converged

    def floor_finish(self, cand_s, cand_i, lse, need, k, reserve, score_out, id_out, state, ws, active_out=None, held_out=None):
        LOG.append(("floor_finish", lse is not None, k, reserve))
        score_out.copy_(cand_s[:, :k])
        id_out.copy_(cand_i[:, :k])

    def topk_explain(self, image, image_lo, tr, id_in, top, r, score_out, id_out):
        LOG.append(("topk_explain", top, r))
        n = tr.hi - tr.lo
        assert tuple(image.shape) == (N_ITEMS, 608) and bool(torch.all(image == 1)) and tuple(id_out.shape) == (n, top, r)
        score_out.copy_((-torch.arange(r).float() - r * self.rank).expand(n, top, r))     # merged over the slabs: rank 0's reasons
        id_out.copy_(id_in[:, :top, None] * 10 + torch.arange(r, dtype=torch.int32))

    def item_audience_ws_bytes(self, n_rows, n_q, k):
        return 64

    def item_audience(self, acts, lse, tr, row_lo, q_col, k, score_out, id_out, ws=None, n_rows=None):
        LOG.append(("item_audience", lse is not None, k))
        assert n_rows == tr.hi - tr.lo and row_lo == tr.lo and tuple(score_out.shape) == (q_col.numel(), k)
        id_out.copy_((row_lo + torch.arange(k, dtype=torch.int32)).expand(q_col.numel(), k))
        score_out.copy_(-id_out.float())

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
    out = {"plain": lambda: dict(k=7),
           "rule": lambda: dict(k=7, rule=MinSlots(LABELS, 3, [2, 0, 4])),
           "rule0": lambda: dict(k=7, rule=MinSlots(LABELS, 3, [0, 0, 0])),
           "diversify": lambda: dict(k=4, diversify=Diversify(0.5, candidates=7))}
    out.update(more_modes())
    return out


def more_modes():
    """k = 7 throughout: calibrated over the three classes; capped and floored out of 9 candidates, ranking by log-probability and by the
    logit; group 1 promoted to 0.3 of the 56 slots (17); the audiences (2 users) of one item of each slab beside the plain lists, and alone"""
    from ltgan.serving import Audience, Calibrate, ExposureCap, ExposureFloor, ShareTarget
    return {"calibrate": lambda: dict(k=7, calibrate=Calibrate(LABELS, 3, 0.5)),
            "cap_logprob": lambda: dict(k=7, cap=ExposureCap(3, candidates=9, score="logprob")),
            "cap_logit": lambda: dict(k=7, cap=ExposureCap(3, candidates=9, score="logit")),
            "floor_logprob": lambda: dict(k=7, floor=ExposureFloor(2, 2, candidates=9, score="logprob")),
            "floor_logit": lambda: dict(k=7, floor=ExposureFloor(2, 2, candidates=9, score="logit")),
            "share": lambda: dict(k=7, share=ShareTarget(LABELS, 3, [1], 0.3)),
            "audience_logprob": lambda: dict(k=7, audience=Audience([3, 140], k=2, score="logprob")),
            "audience_logit": lambda: dict(k=7, audience=Audience([3, 140], k=2, score="logit")),
            "audience_only": lambda: dict(k=0, audience=Audience([3, 140], k=2, score="logprob"))}


def report():
    from ltgan.trainer import LongTailReport
    return LongTailReport(LABELS, 3, k_ndcg=4, k_r1=2, k_r2=3, k_exp=4)


def explain():
    from ltgan.serving import Explain
    return Explain(r=2, top=3)


def readers(name):
    """the (report, explain) a mode is walked with: neither, either, both; k = 0 serves no lists, so nothing reads them"""
    if name == "audience_only":
        return [(None, None)]
    return [(None, None), (report(), None), (None, explain()), (report(), explain())]


LIST_MASK = {"calibrate": 1 << 0, "share": 0x1FF & ~(1 << 1)}      # the stubs keep the head of the first class list / of the rest list


def check_tables(name, rec, full):
    """what run() left behind: the table (the stubs of quota / diversify / cap / floor keep the head of the plain list / of the
    candidates, those of calibrate / share the head of one masked list), the merged lists of the short last chunk where the rule and the
    re-ranking read them, the whole-split rules' gathered tables, and the explanations of the FINAL lists"""
    want = reference(full, rec.k, LIST_MASK.get(name))
    assert equal_lists(rec.scores, rec.ids, want), name
    last = full[ROWS:]
    for whole in (rec.cap, rec.floor):
        if whole is not None:
            assert equal_lists(whole.cand_s, whole.cand_i, reference(full, 9)), name
            if name.endswith("logprob"):                     # the full-row lse of every chunk, whichever way it was combined
                assert whole.needs_lse and torch.equal(whole.lse, torch.arange(N_USERS).float()), name
            else:
                assert not whole.needs_lse and whole.lse is None, name
    if name == "share":
        assert equal_lists(rec.share.pro_s, rec.share.pro_i, reference(full, 7, 1 << 1)), name
        assert equal_lists(rec.share.rest_s, rec.share.rest_i, reference(full, 7, 0x1FF & ~(1 << 1))), name
    if name == "calibrate":
        g_s, g_i = rec.calibrate.class_lists(N_USERS - ROWS, 7)
        for j in range(3):
            assert equal_lists(g_s[j], g_i[j], reference(last, 7, 1 << j)), (name, j)
    if rec.explain is not None:
        assert torch.equal(rec.explain.why_i, rec.ids[:, :3, None] * 10 + torch.arange(2, dtype=torch.int32)), name
        assert torch.equal(rec.explain.why_s, (-torch.arange(2).float()).expand(N_USERS, 3, 2)), name
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

# ---- the flows added since, written out from Recommender.__init__ / .run, Calibrate.apply, ExposureCap / ExposureFloor / ShareTarget
# .gather / .match, Audience.add, Explain.pack / .apply and ShardedRecommender._forward as they stood when every rule had its own branch
# of the walk.  BIND: what the constructor asks the engine.  AFTER: what follows the last chunk (the same on every rank: nothing is
# exchanged); its presence makes the rule one over the whole split, whose report and explanations come in a second pass without a forward.
BIND = {"cap_logprob": [("cap_ws_bytes", 8, 9, 150)], "cap_logit": [("cap_ws_bytes", 8, 9, 150)],
        "floor_logprob": [("floor_ws_bytes", 8, 9, 150)], "floor_logit": [("floor_ws_bytes", 8, 9, 150)],
        "share": [("share_ws_bytes", 8, 7)]}
AFTER = {
    "cap_logprob": [("cap_index", 9, 150), ("cap_rounds", True, 7, 4), ("cap_finish", 7)],
    "cap_logit": [("cap_index", 9, 150), ("cap_rounds", False, 7, 4), ("cap_finish", 7)],
    "floor_logprob": [("floor_index", 9, 150), ("floor_rounds", True, 7, 2, 4), ("floor_finish", True, 7, 2)],
    "floor_logit": [("floor_index", 9, 150), ("floor_rounds", False, 7, 2, 4), ("floor_finish", False, 7, 2)],
    "share": [("topk_share", 7, 17)],
}
UNSHARDED.update({
    "calibrate": lambda lo: [("forward", STEP + lo), ("topk_groups", 7, 1), ("topk_groups", 7, 2), ("topk_groups", 7, 4), ("hist_groups", 3),
                             ("topk_calibrate", (0, 1, 2), 7)],
    "cap_logprob": lambda lo: [("forward", STEP + lo), ("topk", 9)],
    "cap_logit": lambda lo: [("forward", STEP + lo), ("topk", 9)],
    "floor_logprob": lambda lo: [("forward", STEP + lo), ("topk", 9)],
    "floor_logit": lambda lo: [("forward", STEP + lo), ("topk", 9)],
    "share": lambda lo: [("forward", STEP + lo), ("topk_groups", 7, 2), ("topk_groups", 7, 0x1FD)],
    "audience_logprob": lambda lo: [("forward", STEP + lo), ("item_audience", True, 2), ("topk_merge", 2, 2, 2), ("topk", 7)],
    "audience_logit": lambda lo: [("forward", STEP + lo), ("item_audience", False, 2), ("topk_merge", 2, 2, 2), ("topk", 7)],
    "audience_only": lambda lo: [("forward", STEP + lo), ("item_audience", True, 2), ("topk_merge", 2, 2, 2)],
})
UNSHARDED_EXPLAIN_ONCE = [("item_pack",)]                   # (not beside a Diversify of the same space and metric: its image is shared)
UNSHARDED_EXPLAIN = [("topk_explain", 3, 2)]

# the full-row lse: one more all-gather of the row partials and their combination, per chunk of n rows, exactly where something ranks by logprob
SHARDED_LSE = lambda lo, R: [("all_gather", "float32"), ("rowstats_combine", R, min(ROWS, N_USERS - lo))]      # noqa: E731
SHARDED.update({
    "calibrate": lambda lo, R: SHARDED_FORWARD(lo) + [("topk_groups", 7, 1), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7),
                                                      ("topk_groups", 7, 2), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7),
                                                      ("topk_groups", 7, 4), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7),
                                                      ("hist_groups", 3), ("all_reduce", "int32"), ("topk_calibrate", (0, 1, 2), 7)],
    "cap_logprob": lambda lo, R: SHARDED_FORWARD(lo) + SHARDED_LSE(lo, R) + [("topk", 9), ("all_gather", "float32"), ("all_gather", "int32"),
                                                                             ("topk_merge", R, 9, 9)],
    "cap_logit": lambda lo, R: SHARDED_FORWARD(lo) + [("topk", 9), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 9, 9)],
    "floor_logprob": lambda lo, R: SHARDED_FORWARD(lo) + SHARDED_LSE(lo, R) + [("topk", 9), ("all_gather", "float32"), ("all_gather", "int32"),
                                                                               ("topk_merge", R, 9, 9)],
    "floor_logit": lambda lo, R: SHARDED_FORWARD(lo) + [("topk", 9), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 9, 9)],
    "share": lambda lo, R: SHARDED_FORWARD(lo) + [("topk_groups", 7, 2), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7),
                                                  ("topk_groups", 7, 0x1FD), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7)],
    "audience_logprob": lambda lo, R: SHARDED_FORWARD(lo) + SHARDED_LSE(lo, R) + [("item_audience", True, 2), ("topk_merge", 2, 2, 2),
                                                                                  ("topk", 7), ("all_gather", "float32"), ("all_gather", "int32"),
                                                                                  ("topk_merge", R, 7, 7)],
    "audience_logit": lambda lo, R: SHARDED_FORWARD(lo) + [("item_audience", False, 2), ("topk_merge", 2, 2, 2),
                                                           ("topk", 7), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 7, 7)],
    "audience_only": lambda lo, R: SHARDED_FORWARD(lo) + SHARDED_LSE(lo, R) + [("item_audience", True, 2), ("topk_merge", 2, 2, 2)],
})
SHARDED_EXPLAIN_ONCE = [("item_pack",), ("all_reduce", "int32")]
SHARDED_EXPLAIN = lambda R: [("topk_explain", 3, 2), ("all_gather", "float32"), ("all_gather", "int32"), ("topk_merge", R, 2, 2)]      # noqa: E731
LONGEST = {"cap_logprob": 9, "cap_logit": 9, "floor_logprob": 9, "floor_logit": 9,
           "audience_only": 0}      # the SlabLists' buffers: 7 entries a row otherwise


def whole_run(name, rep, why, once, why_once, chunk, why_chunk):
    """the sequence of one run(): what happens once, then per chunk the forward and the lists, each followed by its readers (the report's
    launch, the explanation's) -- unless the lists exist only after the last chunk (AFTER), when the readers follow in a second pass"""
    tail = ([("topk_metrics",)] if rep is not None else []) + (why_chunk if why is not None else [])
    seq = list(once) + (why_once if why is not None and name != "diversify" else [])
    for lo in (0, ROWS):
        seq += chunk(lo) + ([] if name in AFTER else tail)
    return seq + (AFTER[name] + tail + tail if name in AFTER else [])


RULES = {"rule": lambda: modes()["rule"]()["rule"], "diversify": lambda: modes()["diversify"]()["diversify"],
         "calibrate": lambda: modes()["calibrate"]()["calibrate"], "cap": lambda: modes()["cap_logit"]()["cap"],
         "share": lambda: modes()["share"]()["share"], "floor": lambda: modes()["floor_logit"]()["floor"]}


def refusals(Recommender, **kw):
    """no two of the six rules together (15 pairs); k = 0 serves no lists: only an audience walks without them"""
    def refused(**more):
        try:
            Recommender(FakeEngine(), FakeEval(), chunk=ROWS, **kw, **more)
        except ValueError:
            return True
        return False
    names = list(RULES)
    pairs = [(a, b) for i, a in enumerate(names) for b in names[i + 1:]]
    assert len(names) == 6 and len(pairs) == 15
    for a, b in pairs:
        assert refused(k=7, **{a: RULES[a](), b: RULES[b]()}), (a, b)
    for a in names:
        assert refused(k=0, **{a: RULES[a]()}), a
        assert refused(k=0, audience=modes()["audience_only"]()["audience"], **{a: RULES[a]()}), a
    assert refused(k=0, report=report()) and refused(k=0, explain=explain())
    assert not refused(k=0, audience=modes()["audience_only"]()["audience"])


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
        for rep, why in readers(name):
            eng = FakeEngine()
            taken()
            rec = Recommender(eng, FakeEval(), chunk=ROWS, report=rep, explain=why, **kw())
            assert rec.lists.part_s is None and rec.lists.loc_s is None and rec.chunk == ROWS
            assert taken() == BIND.get(name, []), name
            ids, scores = rec.run(rng_step=STEP)
            assert taken() == whole_run(name, rep, why, UNSHARDED_ONCE.get(name, []), UNSHARDED_EXPLAIN_ONCE, UNSHARDED[name],
                                        UNSHARDED_EXPLAIN), (name, rep is not None, why is not None)
            assert ids.shape == scores.shape == (N_USERS, rec.k)
            check_tables(name, rec, full)
            if name == "plain":                                          # straight into the table, chunk by chunk
                assert eng.dst == [(rec.scores[lo:].data_ptr(), rec.ids[lo:].data_ptr()) for lo in (0, ROWS)]
            if name == "rule":                                           # ... and into the rule's own arrays
                g_s, g_i = rec.rule.reserved(N_USERS - ROWS)
                assert eng.dst[-3:] == [(t.data_ptr(), u.data_ptr()) for t, u in (rec.rule.plain(N_USERS - ROWS, 7), (g_s[0], g_i[0]), (g_s[1], g_i[1]))]
    refusals(Recommender)


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
        for rep, why in readers(name):
            eng = FakeEngine(lo_i, hi_i, rank, R)
            taken()
            rec = ShardedRecommender(eng, FakeEval(), chunk=ROWS, report=rep, explain=why, **kw())
            assert rec.chunk == ROWS and rec.lists.parts == R and rec.lists.part_s.numel() == R * ROWS * LONGEST.get(name, 7)
            assert not hasattr(rec.rule, "part_s") and not hasattr(rec.diversify, "part_s")
            assert (rec.rowpart_all is not None) == name.endswith(("logprob", "audience_only")), name
            assert taken() == BIND.get(name, []), name
            rec.run(rng_step=STEP)
            assert taken() == whole_run(name, rep, why, SHARDED_ONCE.get(name, []), SHARDED_EXPLAIN_ONCE, lambda lo: SHARDED[name](lo, R),
                                        SHARDED_EXPLAIN(R)), (rank, name, rep is not None, why is not None)
            check_tables(name, rec, full)
    refusals(ShardedRecommender)
    unsharded()                                                          # (with the collectives recorded: there are none)
    dist.barrier()
    if rank == 0:
        print("SERVING_CPU_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
