"""Everything that serves a trained model: validation / test scoring, top-K lists (plain, with minimum slots per item group, diversified,
calibrated to each user's history, capped in how many lists an item may appear, with a set share of all slots for some item groups,
with a floor under how many lists an item appears in, gated by the discriminator, sampled for exploration with logged propensities), the long-tail report read off them, the explanation
of every list entry (the user's history items nearest to it), the discriminator's critic of every niche entry, similar-item lists,
item audiences (the k likeliest users of an item, gathered over the same chunk walk), the replay of a logged exploration run under other
policies (off-policy estimates, from the same walk), and the set-up the CLIs (test.py, recommend.py, longtail.py, similar.py, audience.py,
replay.py) share.

One chunk walk (Recommender.run) serves every kind of list, unsharded and over item shards: the forward sits behind one method that
ShardedRecommender overrides, and every catalogue-wide list comes from one SlabLists, which alone knows whether the catalogue is cut
into slabs.  The walk knows no kind of list: it asks the one rule it was given (a Rule) the few questions of the protocol, so a new kind
of list is one class.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.distributed as dist

from ._cabi import LTG_CAP_MAX_ROUNDS, LTG_CAP_STATE, LTG_FLOOR_MAX_ROUNDS, LTG_FLOOR_STATE, LTG_METRIC, LTG_PAIR_MAX_K, LTG_SHARE_STATE, LTG_SPACE, LtgError

EVAL_LOGITS_BYTES = 2 << 30


def eval_chunk_rows(n_items_local, budget=EVAL_LOGITS_BYTES):
    """users per scoring chunk so that the [chunk, I] fp32 logits stay within `budget` bytes (test.py:76 scores 20 000
    users at a time: 16 GB at I = 200 000)."""
    return max(1, int(budget // (4 * max(1, n_items_local))))


def chunk_rows(engine, ev, chunk):
    """the users per chunk every scorer walks `ev` in: `chunk`, capped by the users there are and by eval_chunk_rows of the slab"""
    return int(min(chunk, max(1, ev.n), eval_chunk_rows(engine.I)))


def metric_means(out):
    """the metric table [n_users, 4] = {ndcg, recall20, recall50, valid} -> its float64 means over the valid users"""
    o = out.cpu().numpy().astype(np.float64)
    ok = o[:, 3] > 0
    n = int(ok.sum())
    return dict(ndcg=float(o[ok, 0].mean()) if n else float("nan"), recall20=float(o[ok, 1].mean()) if n else float("nan"),
                recall50=float(o[ok, 2].mean()) if n else float("nan"), n_users=n)


def sharded_forward(engine, tr, n, acts, rowpart, keep_prob, rng_step, group=None):
    """the scoring forward of the n rows `tr` over item shards: this slab's part of the encoder pre-activation, ONE all-reduce of it,
    then the replicated middle layers and this slab's logits (dropout on, eps off: Evaluator's forward)"""
    fo = engine.fwd_opts(keep_prob, 0.0, rng_step)
    engine.g_fwd_enc(tr, acts, fo)
    dist.all_reduce(acts.h1[:n], op=dist.ReduceOp.SUM, group=group)
    engine.g_fwd_rest(tr, None, acts, fo, rowpart)


class Evaluator:
    """Validation / test scoring (train.py:333-348, test.py:138-173): forward with dropout ON (Q3),
    fold-in items masked to -inf, NDCG@100 / Recall@20 / Recall@50, in chunks of `chunk` users
    (test.py:76 uses 20000), capped so that a chunk's logits stay within EVAL_LOGITS_BYTES."""

    def __init__(self, engine, ev, chunk=20000):
        self.eng, self.ev, self.chunk = engine, ev, chunk_rows(engine, ev, chunk)
        self.acts = engine.new_acts(self.chunk)
        self.out = torch.zeros(ev.n, 4, dtype=torch.float32, device=engine.device)

    def run(self, rng_step=0, keep_prob=0.75):
        eng, ev = self.eng, self.ev
        for lo in range(0, ev.n, self.chunk):
            hi = min(ev.n, lo + self.chunk)
            tr, te = ev.rows(lo, hi)
            eng.forward(tr, self.acts, keep_prob=keep_prob, is_training=0.0, rng_step=rng_step + lo)
            eng.rank_metrics(self.acts, tr, te, self.out[lo:])
        return metric_means(self.out)


class ShardedEvaluator:
    """Validation / test scoring over item shards (train.py:333-348, test.py:138-173).  Per chunk of users: the
    sharded forward (one all-reduce of the encoder pre-activation), then two small exchanges for the ranking:
      1. all-reduce(sum) of the held-out entries' scores   (float32 per held-out entry; the owner contributes)
      2. all-reduce(sum) of the per-entry rank counts      (int32 per held-out entry)
    The softmax is never materialised: ranking by logits equals ranking by probabilities row by row.  Every rank
    ends with the identical metric table."""

    def __init__(self, engine, ev, group=None, chunk=20000):
        self.eng, self.ev, self.group = engine, ev, group
        self.chunk = chunk_rows(engine, ev, chunk)
        self.acts = engine.new_acts(self.chunk)
        dev = engine.device
        n_te = max(1, int(ev.te_indices.numel()))
        self.score = torch.zeros(n_te, dtype=torch.float32, device=dev)
        self.count = torch.zeros(n_te, dtype=torch.int32, device=dev)
        self.out = torch.zeros(ev.n, 4, dtype=torch.float32, device=dev)
        self.rowpart = torch.zeros(self.chunk * 5, dtype=torch.float32, device=dev)

    def run(self, rng_step=0, keep_prob=0.75):
        eng, ev = self.eng, self.ev
        te_ptr = ev.te_host.indptr
        for lo in range(0, ev.n, self.chunk):
            hi = min(ev.n, lo + self.chunk)
            tr, te = ev.rows(lo, hi)
            sharded_forward(eng, tr, hi - lo, self.acts, self.rowpart, keep_prob, rng_step + lo, self.group)
            e0, e1 = int(te_ptr[lo]), int(te_ptr[hi])
            eng.rank_scores(self.acts, tr, te, self.score)
            if e1 > e0:
                dist.all_reduce(self.score[e0:e1], op=dist.ReduceOp.SUM, group=self.group)
            eng.rank_counts(self.acts, tr, te, self.score, self.count)
            if e1 > e0:
                dist.all_reduce(self.count[e0:e1], op=dist.ReduceOp.SUM, group=self.group)
            eng.rank_finish(te, self.count, self.out[lo:])
        return metric_means(self.out)


class SlabLists:
    """The one source of catalogue-wide lists: the L best items of the logits in `acts` over the WHOLE catalogue, optionally only the
    items a group mask admits.  parts == 1 (the engine holds every item): ltg_topk / ltg_topk_groups straight into the caller's outputs.
    parts > 1 (item shards, one rank per slab): the slab's list (global ids), ONE all-gather of the scores and one of the ids (list
    all-gathers work over gloo as well as nccl), then ltg_topk_merge into the outputs -- every rank ends with the identical lists and no
    logit is ever exchanged.  One flat pair of local / gathered buffers serves lists of every length up to `longest` for chunks of up to
    `rows` rows: each call views them as [n, L] / [parts, n, L], so a short last chunk is contiguous like a full one.  Reusing them for
    the next list of a chunk is safe: the gathers are synchronous collectives on the stream the engine launches on (torch's current
    stream), so the merge that reads the gathered buffers is enqueued before the next local list overwrites them."""

    def __init__(self, engine, rows, longest, group=None, parts=1):
        self.eng, self.group, self.parts = engine, group, int(parts)
        self.loc_s = self.loc_i = self.part_s = self.part_i = None
        if self.parts > 1:
            n, dev = int(rows) * int(longest), engine.device
            self.loc_s = torch.empty(n, dtype=torch.float32, device=dev)
            self.loc_i = torch.empty(n, dtype=torch.int32, device=dev)
            self.part_s = torch.empty(self.parts * n, dtype=torch.float32, device=dev)
            self.part_i = torch.empty(self.parts * n, dtype=torch.int32, device=dev)

    def local(self, n, L, score_out, id_out):
        """where this rank's own [n, L] lists go: the outputs themselves when there is nothing to gather"""
        if self.parts == 1:
            return score_out, id_out
        return self.loc_s[: n * L].view(n, L), self.loc_i[: n * L].view(n, L)

    def merge(self, loc_s, loc_i, score_out, id_out):
        """this rank's lists (where local() put them) -> the catalogue-wide ones in score_out / id_out [n, k]"""
        if self.parts == 1:
            return
        R, (n, L) = self.parts, loc_s.shape
        ps, pi = self.part_s[: R * n * L].view(R, n, L), self.part_i[: R * n * L].view(R, n, L)
        dist.all_gather(list(ps.unbind(0)), loc_s, group=self.group)
        dist.all_gather(list(pi.unbind(0)), loc_i, group=self.group)
        self.eng.topk_merge(ps, pi, int(score_out.shape[1]), score_out, id_out)

    def topk(self, acts, tr, n, L, score_out, id_out, labels=None, mask=None):
        """score_out / id_out [n, L] <- the L best items of the n rows of logits in `acts`, fold-in items of `tr` excluded; mask given:
        only items whose label (labels: uint8 per GLOBAL item id) the group mask admits"""
        ls, li = self.local(n, L, score_out, id_out)
        if mask is None:
            self.eng.topk(acts, tr, L, ls, li)
        else:
            self.eng.topk_groups(acts, tr, L, labels, mask, ls, li)
        self.merge(ls, li, score_out, id_out)


def group_labels(labels, n_groups, engine=None):
    """the item-group labels everything grouped takes: one uint8 per GLOBAL item id, a label >= n_groups is in no group, 1 <= n_groups
    <= 8 -> the contiguous uint8 host array.  engine given (bind time): there must be one label per item of its catalogue -> the labels
    on its device"""
    if not 1 <= int(n_groups) <= 8:
        raise ValueError("n_groups must be in [1, 8]")
    labels = np.ascontiguousarray(np.asarray(labels), dtype=np.uint8)
    if engine is None:
        return labels
    if labels.size != engine.I_global:
        raise ValueError("labels hold %d items, the catalogue %d" % (labels.size, engine.I_global))
    return torch.from_numpy(labels).to(engine.device)


class LongTailReport:
    """The long-tail report a Recommender / ShardedRecommender fills when it is passed as `report=`: per user and item group
    NDCG@k_ndcg / Recall@k_r1 / Recall@k_r2 (plus the all-items slot, which is Evaluator's table) and the exposure counts at k_exp,
    read off the chunk's top-K lists by ltg_topk_metrics -- one forward per chunk serves the lists and the report.
    labels: one uint8 per GLOBAL item id, a label >= n_groups is in no group.  After run(): `out` [n_users, n_groups + 1, 4] and
    `item_hits` [n_items] on the device; table() brings both to the host."""

    def __init__(self, labels, n_groups, k_ndcg=100, k_r1=20, k_r2=50, k_exp=100):
        self.labels_host, self.n_groups = group_labels(labels, n_groups), int(n_groups)
        self.cut = dict(k_ndcg=int(k_ndcg), k_r1=int(k_r1), k_r2=int(k_r2), k_exp=int(k_exp))
        if min(self.cut.values()) < 1 or max(self.cut.values()) > 1024:
            raise ValueError("every cutoff must be in [1, 1024]")
        self.k = max(self.cut.values())                  # the list length the report needs
        self.out = self.item_hits = self.labels = None

    def bind(self, engine, n_users, k):
        if k < self.k:
            raise ValueError("top-K lists of %d entries are shorter than the report's largest cutoff %d" % (k, self.k))
        dev = engine.device
        self.labels = group_labels(self.labels_host, self.n_groups, engine)
        self.out = torch.zeros(n_users, self.n_groups + 1, 4, dtype=torch.float32, device=dev)
        self.item_hits = torch.zeros(self.labels_host.size, dtype=torch.int32, device=dev)

    def add(self, engine, ids, te, lo):
        engine.topk_metrics(ids, te, self.labels, self.n_groups, self.out[lo:], self.item_hits, **self.cut)

    def table(self):
        """-> (out [n_users, n_groups + 1, 4] float32, item_hits [n_items] int32) host arrays"""
        return self.out.cpu().numpy(), self.item_hits.cpu().numpy()


class Rule:
    """What the chunk walk (Recommender.run) asks of the one serve-time rule it is given -- the whole protocol:
      bind(engine, rows, k, n_users)   once: the buffers for chunks of up to `rows` users, lists of k entries and a split of n_users;
                                       sets `longest`, the longest list the rule will ask the SlabLists for
      begin(engine, group)             at the start of every run()
      whole = False:  apply(lists, acts, tr, n, k, lo, score_out, id_out)   per chunk: the lists of users lo .. lo + n, whose logits
                                       `acts` holds, from the SlabLists `lists` into score_out / id_out [n, k]
      whole = True:   gather(lists, acts, tr, n, lo)   per chunk: only what the rule needs of the chunk, since its rows depend on each
                      match(engine, k, score_out, id_out)   other; after the last chunk the lists of the whole split [n_users, k]
      needs_lse                        the rule reads acts.lse: over item shards the walk then combines the full-row lse per chunk"""

    whole = False
    needs_lse = False
    longest = 0

    def begin(self, engine, group=None):
        pass


class MinSlots(Rule):
    """A serve-time rule, passed as `rule=` to a Recommender / ShardedRecommender: at least slots[g] of every user's k list entries come
    from item group g (labels: one uint8 per GLOBAL item id, a label >= n_groups is in no group; the labels a LongTailReport takes).  Walking
    a user's ranking from the top, an item is taken if its group still owes slots, or if a slot is left that no group's outstanding minimum
    claims; a group with fewer eligible items than its minimum hands the rest to the free slots.  slots all 0 is the plain list; slots[g] = k
    is the k best items of group g.  Per chunk: the plain list, one reserved list per group with slots[g] > 0 (ltg_topk_groups with that
    group's bit, every one max(slots) entries long so that they share one array), composed by ltg_topk_quota.  Over item shards every one
    of those lists is gathered and merged by the SlabLists, and every rank composes the same ruled lists.  The report and the
    explanations read the ruled lists."""

    def __init__(self, labels, n_groups, slots):
        self.labels_host, self.n_groups = group_labels(labels, n_groups), int(n_groups)
        self.slots = [int(x) for x in slots]
        if len(self.slots) != self.n_groups:
            raise ValueError("slots holds %d counts for %d groups" % (len(self.slots), self.n_groups))
        if min(self.slots) < 0:
            raise ValueError("a group's minimum must be >= 0")
        self.groups = [g for g, m in enumerate(self.slots) if m > 0]        # the groups with a reserved list
        self.quota = [self.slots[g] for g in self.groups]
        self.m = self.longest = max(self.slots)
        self.labels = None

    def bind(self, engine, rows, k, n_users):
        if sum(self.slots) > k:
            raise ValueError("the minimum slots sum to %d, more than the %d entries of a list" % (sum(self.slots), k))
        dev = engine.device
        self.labels = group_labels(self.labels_host, self.n_groups, engine)
        n_l, m = max(1, len(self.groups)), max(1, self.m)
        self.all_s = torch.empty(rows * k, dtype=torch.float32, device=dev)
        self.all_i = torch.empty(rows * k, dtype=torch.int32, device=dev)
        self.grp_s = torch.empty(n_l * rows * m, dtype=torch.float32, device=dev)
        self.grp_i = torch.empty(n_l * rows * m, dtype=torch.int32, device=dev)

    def plain(self, n, k):
        """where the chunk's plain lists go: ([n, k] scores, [n, k] ids)"""
        return self.all_s[: n * k].view(n, k), self.all_i[: n * k].view(n, k)

    def reserved(self, n):
        """where the chunk's reserved lists go: ([groups, n, m] scores, ids), list j for group self.groups[j]"""
        n_l = len(self.groups)
        return self.grp_s[: n_l * n * self.m].view(n_l, n, self.m), self.grp_i[: n_l * n * self.m].view(n_l, n, self.m)

    def apply(self, lists, acts, tr, n, k, lo, score_out, id_out):
        a_s, a_i = self.plain(n, k)
        lists.topk(acts, tr, n, k, a_s, a_i)
        if not self.groups:                              # nothing reserved: the plain list
            score_out.copy_(a_s)
            id_out.copy_(a_i)
            return
        g_s, g_i = self.reserved(n)
        for j, g in enumerate(self.groups):
            lists.topk(acts, tr, n, self.m, g_s[j], g_i[j], self.labels, 1 << g)
        lists.eng.topk_quota(a_s, a_i, g_s, g_i, self.quota, score_out, id_out)


def catalogue_image(engine, space, metric, image=None, group=None):
    """-> the bf16 operand image [I_global, 608] int16 of the WHOLE catalogue (ltg_item_pack), written into `image` when one is given.
    Over item shards every rank packs its slab into a zeroed buffer at its item_lo, and the buffer is all-reduced viewed as int32 --
    exactly one rank contributes each row."""
    if group is None and engine.I == engine.I_global:
        return engine.item_pack(space, metric, out=image)
    if image is None:
        image = torch.empty(engine.I_global, 608, dtype=torch.int16, device=engine.device)
    image.zero_()
    engine.item_pack(space, metric, out=image[engine.item_lo:engine.item_hi])
    dist.all_reduce(image.view(torch.int32), op=dist.ReduceOp.SUM, group=group)
    return image


class Diversify(Rule):
    """A serve-time re-ranking, passed as `diversify=` to a Recommender / ShardedRecommender: greedy maximal marginal relevance.  Each
    user's `candidates` best items (ltg_topk; default min(256, 2 k), k <= candidates <= 256) are re-ranked so that the next entry is the
    one with the largest  lam * relevance - (1 - lam) * (largest similarity to what the list already holds)  -- relevance = the score
    scaled to [0, 1] over the candidates, similarity = the product of the items' rows in the bf16 image of the `decoder` (W_p1t) or
    `encoder` (W_q0) table, `cosine` or `dot` (ltg_item_pack).  lam = 1 is the plain list.  The image is packed once per run(); per chunk
    ltg_topk at `candidates`, then ONE launch of ltg_topk_diversify: the candidates' similarity matrix never leaves the chip.  The lists
    keep every pick's original score, so they are generally not descending.  After run(): stats() [n_users, 2] = the mean pair similarity
    of the plain top-k list and of the diversified one.  Over item shards the candidates are gathered and merged at their own length by
    the SlabLists and every rank re-ranks the same candidates against the image of the whole catalogue.  The report and the
    explanations read the diversified lists."""

    def __init__(self, lam, candidates=None, space="decoder", metric="cosine"):
        self.lam = float(lam)
        if not 0.0 <= self.lam <= 1.0:               # (NaN fails both comparisons)
            raise ValueError("lam must be in [0, 1], got %r" % (lam,))
        if space not in LTG_SPACE or metric not in LTG_METRIC:
            raise ValueError("space must be decoder or encoder, metric cosine or dot")
        self.candidates = None if candidates is None else int(candidates)
        self.space, self.metric = space, metric
        self.c = self.image = self.stat = None
        self.image_lo = 0

    def bind(self, engine, rows, k, n_users):
        c = min(256, 2 * k) if self.candidates is None else self.candidates
        if not k <= c <= 256:
            raise ValueError("candidates must be in [k, 256] = [%d, 256], got %d" % (k, c))
        self.c = self.longest = c
        dev = engine.device
        self.cand_s = torch.empty(rows * c, dtype=torch.float32, device=dev)
        self.cand_i = torch.empty(rows * c, dtype=torch.int32, device=dev)
        self.stat = torch.zeros(n_users, 2, dtype=torch.float32, device=dev)

    def begin(self, engine, group=None):
        """the image of the whole catalogue, once per run().  group given (item shards): every rank packs its slab into a zeroed
        [I_global, 608] buffer at its item_lo, and the buffer is all-reduced viewed as int32 -- exactly one rank contributes each row."""
        self.image = catalogue_image(engine, self.space, self.metric, self.image, group)

    def candidates_of(self, n):
        """where the chunk's candidate lists go: ([n, candidates] scores, ids)"""
        return self.cand_s[: n * self.c].view(n, self.c), self.cand_i[: n * self.c].view(n, self.c)

    def apply(self, lists, acts, tr, n, k, lo, score_out, id_out):
        c_s, c_i = self.candidates_of(n)
        lists.topk(acts, tr, n, self.c, c_s, c_i)
        lists.eng.topk_diversify(self.image, self.image_lo, c_s, c_i, self.lam, k, score_out, id_out, self.stat[lo:lo + n])

    def stats(self):
        """-> [n_users, 2] float32 host array: mean pair similarity of the first k candidates, and of the list"""
        return self.stat.cpu().numpy()


class Calibrate(Rule):
    """A serve-time re-ranking, passed as `calibrate=` to a Recommender / ShardedRecommender: calibrated recommendation (Steck, RecSys
    2018) with the total-variation distance in place of the KL divergence.  Every user's list follows the class mix of that user's
    fold-in history (labels: one uint8 per GLOBAL item id, the class of an item = min(label, n_groups), the last class is "in no group";
    the labels a LongTailReport takes): greedily, the next entry is the best remaining item of some class with the largest
    (1 - lam) * relevance - lam * (miscalibration of the list so far plus that item) -- relevance = the score scaled to [0, 1] over the
    plain top-k list, miscalibration = half the sum over the classes of |history share - list share|.  lam = 0 is the plain list; a user
    without a history keeps the plain list at every lam.  Per chunk: one ltg_topk_groups list of k entries per class that occurs in the
    catalogue (so the greedy runs over the whole catalogue, not over a truncated candidate set), ltg_hist_groups on the chunk's histories,
    then ONE launch of ltg_topk_calibrate.  The lists keep every pick's original score, so they are generally not descending.  After
    run(): stats() [n_users, 2] = the miscalibration of the plain top-k list and of the calibrated one.  Over item shards every class
    list is gathered and merged by the SlabLists, every rank counts its slab's part of the histories and the counts are all-reduced: no
    logit is exchanged and every rank composes the same lists.  The report and the explanations read the calibrated lists."""

    def __init__(self, labels, n_groups, lam):
        self.labels_host, self.n_groups = group_labels(labels, n_groups), int(n_groups)
        self.lam = float(lam)
        if not 0.0 <= self.lam <= 1.0:               # (NaN fails both comparisons)
            raise ValueError("lam must be in [0, 1], got %r" % (lam,))
        self.classes = self.masks = self.labels = self.stat = None

    def bind(self, engine, rows, k, n_users):
        self.labels = group_labels(self.labels_host, self.n_groups, engine)
        g, dev, self.longest = self.n_groups, engine.device, k
        self.classes = [int(c) for c in np.unique(np.minimum(self.labels_host, g))]      # a class with no item needs no list
        self.masks = [1 << c if c < g else (0x1FF >> g) << g for c in self.classes]       # the last class: bits n_groups .. 8
        n_l = len(self.classes)
        self.grp_s = torch.empty(n_l * rows * k, dtype=torch.float32, device=dev)
        self.grp_i = torch.empty(n_l * rows * k, dtype=torch.int32, device=dev)
        self.hist = torch.empty(rows * (g + 1), dtype=torch.int32, device=dev)
        self.stat = torch.zeros(n_users, 2, dtype=torch.float32, device=dev)

    def class_lists(self, n, k):
        """where the chunk's class lists go: ([classes, n, k] scores, ids), list j for class self.classes[j]"""
        n_l = len(self.classes)
        return self.grp_s[: n_l * n * k].view(n_l, n, k), self.grp_i[: n_l * n * k].view(n_l, n, k)

    def apply(self, lists, acts, tr, n, k, lo, score_out, id_out):
        eng = lists.eng
        g_s, g_i = self.class_lists(n, k)
        for j, mask in enumerate(self.masks):
            lists.topk(acts, tr, n, k, g_s[j], g_i[j], self.labels, mask)
        hist = self.hist[: n * (self.n_groups + 1)].view(n, self.n_groups + 1)
        eng.hist_groups(tr, self.labels, self.n_groups, hist, hist_lo=eng.item_lo if lists.parts > 1 else 0)
        if lists.parts > 1:                              # every rank counted its slab's part of the histories
            dist.all_reduce(hist, op=dist.ReduceOp.SUM, group=lists.group)
        eng.topk_calibrate(g_s, g_i, self.classes, self.n_groups, hist, self.lam, k, score_out, id_out, self.stat[lo:lo + n])

    def stats(self):
        """-> [n_users, 2] float32 host array: the miscalibration of the plain top-k list, and of the calibrated list"""
        return self.stat.cpu().numpy()


class _Matching(Rule):
    """What ExposureCap and ExposureFloor share: a rule over the WHOLE split that is a stable matching between users and items.  The per-item
    value (NOUN: the word for it in messages) is an int (every item), an int array per GLOBAL item id, or (labels, n_groups, {group index:
    value}) -- only the items of those groups, every other item gets FILL (labels: one uint8 per GLOBAL id, the labels a LongTailReport
    takes).  A user's side of the matching is their `candidates` best items (default min(1024, 4 k), k <= candidates <= 1024) in list
    order; an item ranks users by `score` -- `logprob`: logit - lse, the log-probability the user's softmax gives the item, comparable
    across users and the Audience score; `logit`: the raw logit -- equal scores the lower user row.  The rows depend on each other, so the
    chunk walk only stores every chunk's candidates (SlabLists.topk at `candidates`) and lse, and match() runs once after the last chunk:
    the subclass's index call, its rounds call in batches of `batch` rounds until a round changes nothing (state[4] < state[1]), its
    finish call.  The fixed point does not depend on the order or the batching of the rounds, so the table is bit-identical from run to
    run.  Over item shards every rank holds the same merged candidates and the same full-row lse, so every rank runs the same matching and
    nothing is exchanged.  The report and the explanations read the matched lists, in a second pass over the chunks."""

    whole = True
    MAX_C = 1024
    NOUN, FILL, MAX_ROUNDS, N_STATE = None, 0, 0, 0

    def __init__(self, value, candidates, score, batch):
        if score not in ("logprob", "logit"):
            raise ValueError("score must be logprob or logit")
        self.score = score
        self.candidates = None if candidates is None else int(candidates)
        if self.candidates is not None and not 1 <= self.candidates <= self.MAX_C:
            raise ValueError("candidates must be in [1, %d], got %r" % (self.MAX_C, candidates))
        self.batch = int(batch)
        if not 1 <= self.batch <= self.MAX_ROUNDS:
            raise ValueError("batch must be in [1, %d]" % self.MAX_ROUNDS)
        self.uniform = self.vec_host = None
        if isinstance(value, tuple):
            labels, n_groups, by_group = value
            labels = group_labels(labels, n_groups)
            self.vec_host = np.full(labels.size, self.FILL, np.int64)
            for g, v in dict(by_group).items():
                if not 0 <= int(g) < int(n_groups):
                    raise ValueError("group index %r outside [0, %d)" % (g, n_groups))
                self.vec_host[labels == int(g)] = int(v)
        elif np.ndim(value) == 0:
            self.uniform = int(value)
            if self.uniform != value:
                raise ValueError("a uniform %s is an integer, got %r" % (self.NOUN, value))
        else:
            self.vec_host = np.asarray(value).astype(np.int64).reshape(-1)
        low = self.uniform if self.vec_host is None else (int(self.vec_host.min()) if self.vec_host.size else 0)
        if low < 0:
            raise ValueError("a %s must be >= 0" % self.NOUN)
        self.c = self.n_items = self.cand_s = self.cand_i = self.lse = self.state = self.ws = self._stats = None

    @property
    def needs_lse(self):
        return self.score == "logprob"

    def bind(self, engine, rows, k, n_users):
        """-> the per-item values [n_items] int32 on the device; the subclass names them and sizes its workspace"""
        c = min(self.MAX_C, 4 * k) if self.candidates is None else self.candidates
        if not 1 <= k <= c <= self.MAX_C:
            raise ValueError("candidates must be in [k, %d] = [%d, %d], got %d" % (self.MAX_C, k, self.MAX_C, c))
        if n_users * c >= 2 ** 31:
            raise ValueError("%d users x %d candidates: the matching indexes fewer than 2^31 entries" % (n_users, c))
        n_items, dev = int(engine.I_global), engine.device
        vec = np.full(n_items, self.uniform, np.int64) if self.vec_host is None else self.vec_host
        if vec.size != n_items:
            raise ValueError("%s holds %d items, the catalogue %d" % (self.NOUN, vec.size, n_items))
        self.c, self.n_items, self.longest = c, n_items, c
        self.cand_s = torch.empty(n_users, c, dtype=torch.float32, device=dev)
        self.cand_i = torch.empty(n_users, c, dtype=torch.int32, device=dev)
        self.lse = torch.empty(n_users, dtype=torch.float32, device=dev) if self.needs_lse else None
        self.state = torch.zeros(self.N_STATE, dtype=torch.int32, device=dev)
        return torch.from_numpy(np.minimum(vec, 2 ** 31 - 1).astype(np.int32)).to(dev)

    def gather(self, lists, acts, tr, n, lo):
        lists.topk(acts, tr, n, self.c, self.cand_s[lo:lo + n], self.cand_i[lo:lo + n])
        if self.lse is not None:
            self.lse[lo:lo + n].copy_(acts.lse[:n])

    def rounds(self, batch_of_rounds, what):
        """batches of rounds (batch_of_rounds(): the engine's rounds call, bound) until one changes nothing -> the index of that round"""
        while True:
            batch_of_rounds()
            _, rounds, _, _, last = (int(x) for x in self.state[:5].cpu())
            if last < rounds:                            # the last round changed nothing: the fixed point
                return last
            if rounds > int(self.cand_i.shape[0]) * self.c + 1:      # (every round but the last removes at least one entry for good)
                raise LtgError("the %s matching has not converged after %d rounds" % (what, rounds))

    def plain_ids(self, k):
        """-> [n_users, k] int32 host array: the plain top-k lists, the first k columns of the candidates"""
        return self.cand_i[:, :k].cpu().numpy()

    def stats(self):
        return dict(self._stats)


class ExposureCap(_Matching):
    """A serve-time rule over the WHOLE split, passed as `cap=` to a Recommender / ShardedRecommender: no item appears in more than its
    cap of the served lists (so the report's item_hits <= cap), and the slots an over-full item gives up go to the best alternatives of
    the users it turned away.  cap, candidates, score, batch: _Matching's; an item outside the capped groups is UNCAPPED.  The lists are
    the user-optimal stable matching of user-proposing deferred acceptance; a user whose candidates run out gets a short list.  match():
    ltg_cap_index, ltg_cap_rounds until a round raises no threshold, ltg_cap_finish.  After run(): stats() -> dict: rounds (up to and
    including the first that raised no threshold), raises (threshold raises), passed_over (candidate entries a user's walk passed
    over), short (users with fewer than k entries)."""

    UNCAPPED = 2 ** 31 - 1
    NOUN, FILL, MAX_ROUNDS, N_STATE = "cap", UNCAPPED, LTG_CAP_MAX_ROUNDS, LTG_CAP_STATE

    def __init__(self, cap, candidates=None, score="logprob", batch=4):
        super().__init__(cap, candidates, score, batch)
        self.cap = None

    def bind(self, engine, rows, k, n_users):
        self.cap = super().bind(engine, rows, k, n_users)
        self.ws = torch.empty(max(1, engine.cap_ws_bytes(n_users, self.c, self.n_items)), dtype=torch.uint8, device=engine.device)

    def match(self, engine, k, score_out, id_out):
        if int(self.cand_i.shape[0]) == 0:
            self._stats = dict(rounds=0, raises=0, passed_over=0, short=0)
            return
        engine.cap_index(self.cand_i, self.n_items, self.state, self.ws)
        last = self.rounds(lambda: engine.cap_rounds(self.cand_s, self.cand_i, self.lse, self.cap, k, self.batch, self.state, self.ws), "capped")
        engine.cap_finish(self.cand_s, self.cand_i, self.n_items, k, score_out, id_out, self.state, self.ws)
        st = [int(x) for x in self.state.cpu()]
        self._stats = dict(rounds=last + 1, raises=st[0], passed_over=st[2], short=st[3])

    def cap_vector(self):
        """-> [n_items] int32 host array: the cap per GLOBAL item id (UNCAPPED where none applies)"""
        return self.cap.cpu().numpy()


class ExposureFloor(_Matching):
    """A serve-time rule over the WHOLE split, passed as `floor=` to a Recommender / ShardedRecommender, the dual of ExposureCap: every
    item with a floor M reaches M of the served lists if that many users hold it among their candidates and can spare a slot (so the
    report's item_hits >= min(floor, held)) -- the first audience a new or niche item needs.  floor, candidates, score, batch:
    _Matching's; 0 is no floor.  reserve: how many of the last slots of a user's list floor items may take, 0 <= reserve <= k; the first
    k - reserve entries of every list are the plain ones.  The lists are the item-optimal stable matching of item-proposing deferred
    acceptance: an item proposes to the users that hold it among their candidates, best score first, and a user keeps, of the proposals
    behind position k - reserve, the `reserve` it likes best.  Every list stays in score order and every entry keeps its logit.  match():
    ltg_floor_index, ltg_floor_rounds until a round lowers no limit, ltg_floor_finish.  After run(): held(), and stats() -> dict: rounds
    (up to and including the first that lowered no limit), lowerings (limit lowerings), floor_items, short_items (floor items that hold
    fewer entries than their floor), rows_changed (users whose list differs from the plain top-k), inserted (slots that went to entries
    from behind position k - t, summed over the users)."""

    NOUN, FILL, MAX_ROUNDS, N_STATE = "floor", 0, LTG_FLOOR_MAX_ROUNDS, LTG_FLOOR_STATE

    def __init__(self, floor, reserve, candidates=None, score="logprob", batch=4):
        self.reserve = int(reserve)
        if self.reserve != reserve or self.reserve < 0:
            raise ValueError("reserve is an integer >= 0, got %r" % (reserve,))
        super().__init__(floor, candidates, score, batch)
        self.need = self.held_d = None

    def bind(self, engine, rows, k, n_users):
        if self.reserve > k:
            raise ValueError("reserve must be in [0, k] = [0, %d], got %d" % (k, self.reserve))
        self.need = super().bind(engine, rows, k, n_users)
        self.held_d = torch.zeros(self.n_items, dtype=torch.int32, device=engine.device)
        self.ws = torch.empty(max(1, engine.floor_ws_bytes(n_users, self.c, self.n_items)), dtype=torch.uint8, device=engine.device)

    def match(self, engine, k, score_out, id_out):
        if int(self.cand_i.shape[0]) == 0:
            self.held_d.zero_()
            self._stats = dict(rounds=0, lowerings=0, floor_items=int((self.need > 0).sum()), short_items=0, rows_changed=0, inserted=0)
            return
        engine.floor_index(self.cand_i, self.n_items, self.state, self.ws)
        last = self.rounds(lambda: engine.floor_rounds(self.cand_s, self.cand_i, self.lse, self.need, k, self.reserve, self.batch, self.state,
                                                       self.ws), "floor")
        engine.floor_finish(self.cand_s, self.cand_i, self.lse, self.need, k, self.reserve, score_out, id_out, self.state, self.ws,
                            held_out=self.held_d)
        st = [int(x) for x in self.state.cpu()]
        self._stats = dict(rounds=last + 1, lowerings=st[0], floor_items=st[6], short_items=st[2], rows_changed=st[3], inserted=st[5])

    def need_vector(self):
        """-> [n_items] int32 host array: the floor per GLOBAL item id (0 where none applies)"""
        return self.need.cpu().numpy()

    def held(self):
        """-> [n_items] int32 host array: the lists the matching gives every item (0 for items without a floor); an item is served in at
        least min(floor, held) lists, and held < floor means too few users hold it among their candidates or can spare a slot"""
        return self.held_d.cpu().numpy()


class ShareTarget(Rule):
    """A serve-time rule over the WHOLE split, passed as `share=` to a Recommender / ShardedRecommender: the item groups `promote` (group
    indices; labels: one uint8 per GLOBAL item id, the labels a LongTailReport takes) get the part `share` of ALL served slots, and the
    promoted slots go where they cost the least relevance -- not the same number to every user, as MinSlots gives.  For a user, one more
    promoted slot costs the score of the worst remaining other entry minus the score of the best promoted item not yet in the list; these
    step costs never decrease along a user's list, so the cheapest way to a total of want = ceil(share * n_users * k) promoted slots is the
    globally cheapest steps: one selection, no rounds.  Like the cap the rows depend on each other: the chunk walk only stores every
    chunk's two lists of k entries (SlabLists.topk with the promoted groups' mask and with its complement), and match() makes ONE call of
    ltg_topk_share after the last chunk.  Every row stays sorted and every entry keeps its score.  share = 0, or a target the plain
    lists already meet, gives the plain lists bit for bit; a target beyond what the promoted groups can fill gives every row at its
    limit (stats()["reached"] is then False).  Over item shards every rank holds the same merged lists and runs the same call: nothing
    is exchanged.  The report and the explanations read the final lists, in a second pass over the chunks.  After run(): stats()."""

    whole = True

    def __init__(self, labels, n_groups, promote, share):
        self.labels_host, self.n_groups = group_labels(labels, n_groups), int(n_groups)
        self.promote = sorted({int(g) for g in promote})
        self.mask = group_mask_of(self.promote, self.n_groups)           # (raises for an index outside the groups and for an empty list)
        self.rest_mask = 0x1FF & ~self.mask                              # every other label, those in no group (bit 8) included
        self.share = float(share)
        if not 0.0 <= self.share <= 1.0:             # (NaN fails both comparisons)
            raise ValueError("share must be in [0, 1], got %r" % (share,))
        self.k = self.want = self.labels = self.pro_s = self.pro_i = self.rest_s = self.rest_i = self.state = self.ws = self._stats = None

    def bind(self, engine, rows, k, n_users):
        if not 1 <= k <= 1024:
            raise ValueError("k must be in [1, 1024], got %d" % k)
        if n_users * k >= 2 ** 31:
            raise ValueError("%d users x %d entries: the selection indexes fewer than 2^31 steps" % (n_users, k))
        self.labels = group_labels(self.labels_host, self.n_groups, engine)
        dev = engine.device
        self.k = self.longest = int(k)
        self.want = int(np.ceil(np.float64(self.share) * n_users * k))
        self.pro_s = torch.empty(n_users, k, dtype=torch.float32, device=dev)
        self.pro_i = torch.empty(n_users, k, dtype=torch.int32, device=dev)
        self.rest_s = torch.empty(n_users, k, dtype=torch.float32, device=dev)
        self.rest_i = torch.empty(n_users, k, dtype=torch.int32, device=dev)
        self.state = torch.zeros(LTG_SHARE_STATE, dtype=torch.int32, device=dev)
        self.ws = torch.empty(max(1, engine.share_ws_bytes(n_users, k)), dtype=torch.uint8, device=dev)

    def gather(self, lists, acts, tr, n, lo):
        lists.topk(acts, tr, n, self.k, self.pro_s[lo:lo + n], self.pro_i[lo:lo + n], self.labels, self.mask)
        lists.topk(acts, tr, n, self.k, self.rest_s[lo:lo + n], self.rest_i[lo:lo + n], self.labels, self.rest_mask)

    def match(self, engine, k, score_out, id_out):
        st = [0] * LTG_SHARE_STATE
        if int(self.pro_i.shape[0]) > 0:
            engine.topk_share(self.pro_s, self.pro_i, self.rest_s, self.rest_i, k, self.want, score_out, id_out, self.state, self.ws)
            st = [int(x) for x in self.state.cpu()]
        A, N, take, changed, bits, served = st[:6]
        price = float(np.array([bits], np.int32).view(np.float32)[0])
        self._stats = dict(plain_share=A / served if served else float("nan"), share=(A + take) / served if served else float("nan"),
                           target=self.share, taken=take, available=N, rows_changed=changed, price=price, reached=A + take >= self.want)

    def stats(self):
        """-> dict: plain_share / share (the promoted part of the served slots before / after), target, taken (steps taken), available
        (steps there are), rows_changed, price (the cost of the dearest step taken: the marginal relevance price of a promoted slot; 0.0
        when none was taken), reached (the promoted slots are at least ceil(target * n_users * k))"""
        return dict(self._stats)


class Explain:
    """Why a user got each list entry, passed as `explain=` to a Recommender / ShardedRecommender: for the first `top` entries of every
    user's list (default min(k, 256)) the r items of that user's fold-in history nearest to the entry -- "because you interacted with X
    and Y".  Nearness is ItemNeighbors': the product of the two items' rows in the bf16 image of the `decoder` (W_p1t) or `encoder` (W_q0)
    table, `cosine` or `dot`; an entry never explains itself.  The image is packed once per run() (a Diversify of the same space and
    metric shares its image); per chunk ONE launch of ltg_topk_explain on whatever list is served -- plain, ruled or diversified -- and
    the top x history scores never leave the chip.  Over item shards every rank explains from its slab's part of the histories, and the
    SlabLists gathers and merges the [n * top, r] lists: every rank ends with the table of the unsharded run, bit for bit.
    After run(): why_i / why_s [n_users, top, r] on the device (ids are GLOBAL item ids, ordered and padded as ltg_topk writes a
    list); table() brings both to the host."""

    MAX_TOP, MAX_R = 256, 8                          # LTG_WHY_MAX_TOP, LTG_WHY_MAX_R

    def __init__(self, r=3, top=None, space="decoder", metric="cosine"):
        self.r = int(r)
        if not 1 <= self.r <= self.MAX_R:
            raise ValueError("r must be in [1, %d], got %r" % (self.MAX_R, r))
        self.top_arg = None if top is None else int(top)
        if self.top_arg is not None and not 1 <= self.top_arg <= self.MAX_TOP:
            raise ValueError("top must be in [1, %d], got %r" % (self.MAX_TOP, top))
        if space not in LTG_SPACE or metric not in LTG_METRIC:
            raise ValueError("space must be decoder or encoder, metric cosine or dot")
        self.space, self.metric = space, metric
        self.top = self.image = self.why_s = self.why_i = None
        self.image_lo = 0

    def bind(self, engine, k, n_users):
        """the device tables for lists of k entries and a split of n_users"""
        top = min(k, self.MAX_TOP) if self.top_arg is None else self.top_arg
        if not 1 <= top <= min(k, self.MAX_TOP):
            raise ValueError("top must be in [1, min(k, %d)] = [1, %d], got %d" % (self.MAX_TOP, min(k, self.MAX_TOP), top))
        if not 1 <= self.r <= self.MAX_R:
            raise ValueError("r must be in [1, %d], got %d" % (self.MAX_R, self.r))
        self.top = top
        dev = engine.device
        self.why_s = torch.empty(n_users, top, self.r, dtype=torch.float32, device=dev)
        self.why_i = torch.empty(n_users, top, self.r, dtype=torch.int32, device=dev)

    def pack(self, engine, group=None, share=None):
        """the image of the whole catalogue, once per run(); share: the walk's policy -- a Diversify of the same space and metric has
        packed the same image for this run already"""
        if isinstance(share, Diversify) and (share.space, share.metric) == (self.space, self.metric):
            self.image = share.image
        else:
            self.image = catalogue_image(engine, self.space, self.metric, self.image, group)

    def apply(self, lists, tr, n, lo, ids):
        """the explanations of users lo .. lo + n, whose final lists are ids [n, k]; lists: the SlabLists whose buffers the per-slab
        explanations are gathered through"""
        top, r = self.top, self.r
        out_s, out_i = self.why_s[lo:lo + n].view(n * top, r), self.why_i[lo:lo + n].view(n * top, r)
        ls, li = lists.local(n * top, r, out_s, out_i)
        lists.eng.topk_explain(self.image, self.image_lo, tr, ids, top, r, ls.view(n, top, r), li.view(n, top, r))
        lists.merge(ls, li, out_s, out_i)

    def table(self):
        """-> (ids [n_users, top, r] int32 global item ids, scores [n_users, top, r] float32) host arrays"""
        return self.why_i.cpu().numpy(), self.why_s.cpu().numpy()


def gate_tau(min_prob):
    """the logit threshold of a CriticGate: float32(log(p / (1 - p))) computed in fp64; p = 0 -> -inf (everything passes)"""
    p = float(min_prob)
    if not 0.0 <= p < 1.0:                           # (NaN fails both comparisons)
        raise ValueError("min_prob must be in [0, 1), got %r" % (min_prob,))
    return np.float32(-np.inf) if p == 0.0 else np.float32(np.log(np.float64(p)) - np.log1p(-np.float64(p)))


class _CriticSides:
    """What Critic and CriticGate share: the two sides of the discriminator among the items with features (niche_ids: load_pop_niche_tags'
    niche items, valid_ids: load_valid_item_ids' items with features; both GLOBAL ids), their side images and the item id -> image row
    maps, packed once per run(), and the evaluation of a chunk's lists (ltg_pair_critic, over item shards the exchange, ltg_critic_finish)."""

    def __init__(self, niche_ids, valid_ids):
        niche = np.unique(np.fromiter((int(x) for x in niche_ids), np.int64))
        valid = np.unique(np.fromiter((int(x) for x in valid_ids), np.int64))
        if (niche.size and niche.min() < 0) or (valid.size and valid.min() < 0):
            raise ValueError("item ids must be >= 0")
        self.niche_host = np.intersect1d(niche, valid).astype(np.int32)              # niche with features, ascending
        self.pop_host = np.setdiff1d(valid, niche).astype(np.int32)                  # popular with features, ascending
        self.pop_ids = self.niche_ids = self.pop_row = self.niche_row = self.pop_img = self.niche_img = None

    def bind(self, engine):
        n_items, dev = int(engine.I_global), engine.device
        for name, a in (("niche", self.niche_host), ("popular", self.pop_host)):
            if a.size and a.max() >= min(n_items, int(engine.feature_len)):
                raise ValueError("%s ids outside [0, %d)" % (name, min(n_items, int(engine.feature_len))))
        maps = []
        for a in (self.pop_host, self.niche_host):
            m = np.full(n_items, -1, np.int32)
            m[a] = np.arange(a.size, dtype=np.int32)
            maps.append(torch.from_numpy(m).to(dev))
        self.pop_row, self.niche_row = maps
        self.pop_ids, self.niche_ids = torch.from_numpy(self.pop_host).to(dev), torch.from_numpy(self.niche_host).to(dev)

    def pack(self, engine):
        """both side images, from the discriminator as it is now (replicated over item shards: every rank packs for itself)"""
        self.pop_img = engine.pair_pack("popular", self.pop_ids, out=self.pop_img)
        self.niche_img = engine.pair_pack("niche", self.niche_ids, out=self.niche_img)

    def evaluate(self, lists, tr, ids, top, acc, cnt, best_s, best_i, crit, scored):
        """the first `top` entries of the lists ids [n, k_in] -> crit / best_s / best_i [n, top], cnt [n] (the users' anchors), scored [n];
        acc [n, top] int64 is the buffer of the fixed-point sums.  lists: the SlabLists whose buffers the per-slab best anchors are
        gathered through -- over item shards every rank sees its slab's part of the histories, the sums and counts are added as
        integers and the best anchors merged, so every rank finishes identically."""
        eng, n = lists.eng, int(ids.shape[0])
        ls, li = lists.local(n * top, 1, best_s.view(n * top, 1), best_i.view(n * top, 1))
        eng.pair_critic(self.pop_img, self.niche_img, self.pop_row, self.niche_row, tr, ids, top, acc, cnt, ls.view(n, top), li.view(n, top),
                        hist_lo=eng.item_lo if lists.parts > 1 else 0)
        if lists.parts > 1:
            dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=lists.group)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=lists.group)
            lists.merge(ls, li, best_s.view(n * top, 1), best_i.view(n * top, 1))
        eng.critic_finish(ids, top, self.niche_row, int(self.niche_host.size), acc, cnt, crit, scored)


class Critic:
    """What the discriminator thinks of every list entry, passed as `critic=` to a Recommender / ShardedRecommender: for the first `top`
    entries of every user's list (default min(k, 256)) that are niche items with features, the mean pair logit crit(u, b) = mean over the
    user's anchors a (the popular items with features of the fold-in history) of s(a, b), PairCompanions' score -- sigmoid(crit) is the
    geometric-mean-odds probability the discriminator gives "a real user with these head items holds b" -- and the best anchor argmax_a
    s(a, b).  An entry is scored iff it is such a niche item and its user has an anchor.  The mean is taken over 64-bit fixed-point
    integers (ltg_pair_critic), so it does not depend on how the anchors are split.  An attachment like Explain: it reads the final lists,
    plain, ruled, diversified or matched.  niche_ids / valid_ids: GLOBAL ids, load_pop_niche_tags' niche items and load_valid_item_ids'
    items with features.  Both images are packed once per run(); per chunk ONE launch of ltg_pair_critic and one of ltg_critic_finish.
    Over item shards every rank scores its slab's part of the histories; the sums and counts are all-reduced as integers and the best
    anchors merged by the SlabLists: every rank ends with the table of the unsharded run, bit for bit.  After run(): table(), summary()."""

    MAX_TOP = 256                                    # LTG_CRITIC_MAX_TOP

    def __init__(self, niche_ids, valid_ids, top=None):
        self.top_arg = None if top is None else int(top)
        if self.top_arg is not None and not 1 <= self.top_arg <= self.MAX_TOP:
            raise ValueError("top must be in [1, %d], got %r" % (self.MAX_TOP, top))
        self.sides = _CriticSides(niche_ids, valid_ids)
        self.top = self.crit = self.anchor_s = self.anchor_i = self.n_anchor = self.scored = self.acc = None

    def bind(self, engine, rows, k, n_users):
        """the device tables for chunks of up to `rows` users, lists of k entries and a split of n_users"""
        top = min(k, self.MAX_TOP) if self.top_arg is None else self.top_arg
        if not 1 <= top <= min(k, self.MAX_TOP):
            raise ValueError("top must be in [1, min(k, %d)] = [1, %d], got %d" % (self.MAX_TOP, min(k, self.MAX_TOP), top))
        self.top = top
        self.sides.bind(engine)
        dev = engine.device
        self.crit = torch.zeros(n_users, top, dtype=torch.float32, device=dev)
        self.anchor_s = torch.full((n_users, top), float("-inf"), dtype=torch.float32, device=dev)
        self.anchor_i = torch.full((n_users, top), -1, dtype=torch.int32, device=dev)
        self.n_anchor = torch.zeros(n_users, dtype=torch.int32, device=dev)
        self.scored = torch.zeros(n_users, dtype=torch.int32, device=dev)
        self.acc = torch.empty(rows * top, dtype=torch.int64, device=dev)

    def pack(self, engine):
        self.sides.pack(engine)

    def apply(self, lists, tr, n, lo, ids):
        """the critic of users lo .. lo + n, whose final lists are ids [n, k]"""
        top = self.top
        self.sides.evaluate(lists, tr, ids, top, self.acc[: n * top].view(n, top), self.n_anchor[lo:lo + n], self.anchor_s[lo:lo + n],
                            self.anchor_i[lo:lo + n], self.crit[lo:lo + n], self.scored[lo:lo + n])

    def table(self):
        """-> dict of host arrays: crit [n_users, top] float32 (0.0 where unscored), anchor_i [n_users, top] int32 GLOBAL ids (-1 where
        unscored: the flag), anchor_s [n_users, top] float32 (-inf where unscored), n_anchor [n_users] int32"""
        return dict(crit=self.crit.cpu().numpy(), anchor_i=self.anchor_i.cpu().numpy(), anchor_s=self.anchor_s.cpu().numpy(),
                    n_anchor=self.n_anchor.cpu().numpy())

    def summary(self):
        """-> dict: scored (entries), users_with_anchors, mean_prob (the mean sigmoid(crit) over the scored entries; nan without any)"""
        t = self.table()
        ok = t["anchor_i"] >= 0
        with np.errstate(over="ignore"):
            prob = 1.0 / (1.0 + np.exp(-t["crit"][ok].astype(np.float64)))
        return dict(scored=int(ok.sum()), users_with_anchors=int((t["n_anchor"] > 0).sum()),
                    mean_prob=float(prob.mean()) if prob.size else float("nan"))


class CriticGate(Rule):
    """A serve-time rule, passed as `gate=` to a Recommender / ShardedRecommender: a niche entry stays in a user's list only if the
    discriminator gives it at least min_prob beside that user's popular history items.  Each user's `candidates` best items (ltg_topk;
    default min(256, 2 k), k <= candidates <= 256) get Critic's mean anchor logit; walking them in order, an entry passes iff it is
    unscored (a popular item, an item without features, a user without anchors) or crit >= tau = float32(logit(min_prob)), and the first k
    passing entries are the list, with their scores -- a subsequence of the plain ranking, so in score order; fewer than k passing
    entries leave a short list.  min_prob = 0 is the plain list.  Both images are packed once per run(); per chunk ltg_topk at
    `candidates`, ltg_pair_critic, ltg_critic_finish and ltg_topk_gate.  Over item shards the candidates are merged by the SlabLists and
    the critic's sums, counts and best anchors exchanged as Critic's are, so every rank gates the same candidates identically.  After
    run(): stats() [n_users, 3] = scored candidates, candidates rejected before the list was full, list length."""

    MAX_C = 256                                      # LTG_GATE_MAX_C

    def __init__(self, niche_ids, valid_ids, min_prob, candidates=None):
        self.tau = gate_tau(min_prob)
        self.min_prob = float(min_prob)
        self.candidates = None if candidates is None else int(candidates)
        if self.candidates is not None and not 1 <= self.candidates <= self.MAX_C:
            raise ValueError("candidates must be in [1, %d], got %r" % (self.MAX_C, candidates))
        self.sides = _CriticSides(niche_ids, valid_ids)
        self.c = self.stat = None

    def bind(self, engine, rows, k, n_users):
        c = min(self.MAX_C, 2 * k) if self.candidates is None else self.candidates
        if not k <= c <= self.MAX_C:
            raise ValueError("candidates must be in [k, %d] = [%d, %d], got %d" % (self.MAX_C, k, self.MAX_C, c))
        self.c = self.longest = c
        self.sides.bind(engine)
        dev = engine.device
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        self.cand_s, self.cand_i, self.crit, self.best_s, self.best_i = f32(rows * c), i32(rows * c), f32(rows * c), f32(rows * c), i32(rows * c)
        self.acc = torch.empty(rows * c, dtype=torch.int64, device=dev)
        self.cnt, self.scored = i32(rows), i32(rows)
        self.stat = torch.zeros(n_users, 3, dtype=torch.int32, device=dev)

    def begin(self, engine, group=None):
        self.sides.pack(engine)

    def apply(self, lists, acts, tr, n, k, lo, score_out, id_out):
        c = self.c
        v = lambda t: t[: n * c].view(n, c)
        c_s, c_i, crit, b_s, b_i = v(self.cand_s), v(self.cand_i), v(self.crit), v(self.best_s), v(self.best_i)
        lists.topk(acts, tr, n, c, c_s, c_i)
        self.sides.evaluate(lists, tr, c_i, c, v(self.acc), self.cnt[:n], b_s, b_i, crit, self.scored[:n])
        lists.eng.topk_gate(c_s, c_i, crit, b_i, self.tau, k, score_out, id_out, self.stat[lo:lo + n])

    def stats(self):
        """-> [n_users, 3] int32 host array: scored candidates, candidates rejected before the list was full, list length"""
        return self.stat.cpu().numpy()


class Explore(Rule):
    """Exploration lists, passed as `explore=` to a Recommender / ShardedRecommender: randomised exposure with logged propensities.  The
    first `fixed` entries of a user's list are the plain top-`fixed` (log-probability 0.0); the other k - fixed are drawn without
    replacement from the remaining eligible items in proportion to exp(logit / temperature) -- the Plackett-Luce policy -- and every entry
    carries the log of its conditional probability given the earlier picks.  The draw is Gumbel-top-k with the counter RNG at
    (engine seed, stream 8, draw, global user row * n_items + global item id): the same `draw` gives the same lists whatever the chunk
    size, the slab or the rank; another `draw` gives another sample.  Per chunk: the plain top-`fixed` (if any), ltg_topk_sample,
    ltg_topk_sample_mass, ltg_topk_sample_finish, and one plain list of k for the explored share.  Over item shards the per-slab keys
    are gathered and merged by the SlabLists, and three small all-reduces join the mass (max of the largest eligible logit, sum of the
    rescaled rest, max of the picks' logits): ids, scores and keys are those of the unsharded run bit for bit, logp up to the rounding of
    the sum.  The lists keep every pick's raw logit, in draw order, so they are generally not descending; the report, the explanations and
    the critic read them unchanged.  After run(): logp / keys [n_users, k] on the device (a head entry has key +inf), table(), stats()."""

    def __init__(self, temperature, fixed=0, draw=0):
        self.temperature = float(temperature)
        if not (self.temperature > 0.0 and np.isfinite(self.temperature)):     # (NaN fails the comparison)
            raise ValueError("temperature must be > 0 and finite, got %r" % (temperature,))
        with np.errstate(over="ignore"):
            self.inv_temp = np.float32(1.0 / self.temperature)
        if not (self.inv_temp > 0 and np.isfinite(self.inv_temp)):
            raise ValueError("1 / temperature is not a positive finite float32, got temperature %r" % (temperature,))
        self.fixed, self.draw = int(fixed), int(draw)
        if self.fixed != fixed or self.fixed < 0:
            raise ValueError("fixed is an integer >= 0, got %r" % (fixed,))
        if self.draw != draw or not 0 <= self.draw < 2 ** 64:
            raise ValueError("draw is an integer >= 0, got %r" % (draw,))
        self.k = self.logp = self.keys = self.explored = self.sampled = None

    def bind(self, engine, rows, k, n_users):
        if not 0 <= self.fixed < k:
            raise ValueError("fixed must be in [0, k) = [0, %d), got %d" % (k, self.fixed))
        if not 1 <= k <= 1024:
            raise ValueError("k must be in [1, 1024], got %d" % k)
        dev, F = engine.device, self.fixed
        self.k = self.longest = int(k)
        m = k - F
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        self.head_s, self.head_i = f32(rows * max(1, F)), i32(rows * max(1, F))
        self.pick_key, self.pick_i, self.pick_s, self.pick_lp = f32(rows * m), i32(rows * m), f32(rows * m), f32(rows * m)
        self.plain_s, self.plain_i = f32(rows * k), i32(rows * k)
        self.max, self.top, self.rest = f32(rows), f32(rows), f32(rows)
        self.logp = torch.zeros(n_users, k, dtype=torch.float32, device=dev)
        self.keys = torch.full((n_users, k), float("inf"), dtype=torch.float32, device=dev)
        self.explored = torch.zeros(n_users, dtype=torch.int32, device=dev)
        self.sampled = torch.zeros(n_users, dtype=torch.int32, device=dev)

    def apply(self, lists, acts, tr, n, k, lo, score_out, id_out):
        eng, F, m, it = lists.eng, self.fixed, k - self.fixed, float(self.inv_temp)
        v = lambda t, L: t[: n * L].view(n, L)
        head_s, head_i = (v(self.head_s, F), v(self.head_i, F)) if F else (None, None)
        if F:                                            # the fixed head: the plain top-F
            lists.topk(acts, tr, n, F, head_s, head_i)
        key, ids, sc, lp = v(self.pick_key, m), v(self.pick_i, m), v(self.pick_s, m), v(self.pick_lp, m)
        ls, li = lists.local(n, m, key, ids)
        eng.topk_sample(acts, tr, lo, m, it, self.draw, head_i, ls, li)
        lists.merge(ls, li, key, ids)                    # (on the keys: a key does not depend on the slab that holds the item)
        mx, top, rest = self.max[:n], self.top[:n], self.rest[:n]
        eng.topk_sample_mass(acts, tr, it, head_i, ids, sc, mx, rest)
        if lists.parts > 1:                              # the mass of the whole row from the slabs' parts
            top.copy_(mx)
            dist.all_reduce(top, op=dist.ReduceOp.MAX, group=lists.group)
            rest.mul_(torch.where(torch.isinf(mx), torch.zeros_like(mx), torch.exp((mx - top) * it)))   # (a slab without an eligible item)
            dist.all_reduce(rest, op=dist.ReduceOp.SUM, group=lists.group)
            dist.all_reduce(sc, op=dist.ReduceOp.MAX, group=lists.group)
        else:
            top = mx
        eng.topk_sample_finish(sc, top, rest, it, lp)
        if F:
            score_out[:, :F].copy_(head_s)
            id_out[:, :F].copy_(head_i)
        score_out[:, F:].copy_(sc)
        id_out[:, F:].copy_(ids)
        self.logp[lo:lo + n, F:].copy_(lp)
        self.keys[lo:lo + n, F:].copy_(key)
        # the explored share: a sampled entry is outside the plain top-k iff it comes after that list's last entry in ltg_topk's order
        p_s, p_i = v(self.plain_s, k), v(self.plain_i, k)
        lists.topk(acts, tr, n, k, p_s, p_i)
        last_s, last_i = p_s[:, k - 1:k], p_i[:, k - 1:k]
        real = ids >= 0
        outside = real & (last_i >= 0) & ((sc < last_s) | ((sc == last_s) & (ids > last_i)))
        self.explored[lo:lo + n].copy_(outside.sum(1))
        self.sampled[lo:lo + n].copy_(real.sum(1))

    def table(self):
        """-> [n_users, k] float32 host array: the conditional log-probability of every entry (0.0 for the fixed head and padding)"""
        return self.logp.cpu().numpy()

    def stats(self):
        """-> dict: mean_logp (the mean over the users of a list's log-propensity, the sum of its entries' logp), explored_share (the
        share of the sampled slots whose item is not in the plain top-k of the same user), sampled (those slots)"""
        lp = self.logp.sum(1, dtype=torch.float64)
        n_s = int(self.sampled.sum())
        return dict(mean_logp=float(lp.mean()) if lp.numel() else float("nan"),
                    explored_share=int(self.explored.sum()) / n_s if n_s else float("nan"), sampled=n_s)


def inv_temp_of(temperature):
    """float32(1 / T) as Explore forms it, refused where T or the result is not positive and finite"""
    T = float(temperature)
    if not (T > 0.0 and np.isfinite(T)):                 # (NaN fails the comparison)
        raise ValueError("temperature must be > 0 and finite, got %r" % (temperature,))
    with np.errstate(over="ignore"):
        it = np.float32(1.0 / T)
    if not (it > 0 and np.isfinite(it)):
        raise ValueError("1 / temperature is not a positive finite float32, got temperature %r" % (temperature,))
    return it


class ReplayLog:
    """An exploration log on the host: for user row r of a split the served list ids[r] (GLOBAL item ids, -1 = padding, distinct within a
    row), logp0[r] (the log of the conditional probability with which every entry was shown, as Explore.table() gives it: <= 0, and 0.0
    for padding and for the first `fixed` slots, the logging policy's fixed head) and reward[r] (a finite float per entry, e.g. 1.0 =
    clicked; None until rewards_from / rewards_from_file fills it).  uids: the uid of every row where the log came from a file.  A
    ValueError names the first row that breaks a rule."""

    def __init__(self, ids, logp0, reward=None, fixed=0, n_items=None, uids=None):
        ids, logp0 = np.asarray(ids), np.asarray(logp0)
        if ids.ndim != 2 or logp0.shape != ids.shape:
            raise ValueError("ids and logp0 must be [n_users, k] arrays of one shape, got %r and %r" % (ids.shape, logp0.shape))
        self.n, self.k = int(ids.shape[0]), int(ids.shape[1])
        if not 1 <= self.k <= 1024:
            raise ValueError("k must be in [1, 1024], got %d" % self.k)
        self.fixed = int(fixed)
        if self.fixed != fixed or not 0 <= self.fixed < self.k:
            raise ValueError("fixed must be an integer in [0, k) = [0, %d), got %r" % (self.k, fixed))
        if not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("ids must be integers")
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        self.logp0 = np.ascontiguousarray(logp0, dtype=np.float32)
        self.n_items = None
        self.check_ids(n_items)
        srt = np.sort(self.ids, 1)
        self._refuse((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0), "holds an item twice")
        self.ids = self.ids.astype(np.int32)
        pad = self.ids < 0
        with np.errstate(invalid="ignore"):
            self._refuse(~(np.isfinite(self.logp0) & (self.logp0 <= 0)), "has a logp0 that is not finite and <= 0")
        self._refuse(pad & (self.logp0 != 0), "has a logp0 other than 0.0 on padding")
        self._refuse((self.logp0 != 0)[:, : self.fixed], "has a logp0 other than 0.0 in the fixed head")
        self.uids = None if uids is None else np.asarray(uids, np.int64).reshape(-1)
        if self.uids is not None and self.uids.size != self.n:
            raise ValueError("uids holds %d rows, the log %d" % (self.uids.size, self.n))
        self.reward = None
        if reward is not None:
            self.set_reward(reward)

    @staticmethod
    def _refuse(bad, what):
        if bad.any():
            raise ValueError("row %d %s" % (int(np.nonzero(bad.any(1))[0][0]), what))

    def check_ids(self, n_items):
        """ids in [0, n_items) or -1 (n_items None: >= -1 only; Replay checks against the catalogue when it is bound)"""
        self._refuse(self.ids < -1, "has an id below -1")
        if n_items is not None:
            self._refuse(self.ids >= int(n_items), "has an id outside [0, %d)" % int(n_items))
            self.n_items = int(n_items)

    def set_reward(self, reward):
        reward = np.asarray(reward)
        if reward.shape != self.ids.shape:
            raise ValueError("reward must be [n_users, k] = %r, got %r" % (self.ids.shape, reward.shape))
        reward = np.ascontiguousarray(reward, dtype=np.float32)
        self._refuse(~np.isfinite(reward), "has a reward that is not finite")
        self.reward = reward
        return reward

    @classmethod
    def from_npz(cls, path, reward=None, fixed=0, n_items=None):
        """what recommend.py --explore --npz writes: uids [n], ids [n, k], logp [n, k]"""
        z = np.load(path)
        for name in ("uids", "ids", "logp"):
            if name not in z.files:
                raise ValueError("%s holds no `%s`: not the npz of recommend.py --explore" % (path, name))
        return cls(z["ids"], z["logp"], reward=reward, fixed=fixed, n_items=n_items, uids=z["uids"])

    @classmethod
    def from_tsv(cls, path, k, reward=None, fixed=0, n_items=None):
        """recommend.py's props.tsv: one line per user, `uid<TAB>sid:logp,...` in list order, padded here to k entries"""
        uids, rows = [], []
        for n_line, line in enumerate(open(path).read().splitlines()):
            uid, _, rest = line.partition("\t")
            cells = [c.split(":") for c in rest.split(",") if c]
            if len(cells) > int(k) or any(len(c) != 2 for c in cells):
                raise ValueError("%s line %d: expected at most %d fields sid:logp" % (path, n_line + 1, int(k)))
            uids.append(int(uid))
            rows.append(cells)
        ids = np.full((len(rows), int(k)), -1, np.int64)
        logp = np.zeros((len(rows), int(k)), np.float32)
        for r, cells in enumerate(rows):
            ids[r, : len(cells)] = [int(c[0]) for c in cells]
            logp[r, : len(cells)] = [float(c[1]) for c in cells]
        return cls(ids, logp, reward=reward, fixed=fixed, n_items=n_items, uids=uids)

    def rewards_from(self, te):
        """reward 1.0 where the shown item is a held-out item of the user (te: the split's held-out CSR, rows aligned with the log)"""
        te = te.tocsr()
        if te.shape[0] != self.n:
            raise ValueError("the held-out rows hold %d users, the log %d" % (te.shape[0], self.n))
        y = np.zeros(self.ids.shape, np.float32)
        for r in range(self.n):
            y[r] = np.isin(self.ids[r], te.indices[te.indptr[r]:te.indptr[r + 1]])
        return self.set_reward(y)

    def rewards_from_file(self, path, uid_start=None):
        """lines `uid<TAB>sid[,sid...]`: reward 1.0 for the listed items of that user; a user without a line has none.  The uid of row r
        is uids[r] where the log has them, else uid_start + r"""
        if self.uids is None and uid_start is None:
            raise ValueError("the log has no uids: pass uid_start")
        uids = self.uids if self.uids is not None else np.arange(self.n, dtype=np.int64) + int(uid_start)
        row_of = {int(u): r for r, u in enumerate(uids.tolist())}
        y = np.zeros(self.ids.shape, np.float32)
        for n_line, line in enumerate(open(path).read().splitlines()):
            if not line.strip():
                continue
            uid, _, rest = line.partition("\t")
            try:
                u, sids = int(uid), [int(x) for x in rest.split(",") if x.strip()]
            except ValueError:
                raise ValueError("%s line %d: expected uid<TAB>sid[,sid...]" % (path, n_line + 1)) from None
            if u in row_of:
                y[row_of[u]] = np.maximum(y[row_of[u]], np.isin(self.ids[row_of[u]], sids))
        return self.set_reward(y)


class Replay:
    """Off-policy estimates from an exploration log, passed as `replay=` to a Recommender / ShardedRecommender: what the
    logged rewards would have been under the Plackett-Luce policies at `temperatures` (at most 8) behind a fixed head of `fixed` entries
    (default: the log's; a head shorter than the log's is refused, the log has no support there), under THIS model.  It reads the logits
    only, so it goes beside any rule and with k = 0.  Per chunk: the target's plain top-`fixed` through the SlabLists (if any),
    ltg_list_mass on the logged lists of the chunk's users, over item shards four small all-reduces (max of the largest eligible logit,
    sum of the rescaled rest, max of the entries' logits, max of their states), and ltg_replay_rows into the tables of the whole split.
    The walk must be the one the log was made with: the same split, keep_prob and RNG step (keep_prob = 1.0 on both sides is the safe
    choice).  labels / n_groups: the item groups of a LongTailReport (None: one group holding every item).  After run(): table(),
    logp1 (with keep_logp1=True) and estimates().  Over item shards every rank ends with the same tables."""

    MAX_POLICIES = 8                                  # LTG_REPLAY_MAX_POLICIES

    def __init__(self, log, temperatures, fixed=None, clip=100.0, labels=None, n_groups=None, keep_logp1=False):
        if log.reward is None:
            raise ValueError("the log has no rewards: rewards_from / rewards_from_file / set_reward first")
        self.log = log
        self.temperatures = [float(t) for t in np.atleast_1d(np.asarray(temperatures, dtype=np.float64)).tolist()]
        if not 1 <= len(self.temperatures) <= self.MAX_POLICIES:
            raise ValueError("between 1 and %d temperatures, got %d" % (self.MAX_POLICIES, len(self.temperatures)))
        self.inv_temps = [inv_temp_of(t) for t in self.temperatures]
        self.fixed = log.fixed if fixed is None else int(fixed)
        if (fixed is not None and self.fixed != fixed) or not log.fixed <= self.fixed < log.k:
            raise ValueError("fixed must be an integer in [the log's head, k) = [%d, %d), got %r: below the logging head the log has no "
                             "support" % (log.fixed, log.k, fixed))
        self.clip = float(clip)
        if not (self.clip > 0.0 and np.isfinite(self.clip)):
            raise ValueError("clip must be > 0 and finite, got %r" % (clip,))
        if labels is None:
            if n_groups is not None:
                raise ValueError("n_groups needs labels")
            self.labels_host, self.n_groups = None, 1
        else:
            self.n_groups = int(n_groups) if n_groups is not None else int(np.asarray(labels).max()) + 1
            self.labels_host = group_labels(labels, self.n_groups)
        self.keep_logp1 = bool(keep_logp1)
        self.group, self.sharded = None, False
        self.rows = self.w = self.first_bad = self.logp1 = self.state = self.score = self.top = None

    def bind(self, engine, rows, n_users, group=None, sharded=False):
        log, dev, P, G = self.log, engine.device, len(self.inv_temps), self.n_groups
        if log.n != n_users:
            raise ValueError("the log holds %d users, the split %d" % (log.n, n_users))
        log.check_ids(engine.I_global)
        self.group, self.sharded = group, bool(sharded)
        k, F = log.k, self.fixed
        labels = self.labels_host if self.labels_host is not None else np.zeros(engine.I_global, np.uint8)
        self.labels = group_labels(labels, G, engine)
        to = lambda a: torch.from_numpy(a).to(dev)
        self.ids_d, self.logp0_d, self.reward_d = to(log.ids), to(log.logp0), to(log.reward)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.head_s, self.head_i = f32(rows * max(1, F)), torch.empty(rows * max(1, F), dtype=torch.int32, device=dev)
        self.max, self.rest, self.scale = f32(rows), f32(P * rows), f32(rows)
        self.score = f32(n_users, k)
        self.state = torch.zeros(n_users, k, dtype=torch.int32, device=dev)
        self.top = f32(n_users)
        self.rows = torch.zeros(n_users, P, G + 1, 2, dtype=torch.float64, device=dev)
        self.w = torch.zeros(n_users, P, dtype=torch.float64, device=dev)
        self.first_bad = torch.zeros(n_users, P, dtype=torch.int32, device=dev)
        self.logp1 = f32(P, n_users, k) if self.keep_logp1 else None
        self.lp1_chunk = f32(P * rows * k) if self.keep_logp1 else None

    def add(self, lists, acts, tr, n, lo):
        """users lo .. lo + n, whose logits `acts` holds, into the tables"""
        eng, F, k, P = lists.eng, self.fixed, self.log.k, len(self.inv_temps)
        head_i = None
        if F:                                            # the target's head: the plain top-F'
            head_s, head_i = self.head_s[: n * F].view(n, F), self.head_i[: n * F].view(n, F)
            lists.topk(acts, tr, n, F, head_s, head_i)
        ids, sc, st = self.ids_d[lo:lo + n], self.score[lo:lo + n], self.state[lo:lo + n]
        mx, rest = self.max[:n], self.rest[: P * n].view(P, n)
        eng.list_mass(acts, tr, ids, head_i, self.inv_temps, sc, st, mx, rest)
        top = self.top[lo:lo + n]
        top.copy_(mx)
        if lists.parts > 1:                              # the mass of the whole row from the slabs' parts
            dist.all_reduce(top, op=dist.ReduceOp.MAX, group=lists.group)
            for p, it in enumerate(self.inv_temps):
                rest[p].mul_(torch.where(torch.isinf(mx), torch.zeros_like(mx), torch.exp((mx - top) * float(it))))   # (a slab without an eligible item)
            dist.all_reduce(rest, op=dist.ReduceOp.SUM, group=lists.group)
            dist.all_reduce(sc, op=dist.ReduceOp.MAX, group=lists.group)
            dist.all_reduce(st, op=dist.ReduceOp.MAX, group=lists.group)
        lp1 = self.lp1_chunk[: P * n * k].view(P, n, k) if self.keep_logp1 else None
        eng.replay_rows(self.inv_temps, head_i, ids, self.logp0_d[lo:lo + n], self.reward_d[lo:lo + n], sc, st, top, rest, self.labels,
                        self.n_groups, self.clip, self.rows[lo:lo + n], self.w[lo:lo + n], self.first_bad[lo:lo + n], lp1)
        if lp1 is not None:
            self.logp1[:, lo:lo + n].copy_(lp1)

    def table(self):
        """-> dict of host arrays: rows [n_users, n_pol, n_groups + 1, 2] float64 (A, B; slot n_groups = all items), w [n_users, n_pol]
        float64, first_bad [n_users, n_pol] int32, state / score [n_users, k], M [n_users]; logp1 [n_pol, n_users, k] with keep_logp1"""
        out = dict(rows=self.rows.cpu().numpy(), w=self.w.cpu().numpy(), first_bad=self.first_bad.cpu().numpy(),
                   state=self.state.cpu().numpy(), score=self.score.cpu().numpy(), M=self.top.cpu().numpy())
        if self.logp1 is not None:
            out["logp1"] = self.logp1.cpu().numpy()
        return out

    def estimates(self, names=None):
        """-> {temperature: {group: dict(ips, stderr, snips, exposure, logged, logged_per_slot), ..., "ess", "supported", "n_users"}},
        group = names[g] (default the group's index) and "all"; on the host in float64 over the per-row table of the whole split"""
        t = self.table()
        return replay_estimates(t["rows"], t["w"], t["first_bad"], self.log, self.temperatures, self.labels_host, self.n_groups, names)


def replay_estimates(rows, w, first_bad, log, temperatures, labels, n_groups, names=None):
    """the figures of DESIGN 5.22 from the per-row table (Replay.table(), or the numpy reference's): see Replay.estimates"""
    rows, w = np.asarray(rows, np.float64), np.asarray(w, np.float64)
    n, k, G = log.n, log.k, int(n_groups)
    names = [str(g) for g in range(G)] if names is None else list(names)
    real = log.ids >= 0
    lab = (np.zeros(log.ids.shape, np.int64) if labels is None else np.asarray(labels)[np.where(real, log.ids, 0)].astype(np.int64))
    y = log.reward.astype(np.float64)
    div = lambda a, b: float(a / b) if b else float("nan")
    out = {}
    for p, T in enumerate(temperatures):
        res = {}
        for g, name in enumerate(names + ["all"]):
            A, B = rows[:, p, g, 0], rows[:, p, g, 1]
            mean = div(A.sum(), n)
            var = (float((A * A).sum()) / n - mean * mean) * n / (n - 1) if n > 1 else float("nan")
            in_g = real & ((lab == g) | (g == G))
            res[name] = dict(ips=mean, stderr=float(np.sqrt(max(var, 0.0) / n)) if n > 1 else float("nan"), snips=div(A.sum(), B.sum()),
                             exposure=div(B.sum(), n), logged=div(y[in_g].sum(), n), logged_per_slot=div(y[in_g].sum(), int(in_g.sum())))
        W = w[:, p]
        res["ess"] = div(W.sum() ** 2, (W * W).sum())
        res["supported"] = div(int((np.asarray(first_bad)[:, p] == k).sum()), n)
        res["n_users"] = n
        out[T] = res
    return out


POSTERIOR_IMAGE_BYTES = 256 << 20     # the bf16 image of one row block of a Posterior (rows x samples x ld x 2)
POSTERIOR_SAMPLES = (1, 4, 8, 16, 32)


class Posterior:
    """Posterior-aware scores, passed as `posterior=` to a Recommender / ShardedRecommender.  It is not a Rule: it changes what the
    logits ARE, and composes with every rule and attachment.  After the plain forward of a chunk, `samples` draws of z from every user's
    encoder posterior N(mu, exp(logvar)) go through the decoder, and acts.logits becomes mean + beta * std over the draws, acts.lse its
    row log-sum-exp: beta = 0 the posterior mean, beta > 0 UCB (what the model is unsure about ranks higher), beta < 0 LCB, samples = 1
    one Thompson draw (beta must be 0).  The noise is the counter RNG at (engine seed, stream 9, draw, ((global user row) * samples + s)
    * Z + j): the same `draw` gives the same scores whatever the chunk, the row block, the slab or the rank.  A chunk is walked in row
    blocks whose bf16 image stays within POSTERIOR_IMAGE_BYTES; per block ltg_posterior_h2 and ltg_posterior_scores, then one
    ltg_row_lse per chunk.  The [rows * samples, I] logits exist nowhere.  Over item shards mu | logvar are replicated, so every rank
    builds the same image and scores its own slab: the scores are the unsharded run's bit for bit with no new exchange.
    entries=True: after run(), table() holds the posterior mean and std of every served entry (ltg_posterior_entries on the chunk's
    final lists; over shards one float all-reduce of the two tables).  stats=True: one extra plain top-k per chunk on the untouched
    logits, for stats()."""

    def __init__(self, samples=16, beta=1.0, draw=0, entries=True, stats=False):
        self.samples, self.beta, self.draw = int(samples), float(beta), int(draw)
        if self.samples != samples or self.samples not in POSTERIOR_SAMPLES:
            raise ValueError("samples must be one of %s, got %r" % (POSTERIOR_SAMPLES, samples))
        with np.errstate(over="ignore"):
            finite = np.isfinite(self.beta) and np.isfinite(np.float32(self.beta))
        if not finite:
            raise ValueError("beta must be a finite float32, got %r" % (beta,))
        if self.samples == 1 and self.beta != 0.0:
            raise ValueError("samples = 1 is one Thompson draw: it has no std, beta must be 0, got %r" % (beta,))
        if self.draw != draw or not 0 <= self.draw < 2 ** 64:
            raise ValueError("draw is an integer >= 0, got %r" % (draw,))
        self.want_stats = bool(stats)
        self.want_entries = bool(entries) or self.want_stats
        self.k = self.block = self.image = self.mulv = self.mean = self.std = self.plain_i = self.outside = self.real = None

    def bind(self, engine, rows, k, n_users):
        S = self.samples
        per_row = S * engine.posterior_ld() * 2
        self.block = int(max(1, min(rows, POSTERIOR_IMAGE_BYTES // per_row)))
        self.image = engine.posterior_image(self.block, S)
        self.k = int(k)
        dev = engine.device
        if self.want_entries and self.k > 0:
            if self.k > 1024:
                raise ValueError("k must be in [1, 1024] for the entry tables, got %d" % k)
            self.mulv = torch.zeros(n_users, 2 * engine.Z, dtype=torch.float32, device=dev)      # (a whole-split rule reads its lists after the walk)
            self.table_ms = torch.zeros(2, n_users, self.k, dtype=torch.float32, device=dev)
            self.mean, self.std = self.table_ms[0], self.table_ms[1]
            self.ms = torch.empty(2 * rows * self.k, dtype=torch.float32, device=dev)
        if self.want_stats and self.k > 0:
            self.plain_s = torch.empty(rows * self.k, dtype=torch.float32, device=dev)
            self.plain_i = torch.full((n_users, self.k), -1, dtype=torch.int32, device=dev)
            self.outside = torch.zeros(n_users, dtype=torch.int32, device=dev)
            self.real = torch.zeros(n_users, dtype=torch.int32, device=dev)

    def rescore(self, engine, acts, n, lo, lists=None, tr=None):
        """acts.logits [n, I] <- the posterior scores of users lo .. lo + n (this slab's columns), acts.lse <- their row lse"""
        S = self.samples
        if self.plain_i is not None and lists is not None:       # the plain lists, from the untouched logits
            lists.topk(acts, tr, n, self.k, self.plain_s[: n * self.k].view(n, self.k), self.plain_i[lo:lo + n])
        if self.mulv is not None:
            self.mulv[lo:lo + n].copy_(acts.mulv[:n])
        for b0 in range(0, n, self.block):
            nb = min(self.block, n - b0)
            engine.posterior_h2(acts.mulv[b0:], nb, lo + b0, S, self.draw, self.image)
            engine.posterior_scores(self.image, nb, S, self.beta, acts.logits[b0:])
        engine.row_lse(acts.logits, n, acts.lse)

    def entries(self, lists, lo, hi, ids):
        """the tables' rows lo .. hi <- the posterior mean and std of the final lists ids [hi - lo, k]"""
        if self.mean is None:
            return
        eng, S, k, n = lists.eng, self.samples, self.k, hi - lo
        ms = self.ms[: 2 * n * k].view(2, n, k)
        for b0 in range(0, n, self.block):
            nb = min(self.block, n - b0)
            eng.posterior_h2(self.mulv[lo + b0:], nb, lo + b0, S, self.draw, self.image)
            eng.posterior_entries(self.image, S, ids[b0:b0 + nb], ms[0, b0:b0 + nb], ms[1, b0:b0 + nb])
        if lists.parts > 1:                              # an entry's slab holds its values, every other slab 0.0
            dist.all_reduce(ms, op=dist.ReduceOp.SUM, group=lists.group)
        self.mean[lo:hi].copy_(ms[0])
        self.std[lo:hi].copy_(ms[1])
        if self.plain_i is not None:
            for b0 in range(0, n, 1024):                 # ([rows, k, k] comparisons, a block of rows at a time)
                a, p = ids[b0:b0 + 1024], self.plain_i[lo + b0:lo + min(n, b0 + 1024)]
                real = a >= 0
                inside = (a.unsqueeze(2) == p.unsqueeze(1)).any(2)
                self.outside[lo + b0:lo + b0 + a.shape[0]].copy_((real & ~inside).sum(1))
                self.real[lo + b0:lo + b0 + a.shape[0]].copy_(real.sum(1))

    def table(self):
        """-> (mean, std): [n_users, k] float32 host arrays, the posterior mean and std of every served entry (0.0 for padding)"""
        if self.mean is None:
            raise ValueError("this Posterior keeps no entry tables (entries=False, or k = 0)")
        return self.mean.cpu().numpy(), self.std.cpu().numpy()

    def stats(self):
        """-> dict: mean_std (the mean posterior std of the served entries), moved_share (the share of the served entries that are not
        in the same user's plain top-k), entries (the served entries)"""
        if self.plain_i is None:
            raise ValueError("stats() needs Posterior(stats=True) and k >= 1")
        n_e = int(self.real.sum())
        return dict(mean_std=float(self.std.sum(dtype=torch.float64)) / n_e if n_e else float("nan"),
                    moved_share=int(self.outside.sum()) / n_e if n_e else float("nan"), entries=n_e)


class Audience:
    """The item audiences a Recommender / ShardedRecommender gathers when it is passed as `audience=`: for every query item (GLOBAL ids,
    any order, repeats allowed) the k users of the split with the largest score -- `logprob`: logit - lse, the log-probability the user's
    softmax gives the item, comparable across users; `logit`: the raw logit -- among the users whose fold-in row does not hold the item.
    Lists are ltg_topk's with "id" = user row (score descending, ties lower row first, padding -1 / -inf).  Per chunk: ONE
    ltg_item_audience on the chunk's logits (they stay where the forward left them, and no score matrix is written), then ONE
    ltg_topk_merge of [running lists, chunk lists].  The kernel is given the columns in ascending order, so that neighbouring lanes read
    neighbouring columns; table() undoes that.  Over item shards every rank serves the queries whose column it owns, from the full-row lse
    (ShardedRecommender._forward combines it), and table() all-reduces the lists so that every rank ends with the whole table."""

    MAX_K = 256                                      # LTG_AUD_MAX_K

    def __init__(self, items, k=100, score="logprob"):
        self.items = np.ascontiguousarray(np.asarray(items), dtype=np.int32).reshape(-1)
        self.k = int(k)
        if not 1 <= self.k <= self.MAX_K:
            raise ValueError("k must be in [1, %d], got %d" % (self.MAX_K, self.k))
        if score not in ("logprob", "logit"):
            raise ValueError("score must be logprob or logit")
        self.score = score
        self.group, self.sharded = None, False
        self.q_col = self.where = self.pair_s = self.pair_i = self.out_s = self.out_i = self.ws = None

    @property
    def needs_lse(self):
        return self.score == "logprob"

    def bind(self, engine, rows, n_users, group=None, sharded=False):
        """buffers for chunks of up to `rows` users of a split of n_users; sharded: the engine holds one item slab of the ranks of `group`"""
        q, k, dev = self.items, self.k, engine.device
        if q.size and (q.min() < 0 or q.max() >= engine.I_global):
            raise ValueError("query ids outside [0, %d)" % engine.I_global)
        self.group, self.sharded = group, bool(sharded)
        lo = engine.item_lo if self.sharded else 0
        mine = np.nonzero((q >= lo) & (q < lo + engine.I))[0]
        mine = mine[np.argsort(q[mine], kind="stable")]          # this rank's queries, columns ascending
        n = int(mine.size)
        self.where = torch.from_numpy(mine.astype(np.int64)).to(dev)     # list j of this rank = row where[j] of the table
        self.q_col = torch.from_numpy((q[mine] - lo).astype(np.int32)).to(dev)
        self.pair_s = torch.empty(2, n, k, dtype=torch.float32, device=dev)   # [running lists, this chunk's lists]: ltg_topk_merge's parts
        self.pair_i = torch.empty(2, n, k, dtype=torch.int32, device=dev)
        self.out_s = torch.empty(n, k, dtype=torch.float32, device=dev)
        self.out_i = torch.empty(n, k, dtype=torch.int32, device=dev)
        need = neighbors_ws_bytes(lambda r, kk: engine.item_audience_ws_bytes(r, n, kk), n_users, rows, k)
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.reset()

    def reset(self):
        """empty running lists: the start of a run()"""
        self.pair_s[0].fill_(float("-inf"))
        self.pair_i[0].fill_(-1)

    def add(self, engine, acts, tr, n, lo):
        """users lo .. lo + n, whose logits (and lse) `acts` holds, into the running lists"""
        if self.q_col.numel() == 0:
            return
        engine.item_audience(acts, acts.lse if self.needs_lse else None, tr, lo, self.q_col, self.k, self.pair_s[1], self.pair_i[1],
                             ws=self.ws, n_rows=n)
        engine.topk_merge(self.pair_s, self.pair_i, self.k, self.out_s, self.out_i)     # (never in place: the merge scatters)
        self.pair_s[0].copy_(self.out_s)
        self.pair_i[0].copy_(self.out_i)

    def table(self):
        """-> (ids [n_q, k] int32 user rows, scores [n_q, k] float32) host arrays, row r = query items[r].  Over item shards: every rank
        writes its own queries' lists into zeroed buffers, which are all-reduced viewed as int32 -- exactly one rank contributes a row."""
        n_q, k, dev = int(self.items.size), self.k, self.pair_s.device
        ids = torch.zeros(n_q, k, dtype=torch.int32, device=dev)
        scores = torch.zeros(n_q, k, dtype=torch.float32, device=dev)
        if self.where.numel():
            ids[self.where] = self.pair_i[0]
            scores[self.where] = self.pair_s[0]
        if self.sharded:
            dist.all_reduce(ids, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(scores.view(torch.int32), op=dist.ReduceOp.SUM, group=self.group)
        return ids.cpu().numpy(), scores.cpu().numpy()


class Recommender:
    """Top-K recommendations per user (the forward of Evaluator, then ltg_topk instead of the metrics): the same chunks of
    `chunk` users capped by eval_chunk_rows, the same dropout-on forward (Q3) with counter rng_step + lo per chunk, fold-in
    items excluded.  keep_prob = 1.0 gives dropout-free, deterministic recommendations.  Every list comes out of one SlabLists
    (self.lists).  At most one of rule= (MinSlots), diversify=, calibrate=, cap= (ExposureCap), share= (ShareTarget), floor=
    (ExposureFloor), gate= (CriticGate) and explore= (Explore) decides what the lists are: it becomes self.policy, a Rule, and the walk asks it only what Rule's protocol holds;
    without one the lists are the plain top-K.  Per chunk: the forward; audience= (an Audience, audience.table() after run()) gathered
    from the logits; the lists, or with a policy over the whole split only what it gathers; then report= (a LongTailReport, k >= its
    largest cutoff), explain= (an Explain, explain.table() after run()) and critic= (a Critic, critic.table() after run()) read the chunk's
    final lists.  A policy over the whole split
    matches after the last chunk, and a second pass over the chunks (no forward) feeds the report and the explanations.  k = 0 walks the
    chunks for the audience alone: run() returns [n_users, 0] arrays, no list kernel is launched, and nothing that needs lists goes
    with it.  replay= (a Replay, replay.estimates() after run()) re-weights a logged exploration run under other policies from the
    chunk's logits; like the audience it changes no list and works with k = 0.  posterior= (a Posterior) replaces the chunk's logits and
    their lse by posterior scores right after the forward, before anything above reads them; posterior.table() / .stats() after run()."""

    sharded = False                                  # ShardedRecommender: one rank of `group` per item slab

    def __init__(self, engine, ev, k=100, chunk=20000, report=None, rule=None, diversify=None, group=None, audience=None, explain=None,
                 calibrate=None, cap=None, share=None, floor=None, gate=None, critic=None, explore=None, replay=None, posterior=None):
        rules = dict(rule=rule, diversify=diversify, calibrate=calibrate, cap=cap, share=share, floor=floor, gate=gate, explore=explore)
        given = [name for name, r in rules.items() if r is not None]
        if len(given) > 1:
            raise ValueError("%s= cannot be combined with %s=" % (given[-1], "= or ".join(given[:-1])))
        self.policy = rules[given[0]] if given else None
        if int(k) == 0 and (self.policy is not None or report is not None or explain is not None or critic is not None):
            raise ValueError("k = 0 serves no user lists: report=, explain= and every rule need k >= 1")
        self.rule, self.diversify, self.calibrate, self.cap, self.share, self.floor = rule, diversify, calibrate, cap, share, floor
        self.gate, self.critic, self.explore, self.replay, self.posterior = gate, critic, explore, replay, posterior
        self.eng, self.ev, self.k, self.report, self.group, self.audience, self.explain = engine, ev, int(k), report, group, audience, explain
        if report is not None:
            report.bind(engine, ev.n, self.k)
        self.chunk = chunk_rows(engine, ev, chunk)
        longest = self.k
        if self.policy is not None:
            self.policy.bind(engine, self.chunk, self.k, ev.n)
            longest = max(longest, self.policy.longest)
        if explain is not None:
            explain.bind(engine, self.k, ev.n)
            longest = max(longest, explain.top * explain.r)          # (its per-slab lists are [rows * top, r])
        if critic is not None:
            critic.bind(engine, self.chunk, self.k, ev.n)
            longest = max(longest, critic.top)                       # (its per-slab best anchors are [rows * top, 1])
        if replay is not None:
            replay.bind(engine, self.chunk, ev.n, group=group, sharded=self.sharded)
            longest = max(longest, replay.fixed)                     # (the target's head)
        self.lists = SlabLists(engine, self.chunk, longest, group, dist.get_world_size(group) if self.sharded else 1)
        if audience is not None:
            audience.bind(engine, self.chunk, ev.n, group=group, sharded=self.sharded)
        if posterior is not None:
            posterior.bind(engine, self.chunk, self.k, ev.n)
        self.acts = engine.new_acts(self.chunk)
        dev = engine.device
        self.scores = torch.empty(ev.n, self.k, dtype=torch.float32, device=dev)
        self.ids = torch.empty(ev.n, self.k, dtype=torch.int32, device=dev)

    def _forward(self, tr, n, keep_prob, rng_step, lo=0):
        """the logits of the n rows `tr` (users lo .. lo + n) into self.acts; with posterior= the posterior scores in their place"""
        self.eng.forward(tr, self.acts, keep_prob=keep_prob, is_training=0.0, rng_step=rng_step)
        if self.posterior is not None:
            self.posterior.rescore(self.eng, self.acts, n, lo, lists=self.lists, tr=tr)

    def _read(self, tr, te, lo, hi):
        """the report, the explanations and the critic of users lo .. hi, from their final lists"""
        if self.posterior is not None:
            self.posterior.entries(self.lists, lo, hi, self.ids[lo:hi])
        if self.report is not None:
            self.report.add(self.eng, self.ids[lo:hi], te, lo)
        if self.explain is not None:
            self.explain.apply(self.lists, tr, hi - lo, lo, self.ids[lo:hi])
        if self.critic is not None:
            self.critic.apply(self.lists, tr, hi - lo, lo, self.ids[lo:hi])

    def run(self, rng_step=0, keep_prob=0.75):
        """-> (ids [n_users, k] int32 global item ids, scores [n_users, k] float32 logits) as host arrays (over item shards: identical
        on every rank)"""
        eng, ev, k, policy = self.eng, self.ev, self.k, self.policy
        chunks = [(lo, min(ev.n, lo + self.chunk)) for lo in range(0, ev.n, self.chunk)]
        if self.report is not None:
            self.report.item_hits.zero_()
        if policy is not None:
            policy.begin(eng, self.group)
        if self.explain is not None:
            self.explain.pack(eng, group=self.group, share=policy)
        if self.critic is not None:
            self.critic.pack(eng)
        if self.audience is not None:
            self.audience.reset()
        for lo, hi in chunks:
            n = hi - lo
            tr, te = ev.rows(lo, hi)
            self._forward(tr, n, keep_prob, rng_step + lo, lo)
            if self.audience is not None:
                self.audience.add(eng, self.acts, tr, n, lo)
            if self.replay is not None:
                self.replay.add(self.lists, self.acts, tr, n, lo)
            if k == 0:                                   # no user lists: the walk serves the audience alone
                continue
            if policy is not None and policy.whole:      # the lists depend on every chunk: only what the rule gathers now
                policy.gather(self.lists, self.acts, tr, n, lo)
                continue
            if policy is not None:
                policy.apply(self.lists, self.acts, tr, n, k, lo, self.scores[lo:hi], self.ids[lo:hi])
            else:
                self.lists.topk(self.acts, tr, n, k, self.scores[lo:hi], self.ids[lo:hi])
            self._read(tr, te, lo, hi)
        if policy is not None and policy.whole:          # its lists exist only now
            policy.match(eng, k, self.scores, self.ids)
            if self.report is not None or self.explain is not None or self.critic is not None or self.posterior is not None:      # a second pass over the chunks, without a forward
                for lo, hi in chunks:
                    self._read(*ev.rows(lo, hi), lo, hi)
        return self.ids.cpu().numpy(), self.scores.cpu().numpy()


class ShardedRecommender(Recommender):
    """Recommender over item shards: per chunk of users the sharded forward of ShardedEvaluator, and a SlabLists over the ranks of
    `group`, so that every list -- plain, reserved, candidates -- is this slab's list, gathered and merged (ltg_topk_merge).  Every rank
    ends with the identical table, bit-identical to the unsharded Recommender's; the lists a report reads are identical on every rank, so
    the report (item_hits included) needs no exchange, and neither do ltg_topk_quota and ltg_topk_diversify (against the image of the
    whole catalogue, Diversify.begin: one all-reduce per run()).  An Explain sees this slab's part of every history: its per-slab
    explanations are one more gathered and merged list per chunk."""

    sharded = True

    def __init__(self, engine, ev, k=100, group=None, **kw):
        super().__init__(engine, ev, k=k, group=group, **kw)
        self.rowpart = torch.zeros(self.chunk * 5, dtype=torch.float32, device=engine.device)
        self.rowpart_all = None
        if any(x is not None and x.needs_lse for x in (self.audience, self.policy)):      # (replay reads no lse)
            self.rowpart_all = torch.zeros(dist.get_world_size(group) * self.chunk * 5, dtype=torch.float32, device=engine.device)

    def _forward(self, tr, n, keep_prob, rng_step, lo=0):
        """the slab's logits; with an audience or a policy that needs it (needs_lse) also the FULL-row lse in acts.lse: the slabs' row partials
        are all-gathered and combined (ltg_rowstats_combine, as ShardedTrainer.create_phase does) -- one more small collective per chunk.
        With posterior= the slab's posterior scores take the logits' place (mu | logvar are replicated after the h1 all-reduce: nothing new is
        exchanged), and the full-row lse, where it is needed, is combined from one all-gather of the per-slab lse of the scores"""
        sharded_forward(self.eng, tr, n, self.acts, self.rowpart, keep_prob, rng_step, self.group)
        if self.posterior is not None:
            self.posterior.rescore(self.eng, self.acts, n, lo, lists=self.lists, tr=tr)
            if self.rowpart_all is not None:
                R = dist.get_world_size(self.group)
                out = self.rowpart_all[: R * n].view(R, n)
                dist.all_gather(list(out.unbind(0)), self.acts.lse[:n].contiguous(), group=self.group)
                m = out.max(0).values
                self.acts.lse[:n].copy_(m + torch.log(torch.exp(out - m).sum(0)))
            return
        if self.rowpart_all is not None:
            R, m = dist.get_world_size(self.group), n * 5
            out = self.rowpart_all[: R * m]
            dist.all_gather([out[r * m:(r + 1) * m] for r in range(R)], self.rowpart[:m], group=self.group)
            self.eng.rowstats_combine(out, R, n, self.acts.lse)


def group_mask_of(only, n_groups):
    """the group_mask of ltg_topk_groups / ltg_item_neighbors that admits the group indices `only` (None: every group)"""
    if only is None:
        return 0x1FF
    mask = 0
    for g in only:
        if not 0 <= int(g) < int(n_groups):
            raise ValueError("group index %r outside [0, %d)" % (g, n_groups))
        mask |= 1 << min(int(g), 8)
    if mask == 0:
        raise ValueError("`only` admits no group")
    return mask


def neighbors_ws_bytes(ws_bytes, n_q, chunk, k):
    """the workspace for walking n_q queries in chunks of `chunk`: the largest need over the chunk lengths that occur.  ws_bytes(n, k) =
    ltg_item_neighbors_ws_bytes.  It is NOT monotone in n: fewer query blocks get more item segments (the grid is sized to fill the chip),
    so a shorter last chunk can need more than a full one -- 3 392 queries more than 4 096 at 200 000 items."""
    n_q, chunk = int(n_q), max(1, int(chunk))
    sizes = {min(chunk, n_q)} | ({n_q % chunk} if n_q > chunk else set())
    return max([int(ws_bytes(n, k)) for n in sizes if n > 0] + [1])


class ItemNeighbors:
    """The k nearest items of items (ltg_item_neighbors): space `decoder` (rows of W_p1t) or `encoder` (rows of W_q0), metric `cosine` or
    `dot`; a query never returns itself.  labels (uint8 per global item id, longtail.build_groups) + only (group indices) restrict the
    NEIGHBOURS to those groups -- `only=[niche]` over the popular items is the niche shelf of every head item.  The table is packed once
    into the bf16 operand image; the queries are walked in chunks of `chunk`, their rows taken out of the image by index.  The scores
    stay on the chip: the workspace is lists."""

    def __init__(self, engine, k=20, space="decoder", metric="cosine", labels=None, n_groups=None, only=None, chunk=4096):
        self.eng, self.k, self.space, self.metric, self.chunk = engine, int(k), space, metric, max(1, int(chunk))
        dev = engine.device
        self.labels = None
        self.mask = 0x1FF
        if labels is not None:
            self.labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.uint8)).to(dev)
            self.mask = group_mask_of(only, n_groups if n_groups is not None else int(self.labels.max().item()) + 1)
        elif only is not None:
            raise ValueError("`only` needs labels")
        self.image = None

    def pack(self):
        self.image = self.eng.item_pack(self.space, self.metric, out=self.image)
        return self.image

    def _queries(self, query_ids):
        n_glob = self.eng.cfg.n_items_global or self.eng.I
        q = np.arange(n_glob, dtype=np.int32) if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.int32).reshape(-1)
        if q.size and (q.min() < 0 or q.max() >= n_glob):
            raise ValueError("query ids outside [0, %d)" % n_glob)
        return q

    def query_rows(self, gid):
        """the image rows of the global ids gid (a device int32 tensor)"""
        return self.image.index_select(0, gid.long())

    def run(self, query_ids=None):
        """-> (ids [n_q, k] int32 global item ids, scores [n_q, k] float32) as host arrays; query_ids None = every item"""
        eng, k = self.eng, self.k
        dev = eng.device
        q = self._queries(query_ids)
        self.pack()
        ids = torch.empty(len(q), k, dtype=torch.int32, device=dev)
        scores = torch.empty(len(q), k, dtype=torch.float32, device=dev)
        qd = torch.from_numpy(q).to(dev)
        ws = torch.empty(neighbors_ws_bytes(eng.item_neighbors_ws_bytes, len(q), self.chunk, k), dtype=torch.uint8, device=dev)
        for lo in range(0, len(q), self.chunk):
            hi = min(len(q), lo + self.chunk)
            eng.item_neighbors(self.image, self.query_rows(qd[lo:hi]), qd[lo:hi], k, scores[lo:hi], ids[lo:hi], self.labels, self.mask, ws=ws)
        return ids.cpu().numpy(), scores.cpu().numpy()


class ShardedItemNeighbors(ItemNeighbors):
    """ItemNeighbors over item shards.  Every rank packs its slab.  Per chunk of queries every rank copies the image rows of the queries it
    owns into a zeroed [n][608] buffer, which is all-reduced viewed as int32 (exactly one rank contributes a row, so the sum is that row:
    works over gloo and nccl); every rank searches its slab (global ids), and a SlabLists gathers and merges the lists as it does for
    ShardedRecommender.  A pair's score does not depend on the slab that holds the item, so every rank ends with the identical
    table, bit-identical to ItemNeighbors on the whole catalogue."""

    def __init__(self, engine, k=20, space="decoder", metric="cosine", labels=None, n_groups=None, only=None, chunk=4096, group=None):
        super().__init__(engine, k=k, space=space, metric=metric, labels=labels, n_groups=n_groups, only=only, chunk=chunk)
        self.group = group
        self.R = dist.get_world_size(group)

    def run(self, query_ids=None):
        eng, k = self.eng, self.k
        dev = eng.device
        lo_i, hi_i = eng.item_lo, eng.item_hi
        q = self._queries(query_ids)
        self.pack()
        ids = torch.empty(len(q), k, dtype=torch.int32, device=dev)
        scores = torch.empty(len(q), k, dtype=torch.float32, device=dev)
        qd = torch.from_numpy(q).to(dev)
        c = min(self.chunk, max(1, len(q)))
        ws = torch.empty(neighbors_ws_bytes(eng.item_neighbors_ws_bytes, len(q), c, k), dtype=torch.uint8, device=dev)
        qimg = torch.empty(c, 608, dtype=torch.int16, device=dev)
        lists = SlabLists(eng, c, k, self.group, self.R)
        for lo in range(0, len(q), c):
            hi = min(len(q), lo + c)
            n = hi - lo
            g = qd[lo:hi].long()
            qi = qimg[:n]
            qi.zero_()
            own = (g >= lo_i) & (g < hi_i)
            qi[own] = self.image.index_select(0, g[own] - lo_i)
            dist.all_reduce(qi.view(torch.int32), op=dist.ReduceOp.SUM, group=self.group)
            ls, li = lists.local(n, k, scores[lo:hi], ids[lo:hi])
            eng.item_neighbors(self.image, qi, qd[lo:hi], k, ls, li, self.labels, self.mask, ws=ws)
            lists.merge(ls, li, scores[lo:hi], ids[lo:hi])
        return ids.cpu().numpy(), scores.cpu().numpy()


class PairCompanions:
    """The k likeliest partners of items under the DISCRIMINATOR's pair score (ltg_pair_pack / ltg_pair_companions): queries `popular` =
    head items, whose candidates are niche items (the niche shelf of a head item), or `niche`, whose candidates are popular items (the
    anchors of a tail item).  The score is the discriminator's logit without dropout; sigmoid(score) is its probability that a real user
    holds the pair.  Ids are rows of the discriminator's embedding table (item ids).  The candidates' side image is packed once, the
    queries are packed and walked in chunks of `chunk`; the workspace is lists, never scores.  A query never returns itself."""

    def __init__(self, engine, k=20, queries="popular", chunk=4096):
        if queries not in ("popular", "niche"):
            raise ValueError("queries must be 'popular' or 'niche', got %r" % (queries,))
        if not 1 <= int(k) <= LTG_PAIR_MAX_K:
            raise ValueError("k must be in [1, %d]" % LTG_PAIR_MAX_K)
        self.eng, self.k, self.chunk = engine, int(k), max(1, int(chunk))
        self.q_side, self.c_side = queries, "niche" if queries == "popular" else "popular"

    def _ids(self, query_ids, cand_ids):
        n = self.eng.feature_len
        q = np.ascontiguousarray(query_ids, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(cand_ids, dtype=np.int32).reshape(-1)
        for name, a in (("query", q), ("candidate", c)):
            if a.size and (a.min() < 0 or a.max() >= n):
                raise ValueError("%s ids outside [0, %d)" % (name, n))
        if c.size > 1 and np.any(np.diff(c) <= 0):
            raise ValueError("candidate ids must be strictly ascending")
        return q, c

    def _slab(self, c):
        """the candidates this engine searches: all of them"""
        return c

    def _merge(self, n):
        """-> the SlabLists that turns this engine's lists into everybody's (one part: they already are)"""
        return SlabLists(self.eng, n, self.k)

    def run(self, query_ids, cand_ids):
        """-> (ids [n_q, k] int32 item ids, scores [n_q, k] float32 logits) as host arrays; cand_ids strictly ascending"""
        eng, k = self.eng, self.k
        dev = eng.device
        q, c = self._ids(query_ids, cand_ids)
        cd = torch.from_numpy(np.ascontiguousarray(self._slab(c))).to(dev)
        c_img = eng.pair_pack(self.c_side, cd)
        ids = torch.empty(len(q), k, dtype=torch.int32, device=dev)
        scores = torch.empty(len(q), k, dtype=torch.float32, device=dev)
        qd = torch.from_numpy(q).to(dev)
        step = min(self.chunk, max(1, len(q)))
        ws = torch.empty(neighbors_ws_bytes(lambda n, kk: eng.pair_companions_ws_bytes(n, cd.numel(), kk), len(q), step, k), dtype=torch.uint8,
                         device=dev)
        q_img = torch.empty(step, eng.pair_ld(), dtype=torch.float32, device=dev)
        lists = self._merge(step)
        for lo in range(0, len(q), step):
            hi = min(len(q), lo + step)
            qi = eng.pair_pack(self.q_side, qd[lo:hi], out=q_img[: hi - lo])
            ls, li = lists.local(hi - lo, k, scores[lo:hi], ids[lo:hi])
            eng.pair_companions(qi, qd[lo:hi], c_img, cd, k, ls, li, ws=ws)
            lists.merge(ls, li, scores[lo:hi], ids[lo:hi])
        return ids.cpu().numpy(), scores.cpu().numpy()


class ShardedPairCompanions(PairCompanions):
    """PairCompanions over item shards.  The discriminator is replicated, so every rank packs the whole query chunk itself and nothing is
    exchanged for it; each rank searches the candidates whose ids lie in its own item slab, and a SlabLists gathers and merges the lists
    as it does for ShardedItemNeighbors.  A pair's score does not depend on the call that holds the candidate, so every rank ends with
    the table of the unsharded run, bit for bit."""

    def __init__(self, engine, k=20, queries="popular", chunk=4096, group=None):
        super().__init__(engine, k=k, queries=queries, chunk=chunk)
        self.group = group
        self.R = dist.get_world_size(group)

    def _slab(self, c):
        return c[(c >= self.eng.item_lo) & (c < self.eng.item_hi)]

    def _merge(self, n):
        return SlabLists(self.eng, n, self.k, self.group, self.R)


# ---------------------------------------------------------------- what the CLIs share (test.py, recommend.py, longtail.py, similar.py, audience.py, companions.py)
class _Counters:
    """load_checkpoint also restores the trainer's counters; the serving flows have no trainer."""
    update_count = 0.0
    rng_step = 0

    def __init__(self):
        self.np_rng = np.random.RandomState(0)


def open_model(dataset_dir, checkpoint, h_sizes, lr, precision="bf16", device=None):
    """The set-up of a serving CLI: under `python -m torch.distributed.run` (WORLD_SIZE > 1) the process group (LTGAN_DIST_BACKEND,
    default nccl) and this rank's item slab, else the whole catalogue; the device (LOCAL_RANK's, unless given); the generator's engine
    on that slab with the checkpoint restored.  -> (engine, item_lo, item_hi, rank, world, print): print is silent on every rank but 0.
    close_model(world) is its counterpart."""
    import builtins
    from .dataset import count_items
    from .generator import generator_VAECF
    from .sharded import item_slab
    from .train import load_checkpoint
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if device is None:
        device = "cuda:%d" % (int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(os.environ.get("LTGAN_DIST_BACKEND", "nccl"))
    n_items = count_items(dataset_dir)
    lo, hi = item_slab(n_items, rank, world) if world > 1 else (0, n_items)
    gen_net, *_ = generator_VAECF(dataset_dir + "/", h_sizes=tuple(h_sizes), lr=lr, precision=precision, device=device, item_lo=lo, item_hi=hi)
    load_checkpoint(checkpoint, gen_net.engine, _Counters())
    return gen_net.engine, lo, hi, rank, world, builtins.print if rank == 0 else (lambda *a, **k: None)


def close_model(world):
    """every rank has finished: the barrier, then the process group goes"""
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
