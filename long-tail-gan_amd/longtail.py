#!/usr/bin/env python3
"""Long-tail report CLI with test.py's surface:

    cd <dir holding config.ini> && python <repo>/long-tail-gan_amd/longtail.py <dataset_dir> <checkpoint>
        [--split test|validation] [--groups niche|pop:N] [--min-slots NAME:M[,NAME:M...]] [--k 100] [--keep-prob 0.75] [--json report.json]
        [--diversify LAMBDA] [--candidates N] [--div-space decoder|encoder] [--calibrate LAMBDA]
        [--cap C|NAME:C[,NAME:C...]] [--cap-candidates N] [--cap-score logprob|logit] [--share NAME[+NAME...]:S]
        [--floor M|NAME:M[,NAME:M...] --floor-reserve R [--floor-candidates N] [--floor-score logprob|logit]]
        [--gate P [--gate-candidates N]] [--critic [TOP]] [--explore T [--explore-fixed F] [--explore-draw N]]
        [--posterior BETA [--posterior-samples S] [--posterior-draw N]]

restores a checkpoint written by train.py, runs test.py's forward over the users of `<split>_tr.csv` ONCE (chunks of 20 000 users,
dropout on with keep_prob 0.75 by default: Q3, RNG counter 2*10^9 + first row of the chunk), keeps each user's top-K list on the GPU
(ltg_topk, K = max(100, --k)) and reads the whole report off the lists (ltg_topk_metrics): NDCG@100 / Recall@20 / Recall@50 per item
group against `<split>_te.csv`, and the exposure each group gets among the first --k recommendations.

Item groups: `niche` = popular / niche (load_pop_niche_tags' NICHE_TAGS); `pop:N` (2 <= N <= 8) = N popularity buckets of equal size,
items ordered by their row count in train_GAN.csv (descending, equal counts lower id first), pop0 = head.

stdout: test.py's line for the same checkpoint (`NDCG@100<TAB>Recall@20<TAB>Recall@50` over all items), then per group
`name<TAB>items<TAB>users<TAB>NDCG@100<TAB>Recall@20<TAB>Recall@50<TAB>share@k<TAB>coverage@k` (users = those with a held-out item of the
group, over whom the three metrics are averaged, as test.py averages; share = the group's part of the recommended slots; coverage = the
part of the group's items recommended to anyone), then `all<TAB>...` with share 1, the overall coverage and a final gini@k field (Gini
coefficient of the per-item recommendation counts).  --json writes the same numbers.  Under
`python -m torch.distributed.run --nproc-per-node N` the items are sharded as in test.py; rank 0 prints and writes.

--min-slots NAME:M[,NAME:M...] (NAME a group of --groups: popular / niche, or pop0 ..) re-ranks every list on the GPU before the report
reads it, so that at least M of its entries come from group NAME (trainer.MinSlots; ltg_topk_groups + ltg_topk_quota): the table is then
the accuracy / exposure trade-off of that rule.  The lines keep their form, but the first line is the re-ranked lists' NDCG@100 /
Recall@20 / Recall@50 and no longer test.py's.  The rule is stated over the whole list of max(100, --k) entries, so it needs --k >= 100,
and the M may not sum to more than --k.

--diversify LAMBDA (0 <= LAMBDA <= 1; not together with --min-slots) re-ranks every list by greedy maximal marginal relevance before the
report reads it (trainer.Diversify; ltg_topk at --candidates N, then ltg_topk_diversify): the next entry is the candidate with the largest
LAMBDA * relevance - (1 - LAMBDA) * (largest cosine similarity to the entries already chosen), similarity between the rows of the decoder
table (--div-space encoder: W_q0's).  N defaults to min(256, 2 K) and must lie in [K, 256], K = max(100, --k) the length of the lists.
One more line follows the report: `ils@K: <before> -> <after>`, the mean pair similarity inside the plain and the diversified lists.

--calibrate LAMBDA (0 <= LAMBDA <= 1; not together with --min-slots or --diversify) composes every list so that its mix of the groups of
--groups follows the mix of the user's own fold-in history, before the report reads it (trainer.Calibrate; one ltg_topk_groups list per
group, ltg_hist_groups, then ltg_topk_calibrate): the next entry is the best remaining item of some group with the largest
(1 - LAMBDA) * relevance - LAMBDA * miscalibration, miscalibration = the total-variation distance between the history's group shares and
those of the list so far plus that item.  LAMBDA 0 is the plain list.  The last line is then `miscal@K: <before> -> <after>`, the mean
miscalibration of the plain and of the calibrated lists over the users with a non-empty history.

--cap C (C >= 0: every item) or --cap NAME:C[,NAME:C...] (only the items of those groups of --groups; not together with --min-slots,
--diversify or --calibrate) serves lists in which no item appears more than C times, before the report reads them (trainer.ExposureCap;
ltg_topk at --cap-candidates N, then ltg_cap_index / ltg_cap_rounds / ltg_cap_finish once over the whole split): the stable matching in
which a user prefers their N best items in order and an item prefers the users by --cap-score (logprob: logit - lse, the default; logit).
N defaults to min(1024, 4 K) and must lie in [K, 1024], K = max(100, --k).  The last line is then
`cap@K: max exposure <plain> -> <capped>, <items> items at their cap, <users> short lists, <rounds> rounds`.

--share NAME[+NAME...]:S (0 <= S <= 1; NAME a group of --groups; not together with --min-slots, --diversify, --calibrate or --cap) gives
those groups the part S of ALL served slots before the report reads the lists (trainer.ShareTarget; two ltg_topk_groups lists per chunk,
then ltg_topk_share once over the whole split): the promoted slots go to the users for whom they cost the least score, every list stays
in score order, and a target the plain lists already meet changes nothing.  The last line is then
`share@K: <names> <plain share> -> <reached share> (target S), <users> rows changed, price <cost>`, price = the score difference of the
dearest swap made.

--floor M (M >= 0: every item) or --floor NAME:M[,NAME:M...] (only the items of those groups of --groups) with --floor-reserve R (0 <= R
<= K; not together with --min-slots, --diversify, --calibrate, --cap or --share) serves lists in which every floor item appears at least M
times where enough users hold it among their candidates, before the report reads the lists (trainer.ExposureFloor: ltg_topk at
--floor-candidates N, then ltg_floor_index / ltg_floor_rounds / ltg_floor_finish once over the whole split): the stable matching in which
an item proposes to the users that hold it among their N best items, best --floor-score first (logprob: logit - lse, the default; logit),
and a user gives up at most the last R slots of the list, to the proposals it likes best.  The first K - R entries of every list are the
plain ones and every list stays in score order.  N defaults to min(1024, 4 K) and must lie in [K, 1024], K = max(100, --k).  The last
line is then `floor@K: <items> floor items, <items> short of their floor, below the floor <plain> -> <served>, <slots> inserted slots,
<users> rows changed, <rounds> rounds`: short of their floor = the matching holds fewer than M users for the item; below the floor = the
floor items in fewer than M of the plain / the served lists.

--gate P (0 <= P < 1; not together with any rule above) lets a niche entry into a user's list only if the DISCRIMINATOR gives it at least
P beside that user's popular history items, before the report reads the lists (trainer.CriticGate: ltg_topk at --gate-candidates N, then
ltg_pair_critic / ltg_critic_finish / ltg_topk_gate): the critic of a niche entry with features is the mean of the discriminator's pair
logit over the user's popular history items with features, an entry passes iff it has no critic or sigmoid(critic) >= P, and the first K
passing candidates are the list.  N defaults to min(256, 2 K) and must lie in [K, 256], K = max(100, --k).  The table is then what the gate
costs each group; the last line is `gate@K: <entries> scored candidates, <entries> rejected, <users> short lists (min_prob P)`.

--posterior BETA (with any rule, or none) replaces every logit, before anything reads it, by mean + BETA * std over --posterior-samples S
(default 16; one of 1, 4, 8, 16, 32) draws of z from the user's encoder posterior (serving.Posterior: ltg_posterior_h2, ltg_posterior_scores):
BETA = 0 ranks by the posterior mean, BETA > 0 by an upper confidence bound (what the model is unsure about moves up), BETA < 0 by a lower one,
S = 1 with BETA = 0 is one Thompson draw.  --posterior-draw N (default 0) numbers the draw.  After the report come one line per group,
`posterior_std<TAB>name<TAB>entries<TAB>mean std of the served entries of that group`, and the line `posterior@K: beta <B>, samples <S>,
draw <N>, mean entry std <std>, moved share <share of the served entries outside the plain top-K>`: the model's uncertainty about the
tail, next to what the bound costs in NDCG@100 and moves in tail share (compare the report with a run without --posterior).

--explore T (T > 0; not together with any rule above) SAMPLES every list before the report reads it (trainer.Explore: ltg_topk_sample,
ltg_topk_sample_mass, ltg_topk_sample_finish): the first --explore-fixed F entries (default 0, F < K) are the plain top-F, the others are
drawn without replacement in proportion to exp(logit / T) among the remaining items -- the Plackett-Luce policy -- and every entry carries
the log of its conditional probability.  --explore-draw N (default 0) numbers the draw: the same N gives the same lists, another N another
sample.  The table is then what exploration costs in NDCG@100 and gains in tail share / coverage / gini; the last line is
`explore@K: T <T>, fixed <F>, draw <N>, mean list logp <mean log-propensity of a list>, explored share <share>`, explored share = the part
of the sampled slots whose item is not in the plain top-K of the same user.

--critic [TOP] scores the first TOP entries (default min(K, 256)) of whatever lists are served the same way without changing them
(trainer.Critic); the last line is `critic@TOP: <entries> scored entries, <users> users with anchors, mean prob <p>` and --json gets the
same numbers under "critic".
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import sys

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ltgan  # noqa: F401  (alias of this package directory)
    from ltgan import data_processing as dp
else:
    from . import data_processing as dp

RNG_STEP = 2 * 10 ** 9        # test.py's counter: with the defaults the forward is the one test.py scores
K_NDCG, K_R1, K_R2 = 100, 20, 50


def parse_groups(spec):
    """'niche' -> ('niche', 2); 'pop:N' -> ('pop', N), 2 <= N <= 8; anything else raises ValueError"""
    if spec == "niche":
        return "niche", 2
    if spec.startswith("pop:"):
        try:
            n = int(spec[4:])
        except ValueError:
            n = 0
        if 2 <= n <= 8:
            return "pop", n
    raise ValueError("--groups must be niche or pop:N with 2 <= N <= 8, got %r" % (spec,))


def group_names(kind, n):
    """the names build_groups returns for parse_groups' (kind, n)"""
    return ["popular", "niche"] if kind == "niche" else ["pop%d" % g for g in range(n)]


def parse_min_slots(spec, names, k):
    """'NAME:M[,NAME:M...]' -> one minimum per group of `names` (0 where none is given); an unknown name, a name twice, M < 0 or a sum
    above k raises ValueError"""
    slots = [0] * len(names)
    seen = set()
    for part in spec.split(","):
        name, sep, m = part.strip().rpartition(":")
        try:
            m = int(m) if sep else -1
        except ValueError:
            m = -1
        if not sep or m < 0:
            raise ValueError("--min-slots takes NAME:M[,NAME:M...] with M >= 0, got %r" % (part,))
        if name not in names:
            raise ValueError("--min-slots: unknown group %r (the groups are %s)" % (name, ", ".join(names)))
        if name in seen:
            raise ValueError("--min-slots names group %r twice" % (name,))
        seen.add(name)
        slots[names.index(name)] = m
    if sum(slots) > k:
        raise ValueError("--min-slots asks for %d slots, a list has %d" % (sum(slots), k))
    return slots


POSTERIOR_SAMPLES = (1, 4, 8, 16, 32)     # serving.POSTERIOR_SAMPLES (the parsers import no torch)
RULE_OPTIONS = ("min_slots", "diversify", "calibrate", "cap", "share", "floor", "gate", "explore")     # at most one of them; a refusal names the later first


def add_rule_args(ap):
    """the options of the serve-time rules besides --min-slots (trainer.Diversify, Calibrate, ExposureCap, ShareTarget, ExposureFloor,
    CriticGate, Explore) and of the critic (trainer.Critic), shared with recommend.py"""
    ap.add_argument("--diversify", type=float, default=None, metavar="LAMBDA")
    ap.add_argument("--candidates", type=int, default=None, metavar="N")
    ap.add_argument("--div-space", choices=("decoder", "encoder"), default="decoder")
    ap.add_argument("--calibrate", type=float, default=None, metavar="LAMBDA")
    ap.add_argument("--cap", default=None, metavar="C|NAME:C[,NAME:C...]")
    ap.add_argument("--cap-candidates", type=int, default=None, metavar="N")
    ap.add_argument("--cap-score", choices=("logprob", "logit"), default=None)
    ap.add_argument("--share", default=None, metavar="NAME[+NAME...]:S")
    ap.add_argument("--floor", default=None, metavar="M|NAME:M[,NAME:M...]")
    ap.add_argument("--floor-reserve", type=int, default=None, metavar="R")
    ap.add_argument("--floor-candidates", type=int, default=None, metavar="N")
    ap.add_argument("--floor-score", choices=("logprob", "logit"), default=None)
    ap.add_argument("--gate", type=float, default=None, metavar="P")
    ap.add_argument("--gate-candidates", type=int, default=None, metavar="N")
    ap.add_argument("--explore", type=float, default=None, metavar="T")
    ap.add_argument("--explore-fixed", type=int, default=None, metavar="F")
    ap.add_argument("--explore-draw", type=int, default=None, metavar="N")
    ap.add_argument("--critic", type=int, nargs="?", const=0, default=None, metavar="TOP")      # (0: the default, min(k, 256))
    ap.add_argument("--posterior", type=float, default=None, metavar="BETA")
    ap.add_argument("--posterior-samples", type=int, default=None, metavar="S")
    ap.add_argument("--posterior-draw", type=int, default=None, metavar="N")


def parse_item_values(opt, v, spec, names):
    """the per-item value of option `opt`, written with the letter `v` in messages: 'V' -> V; 'NAME:V[,NAME:V...]' -> {group index: V};
    an unknown name, a name twice or V < 0 raises ValueError"""
    try:
        n = int(spec)
    except ValueError:
        n = None
    if n is not None:
        if n < 0:
            raise ValueError("%s takes %s >= 0, got %r" % (opt, v, spec))
        return n
    values = {}
    for part in spec.split(","):
        name, sep, m = part.strip().rpartition(":")
        try:
            m = int(m) if sep else -1
        except ValueError:
            m = -1
        if not sep or m < 0:
            raise ValueError("%s takes %s or NAME:%s[,NAME:%s...] with %s >= 0, got %r" % (opt, v, v, v, v, part))
        if name not in names:
            raise ValueError("%s: unknown group %r (the groups are %s)" % (opt, name, ", ".join(names)))
        if names.index(name) in values:
            raise ValueError("%s names group %r twice" % (opt, name))
        values[names.index(name)] = m
    return values


parse_cap = functools.partial(parse_item_values, "--cap", "C")
parse_floor = functools.partial(parse_item_values, "--floor", "M")


def parse_share(spec, names):
    """'NAME[+NAME...]:S' -> (sorted group indices, S); an unknown name, a name twice, no name or S outside [0, 1] raises ValueError"""
    head, sep, val = spec.strip().rpartition(":")
    try:
        share = float(val) if sep else -1.0
    except ValueError:
        share = -1.0
    if not sep or not head or not 0.0 <= share <= 1.0:
        raise ValueError("--share takes NAME[+NAME...]:S with 0 <= S <= 1, got %r" % (spec,))
    groups = []
    for name in (x.strip() for x in head.split("+")):
        if name not in names:
            raise ValueError("--share: unknown group %r (the groups are %s)" % (name, ", ".join(names)))
        if names.index(name) in groups:
            raise ValueError("--share names group %r twice" % (name,))
        groups.append(names.index(name))
    return sorted(groups), share


def check_rule_args(ap, a, k):
    """refuses (ap.error) two rules together, an option without the rule it belongs to, and what the rule's class would refuse for lists
    of k entries; leaves the parsed --cap / --share / --floor in a.caps / a.shares / a.floors (None without the option)"""
    given = ["--" + o.replace("_", "-") for o in RULE_OPTIONS if getattr(a, o) is not None]
    if len(given) > 1:
        ap.error("%s cannot be combined with %s" % (given[1], given[0]))
    names = group_names(a.group_kind, a.n_groups)
    a.caps = a.shares = a.floors = None

    def parsed(parse, spec):
        try:
            return parse(spec, names)
        except ValueError as e:
            ap.error(str(e))

    if a.diversify is None:
        if a.candidates is not None:
            ap.error("--candidates needs --diversify")
    else:
        if not 0.0 <= a.diversify <= 1.0:
            ap.error("--diversify takes LAMBDA in [0, 1]")
        if k > 256:
            ap.error("--diversify re-ranks at most 256 candidates: lists of %d entries are too long" % k)
        if a.candidates is not None and not k <= a.candidates <= 256:
            ap.error("--candidates must be in [k, 256] = [%d, 256], got %d" % (k, a.candidates))
    if a.calibrate is not None and not 0.0 <= a.calibrate <= 1.0:
        ap.error("--calibrate takes LAMBDA in [0, 1]")
    if a.cap is None:
        if a.cap_candidates is not None or a.cap_score is not None:
            ap.error("--cap-candidates and --cap-score need --cap")
    else:
        a.caps = parsed(parse_cap, a.cap)
        if a.cap_candidates is not None and not k <= a.cap_candidates <= 1024:
            ap.error("--cap-candidates must be in [k, 1024] = [%d, 1024], got %d" % (k, a.cap_candidates))
    if a.share is not None:
        a.shares = parsed(parse_share, a.share)
    if a.floor is None:
        if a.floor_reserve is not None or a.floor_candidates is not None or a.floor_score is not None:
            ap.error("--floor-reserve, --floor-candidates and --floor-score need --floor")
    else:
        if a.floor_reserve is None:
            ap.error("--floor needs --floor-reserve R")
        if not 0 <= a.floor_reserve <= k:
            ap.error("--floor-reserve must be in [0, k] = [0, %d], got %d" % (k, a.floor_reserve))
        a.floors = parsed(parse_floor, a.floor)
        if a.floor_candidates is not None and not k <= a.floor_candidates <= 1024:
            ap.error("--floor-candidates must be in [k, 1024] = [%d, 1024], got %d" % (k, a.floor_candidates))
    if a.gate is None:
        if a.gate_candidates is not None:
            ap.error("--gate-candidates needs --gate")
    else:
        if not 0.0 <= a.gate < 1.0:
            ap.error("--gate takes P in [0, 1)")
        if k > 256:
            ap.error("--gate walks at most 256 candidates: lists of %d entries are too long" % k)
        if a.gate_candidates is not None and not k <= a.gate_candidates <= 256:
            ap.error("--gate-candidates must be in [k, 256] = [%d, 256], got %d" % (k, a.gate_candidates))
    if a.explore is None:
        if a.explore_fixed is not None or a.explore_draw is not None:
            ap.error("--explore-fixed and --explore-draw need --explore")
    else:
        if not (a.explore > 0.0 and np.isfinite(a.explore) and np.isfinite(np.float32(1.0 / a.explore))):
            ap.error("--explore takes a temperature T > 0, finite")
        if a.explore_fixed is not None and not 0 <= a.explore_fixed < k:
            ap.error("--explore-fixed must be in [0, k) = [0, %d), got %d" % (k, a.explore_fixed))
        if a.explore_draw is not None and a.explore_draw < 0:
            ap.error("--explore-draw takes N >= 0")
    if a.critic is not None and a.critic != 0 and not 1 <= a.critic <= min(k, 256):
        ap.error("--critic takes TOP in [1, min(k, 256)] = [1, %d]" % min(k, 256))
    if a.posterior is None:
        if a.posterior_samples is not None or a.posterior_draw is not None:
            ap.error("--posterior-samples and --posterior-draw need --posterior")
    else:
        with np.errstate(over="ignore"):
            finite = np.isfinite(a.posterior) and np.isfinite(np.float32(a.posterior))
        if not finite:
            ap.error("--posterior takes a finite BETA")
        if a.posterior_samples is not None and a.posterior_samples not in POSTERIOR_SAMPLES:
            ap.error("--posterior-samples must be one of %s, got %d" % (", ".join(str(x) for x in POSTERIOR_SAMPLES), a.posterior_samples))
        if (a.posterior_samples or 16) == 1 and a.posterior != 0.0:
            ap.error("--posterior-samples 1 is one Thompson draw: it has no std, BETA must be 0")
        if a.posterior_draw is not None and a.posterior_draw < 0:
            ap.error("--posterior-draw takes N >= 0")


def build_rules(args, dataset_dir, n_items, groups=None):
    """the serve-time rule of the parsed options -> (its keyword for a Recommender: {} or one entry, the stdout lines it adds after
    run(): callables (ids, tr, k) -> str).  groups: (labels, names) of --groups where the caller has built them; else they are built
    here, and only for a rule that refers to them"""
    from ltgan.serving import Calibrate, CriticGate, Diversify, Explore, ExposureCap, ExposureFloor, MinSlots, ShareTarget

    def grouped():
        labels, names = groups or build_groups(dataset_dir, args.group_kind, args.n_groups, n_items)
        return labels, names, len(names)

    def per_item(values):                                # an int for every item, or {group index: value} with the labels it refers to
        if not isinstance(values, dict):
            return values
        labels, _, n = grouped()
        return labels, n, values

    if getattr(args, "slots", None):
        labels, _, n = grouped()
        return dict(rule=MinSlots(labels, n, args.slots)), []
    if getattr(args, "diversify", None) is not None:
        div = Diversify(args.diversify, candidates=args.candidates, space=args.div_space)
        return dict(diversify=div), [lambda ids, tr, k: ils_line(div.stats(), ids, k)]
    if getattr(args, "calibrate", None) is not None:
        labels, _, n = grouped()
        cal = Calibrate(labels, n, args.calibrate)
        return dict(calibrate=cal), [lambda ids, tr, k: miscal_line(cal.stats(), tr, k)]
    if getattr(args, "caps", None) is not None:
        cap = ExposureCap(per_item(args.caps), candidates=args.cap_candidates, score=args.cap_score or "logprob")
        return dict(cap=cap), [lambda ids, tr, k: cap_line(cap.plain_ids(k), ids, cap.cap_vector(), cap.stats(), k)]
    if getattr(args, "shares", None) is not None:
        labels, names, n = grouped()
        share = ShareTarget(labels, n, args.shares[0], args.shares[1])
        return dict(share=share), [lambda ids, tr, k: share_line([names[g] for g in share.promote], share.stats(), k)]
    if getattr(args, "floors", None) is not None:
        floor = ExposureFloor(per_item(args.floors), args.floor_reserve, candidates=args.floor_candidates, score=args.floor_score or "logprob")
        return dict(floor=floor), [lambda ids, tr, k: floor_line(floor.plain_ids(k), ids, floor.need_vector(), floor.stats(), k)]
    if getattr(args, "gate", None) is not None:
        gate = CriticGate(*critic_sides(dataset_dir, n_items), args.gate, candidates=args.gate_candidates)
        return dict(gate=gate), [lambda ids, tr, k: gate_line(gate.stats(), gate.min_prob, k)]
    if getattr(args, "explore", None) is not None:
        exp = Explore(args.explore, fixed=args.explore_fixed or 0, draw=args.explore_draw or 0)
        return dict(explore=exp), [lambda ids, tr, k: explore_line(exp, k)]
    return {}, []


def critic_sides(dataset_dir, n_items):
    """-> (niche ids, ids with features): what a Critic / CriticGate takes, read as companions.py reads them"""
    d = dataset_dir
    show2id, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(d, "item2id.txt"), os.path.join(d, "item_list.txt"),
                                                     os.path.join(d, "niche_items.txt"), n_items)
    return niche, dp.load_valid_item_ids(os.path.join(d, "item_list.txt"), show2id)


def build_critic(args, dataset_dir, n_items):
    """the Critic of --critic [TOP], or None"""
    if getattr(args, "critic", None) is None:
        return None
    from ltgan.serving import Critic
    return Critic(*critic_sides(dataset_dir, n_items), top=args.critic or None)


def build_posterior(args):
    """the Posterior of --posterior BETA, or None; it composes with every rule (it is not one)"""
    if getattr(args, "posterior", None) is None:
        return None
    from ltgan.serving import Posterior
    return Posterior(samples=args.posterior_samples or 16, beta=args.posterior, draw=args.posterior_draw or 0, entries=True, stats=True)


def posterior_line(post, k):
    """the line --posterior adds: the mean posterior std of the served entries and the share of them outside the plain top-k"""
    st = post.stats()
    return "posterior@%d: beta %.6g, samples %d, draw %d, mean entry std %.6f, moved share %.6f" % (
        k, post.beta, post.samples, post.draw, st["mean_std"], st["moved_share"])


def posterior_group_lines(post, ids, labels, names):
    """one line per item group: the mean posterior std of the served entries of that group (host arithmetic on Posterior.table())"""
    _, std = post.table()
    ids, labels = np.asarray(ids), np.asarray(labels)
    real = ids >= 0
    lab = np.where(real, labels[np.where(real, ids, 0)], 255)
    out = []
    for g, name in enumerate(names):
        sel = lab == g
        n = int(sel.sum())
        out.append("posterior_std\t%s\t%d\t%s" % (name, n, "%.6f" % float(std[sel].astype(np.float64).mean()) if n else "nan"))
    return out


def gate_line(stats, min_prob, k):
    """the line --gate adds: the scored candidates, those rejected before their list was full and the short lists (CriticGate.stats()
    [n_users, 3])"""
    st = np.asarray(stats).astype(np.int64).reshape(-1, 3)
    return "gate@%d: %d scored candidates, %d rejected, %d short lists (min_prob %.6g)" % (
        k, int(st[:, 0].sum()), int(st[:, 1].sum()), int((st[:, 2] < k).sum()), min_prob)


def explore_line(exp, k):
    """the line --explore adds: the mean log-propensity of a list and the explored share (Explore.stats())"""
    st = exp.stats()
    return "explore@%d: T %.6g, fixed %d, draw %d, mean list logp %.6f, explored share %.6f" % (
        k, exp.temperature, exp.fixed, exp.draw, st["mean_logp"], st["explored_share"])


def critic_line(summary, top):
    """the line --critic adds (Critic.summary())"""
    return "critic@%d: %d scored entries, %d users with anchors, mean prob %.6f" % (
        top, summary["scored"], summary["users_with_anchors"], summary["mean_prob"])


def cap_line(plain_ids, ids, cap_vec, stats, k):
    """the line --cap adds: the largest number of lists one item appears in, plain top-k -> capped (plain_ids / ids [n_users, k],
    padding -1; cap_vec: the cap per item), the items that sit exactly at their cap, the short lists and the rounds (ExposureCap.stats())"""
    n_items = len(cap_vec)
    before = np.bincount(plain_ids[plain_ids >= 0], minlength=n_items)
    after = np.bincount(ids[ids >= 0], minlength=n_items)
    at_cap = int(((after == np.asarray(cap_vec)) & (np.asarray(cap_vec) > 0)).sum())
    return "cap@%d: max exposure %d -> %d, %d items at their cap, %d short lists, %d rounds" % (
        k, int(before.max()) if n_items else 0, int(after.max()) if n_items else 0, at_cap, stats["short"], stats["rounds"])


def floor_line(plain_ids, ids, need_vec, stats, k):
    """the line --floor adds: the floor items, those the matching leaves short of their floor, the floor items in fewer lists than their
    floor, plain top-k -> served (plain_ids / ids [n_users, k], padding -1; need_vec: the floor per item), the inserted slots, the rows
    changed and the rounds (ExposureFloor.stats())"""
    need = np.asarray(need_vec)
    before = np.bincount(plain_ids[plain_ids >= 0], minlength=len(need))
    after = np.bincount(ids[ids >= 0], minlength=len(need))
    return ("floor@%d: %d floor items, %d short of their floor, below the floor %d -> %d, %d inserted slots, %d rows changed, %d rounds" % (
        k, stats["floor_items"], stats["short_items"], int(((need > 0) & (before < need)).sum()), int(((need > 0) & (after < need)).sum()),
        stats["inserted"], stats["rows_changed"], stats["rounds"]))


def share_line(names, stats, k):
    """the line --share adds: the promoted groups' part of the served slots, plain -> reached, the target, the rows whose list changed and
    the price of the dearest swap (ShareTarget.stats())"""
    return "share@%d: %s %.6f -> %.6f (target %.6f), %d rows changed, price %.6g" % (
        k, "+".join(names), stats["plain_share"], stats["share"], stats["target"], stats["rows_changed"], stats["price"])


def miscal_line(stats, tr, k):
    """the line --calibrate adds: the mean miscalibration of the plain top-k lists -> of the calibrated ones (Calibrate.stats()
    [n_users, 2]), averaged in float64 over the users with a non-empty fold-in history (tr: the fold-in CSR, rows aligned with stats)"""
    st = np.asarray(stats).astype(np.float64)
    ok = np.diff(tr.tocsr().indptr) > 0
    b, a = (float(st[ok, 0].mean()), float(st[ok, 1].mean())) if ok.any() else (float("nan"), float("nan"))
    return "miscal@%d: %.6f -> %.6f" % (k, b, a)


def ils_line(stats, ids, k):
    """the line --diversify adds: the mean pair similarity of the plain top-k lists -> of the diversified ones (Diversify.stats()
    [n_users, 2]), averaged in float64 over the users whose list holds at least two entries (ids [n_users, k], padding -1)"""
    st = np.asarray(stats).astype(np.float64)
    ok = (np.asarray(ids) >= 0).sum(axis=1) >= 2
    b, a = (float(st[ok, 0].mean()), float(st[ok, 1].mean())) if ok.any() else (float("nan"), float("nan"))
    return "ils@%d: %.6f -> %.6f" % (k, b, a)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="longtail.py", description="per-group accuracy and exposure of a Long-Tail-GAN checkpoint")
    ap.add_argument("dataset_dir")
    ap.add_argument("checkpoint")
    ap.add_argument("--split", choices=("test", "validation"), default="test")
    ap.add_argument("--groups", default="niche")
    ap.add_argument("--min-slots", default=None)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--keep-prob", type=float, default=0.75)
    ap.add_argument("--json", default=None)
    add_rule_args(ap)
    a = ap.parse_args(argv)
    try:
        a.group_kind, a.n_groups = parse_groups(a.groups)
    except ValueError as e:
        ap.error(str(e))
    if not 1 <= a.k <= 1024:
        ap.error("--k must be in [1, 1024]")
    if not 0.0 < a.keep_prob <= 1.0:
        ap.error("--keep-prob must be in (0, 1]")
    a.slots = None
    if a.min_slots is not None:
        if a.k < 100:
            ap.error("--min-slots needs --k >= 100: the rule is stated over the whole list of max(100, --k) entries")
        try:
            a.slots = parse_min_slots(a.min_slots, group_names(a.group_kind, a.n_groups), a.k)
        except ValueError as e:
            ap.error(str(e))
    check_rule_args(ap, a, max(K_NDCG, K_R1, K_R2, a.k))           # (the length of the lists: LongTailReport.k)
    return a


def niche_groups(niche, n_items):
    """-> (labels uint8 [n_items], names): 0 = popular, 1 = niche (niche: the NICHE_TAGS ids)"""
    labels = np.zeros(n_items, np.uint8)
    labels[np.fromiter((int(x) for x in niche), np.int64, len(niche))] = 1
    return labels, group_names("niche", 2)


def pop_groups_from_counts(counts, n):
    """items ordered by count descending, equal counts lower id first; the item at position p gets group p * n // n_items"""
    counts = np.asarray(counts, np.int64)
    n_items = counts.size
    order = np.lexsort((np.arange(n_items), -counts))
    labels = np.empty(n_items, np.uint8)
    labels[order] = (np.arange(n_items, dtype=np.int64) * n // n_items).astype(np.uint8)
    return labels, group_names("pop", n)


def pop_groups(train_csv, n_items, n):
    """popularity buckets from the rows of train_GAN.csv (one row per interaction)"""
    import pandas as pd
    sid = pd.read_csv(train_csv)["sid"].to_numpy()
    return pop_groups_from_counts(np.bincount(sid, minlength=n_items)[:n_items], n)


def build_groups(dataset_dir, kind, n, n_items):
    if kind == "niche":
        _, _, niche, _, _ = dp.load_pop_niche_tags(os.path.join(dataset_dir, "item2id.txt"), os.path.join(dataset_dir, "item_list.txt"),
                                                   os.path.join(dataset_dir, "niche_items.txt"), n_items)
        return niche_groups(niche, n_items)
    return pop_groups(os.path.join(dataset_dir, "train_GAN.csv"), n_items, n)


def gini(hits):
    """sum_i (2i - n - 1) h_(i) / (n sum h), h ascending, i = 1..n; nan when nothing was recommended"""
    h = np.sort(np.asarray(hits, np.float64))
    n, tot = h.size, h.sum()
    if n == 0 or tot == 0:
        return float("nan")
    return float(((2.0 * np.arange(1, n + 1) - n - 1.0) * h).sum() / (n * tot))


def aggregate(out, item_hits, labels, names, k):
    """out [n_users, n_groups + 1, 4] and item_hits [n_items] as ltg_topk_metrics fills them -> the report (a dict).  The means are
    Evaluator.run's: float64, over the users whose slot is valid."""
    o = np.asarray(out).astype(np.float64)
    hits = np.asarray(item_hits).astype(np.int64)
    labels = np.asarray(labels)
    total = int(hits.sum())

    def means(s):
        ok = o[:, s, 3] > 0
        n = int(ok.sum())
        m = [float(o[ok, s, c].mean()) if n else float("nan") for c in range(3)]
        return dict(users=n, ndcg=m[0], recall20=m[1], recall50=m[2])

    groups = []
    for g, name in enumerate(names):
        sel = labels == g
        n_it = int(sel.sum())
        row = dict(name=name, items=n_it, **means(g))
        row["share"] = float(hits[sel].sum()) / total if total else float("nan")
        row["coverage"] = float((hits[sel] > 0).sum()) / n_it if n_it else float("nan")
        groups.append(row)
    allrow = dict(name="all", items=int(hits.size), **means(len(names)))
    allrow["share"] = 1.0 if total else float("nan")
    allrow["coverage"] = float((hits > 0).sum()) / hits.size if hits.size else float("nan")
    allrow["gini"] = gini(hits)
    return dict(k=int(k), groups=groups, all=allrow)


def _row(r):
    return "%s\t%d\t%d\t%.9f\t%.9f\t%.9f\t%.6f\t%.6f" % (r["name"], r["items"], r["users"], r["ndcg"], r["recall20"], r["recall50"],
                                                          r["share"], r["coverage"])


def report_lines(rep):
    """stdout of the CLI: test.py's line, one line per group, the `all` line with gini@k at the end"""
    a = rep["all"]
    lines = [str(a["ndcg"]) + "\t" + str(a["recall20"]) + "\t" + str(a["recall50"])]
    lines += [_row(g) for g in rep["groups"]]
    lines.append(_row(a) + "\t%.6f" % a["gini"])
    return lines


def write_json(rep, path):
    with open(path, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")


def longtail(args, h0_size, h1_size, h2_size, h3_size, LEARNING_RATE, precision="bf16", batch_size_test=20000, **_):
    from ltgan.dataset import EvalData
    from ltgan.serving import LongTailReport, Recommender, ShardedRecommender, close_model, open_model
    d = args.dataset_dir
    eng, lo, hi, rank, world, print = open_model(d, args.checkpoint, (h0_size, h1_size, h2_size, h3_size), LEARNING_RATE, precision)  # noqa: A001
    n_items = eng.I_global
    tr, te, _ = dp.load_tr_te_data(os.path.join(d, "%s_tr.csv" % args.split), os.path.join(d, "%s_te.csv" % args.split), n_items)
    labels, names = build_groups(d, args.group_kind, args.n_groups, n_items)
    report = LongTailReport(labels, len(names), k_ndcg=K_NDCG, k_r1=K_R1, k_r2=K_R2, k_exp=args.k)
    rule, rule_lines = build_rules(args, d, n_items, (labels, names))
    critic = build_critic(args, d, n_items)
    if critic is not None:
        rule = dict(rule, critic=critic)
    post = build_posterior(args)
    if post is not None:
        rule = dict(rule, posterior=post)
    if world > 1:
        rec = ShardedRecommender(eng, EvalData(tr, te, eng.device, item_lo=lo, item_hi=hi), k=report.k, chunk=batch_size_test, report=report, **rule)
    else:
        rec = Recommender(eng, EvalData(tr, te, eng.device), k=report.k, chunk=batch_size_test, report=report, **rule)
    ids, _ = rec.run(rng_step=RNG_STEP, keep_prob=args.keep_prob)
    rep = aggregate(*report.table(), labels, names, args.k)
    rep.update(split=args.split, groups_spec=args.groups)
    for line in report_lines(rep):
        print(line)
    for line in rule_lines:
        print(line(ids, tr, report.k))
    if critic is not None:
        rep["critic"] = dict(critic.summary(), top=critic.top)
        print(critic_line(rep["critic"], critic.top))
    if post is not None:
        rep["posterior"] = dict(post.stats(), beta=post.beta, samples=post.samples, draw=post.draw)
        for line in posterior_group_lines(post, ids, labels, names):
            print(line)
        print(posterior_line(post, report.k))
    if args.json and rank == 0:
        write_json(rep, args.json)
    close_model(world)
    return rep


if __name__ == "__main__":
    a = parse_args(sys.argv[1:])
    from ltgan.train import read_config
    longtail(a, **read_config())
