#!/usr/bin/env python3
"""Replay CLI: off-policy estimates for other exploration policies from a logged exploration run.

    cd <dir holding config.ini> && python <repo>/long-tail-gan_amd/replay.py <dataset_dir> <checkpoint>
        --log recs.npz|props.tsv --feedback heldout|FILE --temperature T[,T...] [--fixed F] [--logged-fixed F0] [--clip 100]
        [--groups niche|pop:N] [--split test|validation] [--keep-prob 1.0] [--k K] [--json out.json] [--propensities-out FILE]

`recommend.py --explore T0` serves sampled lists and logs, per entry, the log of the probability with which it was shown (--npz, or
props.tsv).  Given that log and the feedback on it, this answers what the reward would have been under OTHER Plackett-Luce policies: at
other temperatures (up to 8, comma-separated), with a longer fixed head (--fixed F >= --logged-fixed F0, the head the log was made with;
below F0 the log has no support), or under another checkpoint.  Per chunk of users the checkpoint's forward runs as recommend.py runs it,
ltg_list_mass reads each chunk's logits once for all temperatures, and ltg_replay_rows forms the prefix importance weights w_j =
exp(min(sum_{m <= j} (logp1_m - logp0_m), log(clip))), zero from the first slot the target could not have shown (trainer.Replay, DESIGN
5.22).

THE FORWARD MUST BE THE ONE THE LOG WAS MADE WITH: the same --split, the same --keep-prob and recommend.py's RNG step.  With dropout on
(keep-prob < 1) the logits depend on the chunking as well, so --keep-prob 1.0 on both sides is the safe choice and the default here (pass
recommend.py --keep-prob 1.0 when logging).  Replaying the logging policy itself under the logging checkpoint must give weights of 1: the
`T <T0>` line then shows ips = the logged mean reward, exposure = the list length and ess = the number of users.

--feedback heldout: reward 1.0 where the shown item is a held-out item of the user (<split>_te.csv); FILE: lines `uid<TAB>sid[,sid...]`,
the entries of that user's list that were clicked.  --log: the npz of recommend.py --explore --npz (uids / ids / logp) or its props.tsv
(then --k pads the lists, default the longest line).

One stdout line per temperature and group of --groups (and `all`):
    replay T <T> <group>: ips <mean reward per user> +- <stderr>, per-slot <reward per shown slot> (logged <..>), exposure <slots>/user,
    ess <effective sample size> of <users>, supported <share of fully supported lists>
--json writes the same figures; --propensities-out writes the target log-probabilities in props.tsv's format, one block per temperature
(`# T <T>` lines between them; an unsupported slot reads -inf).  Under `python -m torch.distributed.run --nproc-per-node N` the items are
sharded as in test.py; rank 0 writes.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ltgan  # noqa: F401  (alias of this package directory)
    from ltgan import data_processing as dp
    from ltgan import longtail as lt
    from ltgan.recommend import RNG_STEP
else:
    from . import data_processing as dp
    from . import longtail as lt
    from .recommend import RNG_STEP

MAX_POLICIES = 8      # LTG_REPLAY_MAX_POLICIES


def parse_temperatures(spec):
    """'T[,T...]' -> floats, each > 0 and finite, at most 8; anything else raises ValueError"""
    try:
        ts = [float(x) for x in spec.split(",")]
    except ValueError:
        raise ValueError("--temperature takes T[,T...], got %r" % (spec,)) from None
    if not 1 <= len(ts) <= MAX_POLICIES:
        raise ValueError("--temperature takes between 1 and %d values" % MAX_POLICIES)
    for t in ts:
        with np.errstate(over="ignore"):
            it = np.float32(1.0 / t) if t > 0.0 and np.isfinite(t) else np.float32(0)
        if not (it > 0 and np.isfinite(it)):             # (as Explore: 1 / T must be a positive finite float32)
            raise ValueError("every temperature must be > 0 and finite, got %r" % (t,))
    return ts


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="replay.py", description="off-policy estimates for other exploration policies from a logged run; the "
                                 "forward must be the one the log was made with: same --split, --keep-prob (1.0 on both sides is the safe "
                                 "choice) and RNG step")
    ap.add_argument("dataset_dir")
    ap.add_argument("checkpoint")
    ap.add_argument("--log", required=True, help="recommend.py's --npz file or its props.tsv")
    ap.add_argument("--feedback", required=True, help="heldout, or a file of lines uid<TAB>sid[,sid...]")
    ap.add_argument("--temperature", required=True, metavar="T[,T...]")
    ap.add_argument("--fixed", type=int, default=None, metavar="F", help="the target's fixed head (default: --logged-fixed)")
    ap.add_argument("--logged-fixed", type=int, default=0, metavar="F0", help="the fixed head the log was made with")
    ap.add_argument("--clip", type=float, default=100.0)
    ap.add_argument("--groups", default="niche")
    ap.add_argument("--split", choices=("test", "validation"), default="test")
    ap.add_argument("--keep-prob", type=float, default=1.0, help="must equal the logging run's; 1.0 on both sides is the safe choice")
    ap.add_argument("--k", type=int, default=None, help="list length of a props.tsv log (default: its longest line)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--propensities-out", default=None)
    a = ap.parse_args(argv)
    try:
        a.temperatures = parse_temperatures(a.temperature)
        a.group_kind, a.n_groups = lt.parse_groups(a.groups)
    except ValueError as e:
        ap.error(str(e))
    if a.k is not None and not 1 <= a.k <= 1024:
        ap.error("--k must be in [1, 1024]")
    if not 0.0 < a.keep_prob <= 1.0:
        ap.error("--keep-prob must be in (0, 1]")
    if not (a.clip > 0.0 and np.isfinite(a.clip)):
        ap.error("--clip must be > 0 and finite")
    if a.logged_fixed < 0:
        ap.error("--logged-fixed must be >= 0")
    if a.fixed is not None and a.fixed < a.logged_fixed:
        ap.error("--fixed must be >= --logged-fixed: below the logging head the log has no support")
    return a


def read_log(path, k=None, fixed=0, n_items=None):
    """the ReplayLog of an npz (recommend.py --npz) or of a props.tsv"""
    from ltgan.serving import ReplayLog
    if path.endswith(".npz"):
        log = ReplayLog.from_npz(path, fixed=fixed, n_items=n_items)
        if k is not None and k != log.k:
            raise ValueError("--k %d, but the lists of %s hold %d entries" % (k, path, log.k))
        return log
    if k is None:
        k = max([line.count(":") for line in open(path).read().splitlines()] + [1])
    return ReplayLog.from_tsv(path, k, fixed=fixed, n_items=n_items)


def replay_lines(est, names):
    """the stdout lines of Replay.estimates(names)"""
    lines = []
    for T, res in est.items():
        for name in list(names) + ["all"]:
            g = res[name]
            lines.append("replay T %g %s: ips %.6f +- %.6f, per-slot %.6f (logged %.6f), exposure %.4f/user, ess %.1f of %d, supported %.4f" % (
                T, name, g["ips"], g["stderr"], g["snips"], g["logged_per_slot"], g["exposure"], res["ess"], res["n_users"], res["supported"]))
    return lines


def write_json(est, args, log, path):
    doc = dict(k=log.k, users=log.n, logged_fixed=log.fixed, fixed=args.fixed if args.fixed is not None else log.fixed, clip=args.clip,
               policies=[dict(temperature=T, **res) for T, res in est.items()])
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def write_target_propensities(logp1, temperatures, ids, uid_start, path):
    """logp1 [n_pol, n_users, k] (Replay.table()["logp1"]): per temperature a `# T <T>` line and then props.tsv's lines,
    `uid<TAB>sid:logp1,...` (%.6g; padding left out; an unsupported slot reads -inf) -> lines written"""
    ids = np.asarray(ids)
    n = 0
    with open(path, "w") as f:
        for p, T in enumerate(temperatures):
            f.write("# T %g\n" % T)
            for u in range(ids.shape[0]):
                keep = ids[u] >= 0
                f.write("%d\t%s\n" % (int(uid_start) + u, ",".join(
                    "%d:%.6g" % (int(i), float(x)) for i, x in zip(ids[u][keep].tolist(), np.asarray(logp1[p][u])[keep].tolist()))))
                n += 1
    return n + len(temperatures)


def replay(args, h0_size, h1_size, h2_size, h3_size, LEARNING_RATE, precision="bf16", batch_size_test=20000, **_):
    from ltgan.dataset import EvalData
    from ltgan.serving import Recommender, Replay, ShardedRecommender, close_model, open_model
    d = args.dataset_dir
    eng, lo, hi, rank, world, print = open_model(d, args.checkpoint, (h0_size, h1_size, h2_size, h3_size), LEARNING_RATE, precision)  # noqa: A001
    n_items = eng.I_global
    tr, te, uid0 = dp.load_tr_te_data(os.path.join(d, "%s_tr.csv" % args.split), os.path.join(d, "%s_te.csv" % args.split), n_items)
    labels, names = lt.build_groups(d, args.group_kind, args.n_groups, n_items)
    log = read_log(args.log, args.k, args.logged_fixed, n_items)
    if log.n != tr.shape[0]:
        raise SystemExit("replay.py: the log holds %d users, the %s split %d" % (log.n, args.split, tr.shape[0]))
    if log.uids is not None and not np.array_equal(log.uids, np.arange(log.n) + int(uid0)):
        raise SystemExit("replay.py: the log's uids are not those of the %s split" % args.split)
    if args.feedback == "heldout":
        log.rewards_from(te)
    else:
        log.rewards_from_file(args.feedback, uid_start=uid0)
    rp = Replay(log, args.temperatures, fixed=args.fixed, clip=args.clip, labels=labels, n_groups=len(names),
                keep_logp1=args.propensities_out is not None)
    if world > 1:
        rec = ShardedRecommender(eng, EvalData(tr, te, eng.device, item_lo=lo, item_hi=hi), k=0, chunk=batch_size_test, replay=rp)
    else:
        rec = Recommender(eng, EvalData(tr, te, eng.device), k=0, chunk=batch_size_test, replay=rp)
    rec.run(rng_step=RNG_STEP, keep_prob=args.keep_prob)
    est = rp.estimates(names)
    if rank == 0:
        if args.json:
            write_json(est, args, log, args.json)
        if args.propensities_out:
            write_target_propensities(rp.table()["logp1"], args.temperatures, log.ids, uid0, args.propensities_out)
    for line in replay_lines(est, names):
        print(line)
    close_model(world)
    return est


if __name__ == "__main__":
    a = parse_args(sys.argv[1:])
    from ltgan.train import read_config
    replay(a, **read_config())
