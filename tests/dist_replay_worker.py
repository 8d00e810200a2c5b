"""Worker of tests/test_gpu_replay.py::test_sharded_recommender_with_replay: `torchrun --nproc-per-node N` on ONE GPU (gloo backend, every
rank on cuda:0).  ShardedRecommender with replay= (sharded forward; the target's plain top-F' per slab, gathered and merged; ltg_list_mass
per slab and the four small all-reduces; ltg_replay_rows on every rank) against the unsharded Recommender on the whole catalogue, on a log
made by the unsharded Recommender(explore=): states, scores, M and first_bad identical, the estimates within the bounds of DESIGN 5.22, the
same tables on every rank; in one chunk and over several chunks with a short last one, with the log's head and with a longer one.

The two forwards agree bit for bit by the model of serving_harness.exact_sum_model, so what is left is the claim under test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOGP_TOL = 1e-4


def close(a, b, rel):
    """a within a relative `rel` of b; both nan (an estimate over no supported row) counts as equal"""
    return (a != a and b != b) or abs(a - b) <= rel * abs(b)


def main():
    import serving_harness as H
    from ltgan.sharded import Replay, ReplayLog, ShardedRecommender
    from ltgan.trainer import Explore, Recommender
    I, n_ev = int(sys.argv[1]), int(sys.argv[2])
    rank, world, dev = H.open_ranks()
    ref, eng, lo, hi = H.slab_engines(I, (16, 24, 40, 32), rank, world)
    rng = np.random.default_rng(3)
    fold, ev_full, ev_sh = H.exact_sum_model(rng, ref, eng, n_ev)
    labels = rng.integers(0, 3, I).astype(np.uint8)
    k, T0, F0, step, temps = 20, 0.7, 2, 900, [0.7, 0.4, 2.0]
    exp = Explore(T0, fixed=F0, draw=2)
    ids, _ = Recommender(ref, ev_full, k=k, chunk=n_ev, explore=exp).run(rng_step=step, keep_prob=1.0)
    y = (rng.random((n_ev, k)) < 0.25).astype(np.float32)
    log = ReplayLog(ids, exp.table(), y, fixed=F0, n_items=I)
    bits = H.bits
    rel = float(np.expm1(k * LOGP_TOL))
    worst, ess = 0.0, None
    for chunk, fixed in ((n_ev, None), (100, None), (100, 5)):
        rp = Replay(log, temps, fixed=fixed, labels=labels, n_groups=3, keep_logp1=True)
        ShardedRecommender(eng, ev_sh, k=0, chunk=chunk, replay=rp).run(rng_step=step, keep_prob=1.0)
        H.same_on_every_rank(rp.rows, rp.w, rp.first_bad, rp.state, rp.score, rp.top, rp.logp1)
        rp_1 = Replay(log, temps, fixed=fixed, labels=labels, n_groups=3, keep_logp1=True)
        Recommender(ref, ev_full, k=0, chunk=chunk, replay=rp_1).run(rng_step=step, keep_prob=1.0)
        t, t_1 = rp.table(), rp_1.table()
        assert np.array_equal(t["state"], t_1["state"]) and np.array_equal(bits(t["score"]), bits(t_1["score"]))
        assert np.array_equal(t["M"], t_1["M"]) and np.array_equal(t["first_bad"], t_1["first_bad"])
        if fixed is None:
            assert (t["first_bad"] == k).all()
        else:
            assert (t["first_bad"] < k).any()
        fin = np.isfinite(t_1["logp1"])
        assert np.array_equal(fin, np.isfinite(t["logp1"]))
        d = float(np.abs(t["logp1"][fin].astype(np.float64) - t_1["logp1"][fin]).max())
        worst = max(worst, d)
        assert d <= LOGP_TOL, d
        assert (np.abs(t["rows"] - t_1["rows"]) <= rel * np.abs(t_1["rows"])).all() and (np.abs(t["w"] - t_1["w"]) <= rel * t_1["w"]).all()
        est, est_1 = rp.estimates(), rp_1.estimates()
        ess = est_1[temps[0]]["ess"] if ess is None else ess
        for T in temps:
            assert est[T]["supported"] == est_1[T]["supported"] and close(est[T]["ess"], est_1[T]["ess"], 2 * rel)
            for name in ("0", "1", "2", "all"):
                for key in ("ips", "snips", "exposure"):
                    assert close(est[T][name][key], est_1[T][name][key], 2 * rel), (T, name, key)
    H.close_ranks("REPLAY_SHARDED_OK world=%d items=%d slabs=%s largest logp1 difference %.3g ess at the logging temperature %.2f of %d" % (
        world, I, H.slab_sizes(I, world), worst, ess, n_ev))


if __name__ == "__main__":
    main()
