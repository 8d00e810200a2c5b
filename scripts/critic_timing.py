#!/usr/bin/env python3
"""DESIGN 5.20's numbers: python scripts/critic_timing.py [out.json] on an MI355X.  Wall time of recommend.py's walk (Recommender.run, which
ends in a device-to-host copy) on Askubuntu_Sample at k = 100 with a freshly initialised model: plain, with critic=, with gate= 0.5 --
one warm-up each, then nine rounds that alternate the three; plus device-event times of the critic's own calls (20 each after a warm-up)
and the counts that bound them: anchors x scored entries pairs, reciprocals, bytes gathered."""
import json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ltgan  # noqa: F401  (alias of the package directory)
import torch
from ltgan import data_processing as dp, longtail as lt, recommend as rc
from ltgan.dataset import EvalData, count_items, materialize_askubuntu
from ltgan.generator import generator_VAECF
from ltgan.serving import Critic, CriticGate, Recommender, SlabLists

tmp = tempfile.mkdtemp()
ds = os.path.join(tmp, "Askubuntu_Sample")
materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), ds)
n_items = count_items(ds)
gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device="cuda:0")
eng = gen.engine
tr, te, uid0 = dp.load_tr_te_data(os.path.join(ds, "test_tr.csv"), os.path.join(ds, "test_te.csv"), n_items)
niche, valid = lt.critic_sides(ds, n_items)
ev = EvalData(tr, te, eng.device)
k = 100
crt, gate = Critic(niche, valid), CriticGate(niche, valid, 0.5)
recs = dict(plain=Recommender(eng, ev, k=k), critic=Recommender(eng, ev, k=k, critic=crt), gate=Recommender(eng, ev, k=k, gate=gate))
for r in recs.values():
    r.run(rng_step=rc.RNG_STEP)
torch.cuda.synchronize()
times = {name: [] for name in recs}
for rnd in range(9):
    for name, r in recs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run(rng_step=rc.RNG_STEP)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) * 1e3)
out = dict(users=int(ev.n), items=int(n_items), n_pop=int(crt.sides.pop_host.size), n_niche=int(crt.sides.niche_host.size), chunks=len(range(0, ev.n, recs["plain"].chunk)))
for name, t in times.items():
    out["walk_ms_" + name] = dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)))


def ev_time(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))


n = ev.n
trr = ev.rows(0, n)[0]
new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=eng.device)
for label, sides, ids, top in (("critic_top100", crt.sides, recs["critic"].ids, 100),):
    acc, cnt, b_s, b_i, crit, sc = new(n, top, dt=torch.int64), new(n, dt=torch.int32), new(n, top), new(n, top, dt=torch.int32), new(n, top), new(n, dt=torch.int32)
    out["call_ms_pair_critic_" + label] = ev_time(lambda: eng.pair_critic(sides.pop_img, sides.niche_img, sides.pop_row, sides.niche_row, trr, ids, top, acc, cnt, b_s, b_i, hist_lo=0))
    out["call_ms_critic_finish_" + label] = ev_time(lambda: eng.critic_finish(ids, top, sides.niche_row, int(sides.niche_host.size), acc, cnt, crit, sc))
    out["call_ms_pack_both"] = ev_time(lambda: sides.pack(eng))
    torch.cuda.synchronize()
    cn, s = cnt.cpu().numpy().astype(np.int64), sc.cpu().numpy().astype(np.int64)
    cand = (b_i.cpu().numpy() >= 0).sum(1)
    out[label] = dict(anchors_mean=float(cn.mean()), anchors_max=int(cn.max()), users_with_anchors=int((cn > 0).sum()), scored=int(s.sum()),
                      pairs=int((cn * s).sum()), rcp=int((cn * s).sum()) * 300,
                      tile_bytes=int(((s + 63) // 64 * 64 * 300 * 4).sum()), anchor_row_bytes=int((cn * ((s + 63) // 64) * 300 * 4).sum()))
# the gate's critic: 200 candidates
c = gate.c
wide = Recommender(eng, ev, k=c)
wide.run(rng_step=rc.RNG_STEP)
acc, cnt, b_s, b_i, crit, sc = new(n, c, dt=torch.int64), new(n, dt=torch.int32), new(n, c), new(n, c, dt=torch.int32), new(n, c), new(n, dt=torch.int32)
gs, gi, st = new(n, k), new(n, k, dt=torch.int32), new(n, 3, dt=torch.int32)
sides = gate.sides
out["call_ms_pair_critic_gate_c%d" % c] = ev_time(lambda: eng.pair_critic(sides.pop_img, sides.niche_img, sides.pop_row, sides.niche_row, trr, wide.ids, c, acc, cnt, b_s, b_i, hist_lo=0))
eng.critic_finish(wide.ids, c, sides.niche_row, int(sides.niche_host.size), acc, cnt, crit, sc)
out["call_ms_topk_gate"] = ev_time(lambda: eng.topk_gate(wide.scores, wide.ids, crit, b_i, 0.0, k, gs, gi, st))
out["call_ms_topk_c%d" % c] = ev_time(lambda: wide.lists.topk(wide.acts, trr, n, c, wide.scores, wide.ids))
out["call_ms_topk_k%d" % k] = ev_time(lambda: recs["plain"].lists.topk(recs["plain"].acts, trr, n, k, recs["plain"].scores, recs["plain"].ids))
cn, s = cnt.cpu().numpy().astype(np.int64), sc.cpu().numpy().astype(np.int64)
out["gate_c%d" % c] = dict(scored=int(s.sum()), pairs=int((cn * s).sum()), rcp=int((cn * s).sum()) * 300, rejected=int(gate.stats()[:, 1].sum()))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
