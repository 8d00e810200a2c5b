#!/usr/bin/env python3
"""Standalone timing of ltg_pair_companions alone at config.ini's sizes (100 / 150 / 250 / 300): 4 096 popular queries x the niche side of the
200 000-item synthetic catalogue (niche = 90 %: 180 000 candidates), k = 20, the reference's discriminator initialiser x 2 (a trained model's
range).  Both side images are packed once outside the timed region (ltg_pair_pack is timed on its own); device events around each call,
3 warm-up calls, then `reps` timed ones (default 15) on an otherwise idle device, the clocks as found -- nothing is set.  Prints one JSON
line: median / min / max, the reciprocal-rate floor of DESIGN 5.19 beside it, the workspace and the bytes a score table would have taken.
usage: companions_timing.py [reps] [n_q] [n_c] [k]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# per element one v_rcp_f32 (8 cycles of a SIMD per wave instruction) and two v_fma_f32 (2 each, two waves per SIMD)
SIMDS, CLOCK_HZ, CYC_RCP, CYC_ALL = 256 * 4, 2.4e9, 8, 12


def main():
    from ltgan import _cabi as cabi
    from ltgan.engine import init_discriminator_host
    lib = cabi.load()
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    reps, n_q, n_c, k = arg(1, 15), arg(2, 4096), arg(3, 180000), arg(4, 20)
    I, hs = 200000, (100, 150, 250, 300)
    dev = "cuda:0"
    st = lambda: torch.cuda.current_stream().cuda_stream
    cfg = cabi.ltg_config(I, 600, 200, I, *hs, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    emb, host = init_discriminator_host(I, hs, 0)
    t = [torch.from_numpy(np.ascontiguousarray(2.0 * a if a.ndim == 2 or i == 7 else a, dtype=np.float32).reshape(-1)).to(dev)
         for i, a in enumerate([emb] + list(host))]
    disc = cabi.ltg_disc_state()
    disc.emb = t[0].data_ptr()
    for i in range(8):
        disc.p[i] = t[1 + i].data_ptr()
    ld = lib.ltg_pair_ld(C.byref(cfg))
    rng = np.random.default_rng(1)
    c = torch.from_numpy(np.sort(rng.choice(I, n_c, replace=False)).astype(np.int32)).to(dev)
    q = torch.from_numpy(rng.choice(I, n_q, replace=False).astype(np.int32)).to(dev)
    q_img = torch.empty(n_q, ld, dtype=torch.float32, device=dev)
    c_img = torch.empty(n_c, ld, dtype=torch.float32, device=dev)
    need = lib.ltg_pair_companions_ws_bytes(C.byref(cfg), n_q, n_c, k)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = torch.empty(n_q, k, dtype=torch.float32, device=dev)
    i_out = torch.empty(n_q, k, dtype=torch.int32, device=dev)

    def pack():
        cabi.check(lib.ltg_pair_pack(C.byref(cfg), C.byref(disc), 0, q.data_ptr(), n_q, q_img.data_ptr(), st()), "ltg_pair_pack")
        cabi.check(lib.ltg_pair_pack(C.byref(cfg), C.byref(disc), 1, c.data_ptr(), n_c, c_img.data_ptr(), st()), "ltg_pair_pack")

    def search():
        cabi.check(lib.ltg_pair_companions(C.byref(cfg), C.byref(disc), q_img.data_ptr(), q.data_ptr(), n_q, c_img.data_ptr(), c.data_ptr(), n_c, k,
                                           s.data_ptr(), i_out.data_ptr(), ws.data_ptr(), need, st()), "ltg_pair_companions")

    for _ in range(3):
        pack()
        search()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tm = {"pack": [], "search": []}
    for _ in range(reps):
        for name, fn in (("pack", pack), ("search", search)):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            tm[name].append(e0.elapsed_time(e1) * 1e3)
    elements = float(n_q) * n_c * hs[3]
    out = dict(n_q=n_q, n_c=n_c, k=k, h3=hs[3], reps=reps, workspace_bytes=int(need), score_table_bytes=n_q * n_c * 4,
               rcp_floor_us=round(elements / 64 * CYC_RCP / SIMDS / CLOCK_HZ * 1e6, 1),
               fma_rcp_fma_floor_us=round(elements / 64 * CYC_ALL / SIMDS / CLOCK_HZ * 1e6, 1), mean_prob_at_1=round(float(torch.sigmoid(s[:, 0]).mean()), 4))
    for name, v in tm.items():
        out[name + "_us_median"] = round(float(np.median(v)), 1)
        out[name + "_us_min"] = round(float(min(v)), 1)
        out[name + "_us_max"] = round(float(max(v)), 1)
    out["search_over_rcp_floor"] = round(out["search_us_median"] / out["rcp_floor_us"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
