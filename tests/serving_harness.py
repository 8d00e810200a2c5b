"""What the serving tests share: how a test starts rank processes and CLI children (parent side, used by test_*.py) and how a
dist_*_worker.py opens its ranks, builds its engines and its model (worker side).  A plain module: tests/ is on sys.path for pytest
(tests/conftest.py) and the workers insert it themselves; nothing here is a fixture.

Every child is a fresh process started with subprocess under `timeout -k 10 <limit>`; nothing is retried, and a child that failed or
ran out of time fails the test at once, so nothing is started after it."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
PKG = os.path.join(ROOT, "long-tail-gan_amd")
DEV = "cuda:0"

# ================================================================================================ parent side
# One port per launch site: "<test module>::<test function>[<case>]" -> (the script the ranks run, the rendezvous port).  Scripts named
# dist_*_worker.py / *_cpu_worker.py live in tests/, the others are the package's CLIs.
PORTS = {
    "test_gpu_sharded::test_two_rank_item_sharding_matches_unsharded": ("dist_shard_worker.py", 29577),
    "test_gpu_sharded::test_two_ranks_on_two_gpus_over_rccl": ("dist_shard_worker.py", 29579),
    "test_gpu_sharded::test_one_shot_exchange_equals_the_rank_ordered_host_transport": ("dist_oneshot_worker.py", 29583),
    "test_gpu_sharded::test_one_shot_exchange_gives_up_and_raises_when_a_peer_never_sends": ("dist_oneshot_worker.py", 29585),
    "test_gpu_sharded::test_four_rank_item_sharding_matches_unsharded": ("dist_shard_worker.py", 29587),
    "test_dist_cpu::test_gloo_exchange_algebra[2]": ("dist_cpu_worker.py", 29613),
    "test_dist_cpu::test_gloo_exchange_algebra[8]": ("dist_cpu_worker.py", 29619),
    "test_serving_cpu::test_world_size_two_lists_and_call_sequences": ("serving_cpu_worker.py", 29641),
    "test_gpu_topk::test_sharded_recommender": ("dist_topk_worker.py", 29643),
    "test_gpu_topk::test_recommender_recall_equals_rank_metrics_and_cli_equals_test_py": ("recommend.py", 29645),
    "test_gpu_neighbors::test_similar_cli_equals_the_class": ("similar.py", 29647),
    "test_gpu_neighbors::test_sharded_item_neighbors": ("dist_neighbors_worker.py", 29649),
    "test_gpu_companions::test_companions_cli_equals_the_class": ("companions.py", 29651),
    "test_gpu_companions::test_sharded_pair_companions": ("dist_companions_worker.py", 29653),
    "test_gpu_longtail::test_sharded_report": ("dist_longtail_worker.py", 29655),
    "test_gpu_longtail::test_cli_against_test_py": ("longtail.py", 29657),
    "test_gpu_quota::test_sharded_recommender_with_rule": ("dist_quota_worker.py", 29661),
    "test_gpu_diversify::test_sharded_recommender_with_diversify": ("dist_diversify_worker.py", 29671),
    "test_gpu_calibrate::test_sharded_recommender_with_calibrate": ("dist_calibrate_worker.py", 29673),
    "test_gpu_capped::test_sharded_recommender_with_cap": ("dist_capped_worker.py", 29674),
    "test_gpu_share::test_sharded_recommender_with_share": ("dist_share_worker.py", 29675),
    "test_gpu_floor::test_sharded_recommender_with_floor": ("dist_floor_worker.py", 29676),
    "test_gpu_audience::test_sharded_audience": ("dist_audience_worker.py", 29681),
    "test_gpu_explain::test_sharded_recommender_with_explain": ("dist_explain_worker.py", 29691),
    "test_gpu_critic::test_sharded_critic_and_gate": ("dist_critic_worker.py", 29695),
}
assert len({port for _, port in PORTS.values()}) == len(PORTS), "two launch sites share a rendezvous port"

RANK_ENV = {"MASTER_ADDR": "127.0.0.1", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "OMP_NUM_THREADS": "2"}

CONFIG = """[Long-Tail-GAN]
h0_size = 100
h1_size = 150
h2_size = 250
h3_size = 300
NUM_EPOCH = 8
BATCH_SIZE = 100
DISPLAY_ITER = 50
LEARNING_RATE = 0.0001
to_restore = 0
model_name = LT_GAN
GANLAMBDA = 1.0
"""


def _site():
    """the launch site pytest is running: tests/test_gpu_floor.py::test_x[2] (call) -> test_gpu_floor::test_x"""
    path, _, rest = os.environ["PYTEST_CURRENT_TEST"].partition("::")
    return "%s::%s" % (os.path.splitext(os.path.basename(path))[0], rest.split("[")[0].split(" ")[0])


def _ranks(script, args, world, port_of, env, limit, cwd=None):
    """one fresh `torch.distributed.run` child of `world` ranks on this host, under its own time limit -> the CompletedProcess"""
    name, port = PORTS[port_of or _site()]
    assert name == os.path.basename(script), (name, script)
    full = dict(os.environ)
    for key, value in dict(RANK_ENV, **(env or {})).items():       # a value of None leaves the variable as this process has it
        if value is not None:
            full[key] = value
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), script] + [str(a) for a in args]
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=full, timeout=limit + 100)


def run_ranks(worker, args, world, ok, port_of=None, limit=900, env=None):
    """`world` gloo ranks of tests/<worker> sharing this host (and its one GPU).  The port is PORTS[port_of], by default the entry of the
    test that is running; `env` adds to RANK_ENV.  Prints the end of the child's stdout, asserts that it exited with 0 AND printed the
    token `ok`, and returns its stdout."""
    out = _ranks(os.path.join(TESTS, worker), args, world, port_of, env, limit)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-3000:] + out.stderr[-6000:]
    return out.stdout


def run_cli(script, args, cwd, world=1, limit=600, port_of=None):
    """a fresh child of the package CLI `script` in `cwd`; with world > 1 as that many gloo ranks sharing the GPU (LTGAN_DIST_BACKEND=gloo,
    the thread count left as it is).  Asserts on the return code with the output's ends -> the stripped stdout lines"""
    path = os.path.join(PKG, script)
    if world > 1:
        r = _ranks(path, args, world, port_of, {"LTGAN_DIST_BACKEND": "gloo", "OMP_NUM_THREADS": None}, limit, cwd)
    else:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, path] + [str(a) for a in args], cwd=cwd, capture_output=True,
                           text=True, timeout=limit + 100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().splitlines()


def askubuntu_run(tmp_path, device=DEV, model=True, split="test"):
    """Askubuntu_Sample materialised under tmp_path and a run directory with config.ini -> (ds, cwd, n_items); with `model` also a
    generator at config.ini's sizes, its checkpoint and the split's fold-in / held-out rows ->
    (ds, cwd, n_items, engine, model_0.pt, tr, te, uid0)"""
    from ltgan.dataset import count_items, materialize_askubuntu
    ds = str(tmp_path / "Askubuntu_Sample")
    materialize_askubuntu(os.path.join(TESTS, "golden", "askubuntu_raw.npz"), ds)
    cwd = str(tmp_path / "run")
    os.makedirs(cwd)
    open(os.path.join(cwd, "config.ini"), "w").write(CONFIG)
    n_items = count_items(ds)
    if not model:
        return ds, cwd, n_items
    from ltgan import data_processing as dp
    from ltgan.generator import generator_VAECF
    from ltgan.test import _Counters
    from ltgan.train import save_checkpoint
    gen, *_ = generator_VAECF(ds + "/", h_sizes=(100, 150, 250, 300), lr=1e-4, precision="bf16", device=device)
    ck = os.path.join(cwd, "model_0.pt")
    save_checkpoint(ck, gen.engine, _Counters(), 0)
    rows = (None, None, None)                            # split=None: a test that reads no rows
    if split is not None:
        rows = dp.load_tr_te_data(os.path.join(ds, "%s_tr.csv" % split), os.path.join(ds, "%s_te.csv" % split), n_items)
    return (ds, cwd, n_items, gen.engine, ck) + tuple(rows)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_bits = bits


def _cfg(cabi, n_items, h=600, item_lo=0, n_glob=0):
    return cabi.ltg_config(n_items, h, 200, n_items, 100, 150, 250, 300, 0, 0, item_lo, n_glob, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


def _pack_dev(W, metric, space="decoder"):
    """ltg_item_pack on a host table [I, H] float32 -> the image as a device int16 tensor [I, 608]"""
    import ctypes as C
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    Wd = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).cuda()
    I, H = W.shape
    gen = cabi.ltg_gen_state()
    gen.p[3 if space == "decoder" else 0] = Wd.data_ptr()
    img = torch.full((I, 608), 0x5555, dtype=torch.int16, device="cuda")      # (the pad columns must be WRITTEN)
    rc = lib.ltg_item_pack(C.byref(_cfg(cabi, I, H)), C.byref(gen), cabi.LTG_SPACE[space], cabi.LTG_METRIC[metric], img.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return img


def _nbr_dev(table, q_img, q_gid, k, labels=None, mask=0x1FF, item_lo=0, n_glob=0):
    """ltg_item_neighbors: table / q_img device int16 images, q_gid host int32, labels host uint8 per GLOBAL id -> host (scores, ids)"""
    import ctypes as C
    import torch
    from ltgan import _cabi as cabi
    lib = cabi.load()
    I, n = int(table.shape[0]), int(q_img.shape[0])
    cfg = _cfg(cabi, I, 600, item_lo, n_glob)
    gid = torch.from_numpy(np.ascontiguousarray(q_gid, dtype=np.int32)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8)).cuda() if labels is not None else None
    need = lib.ltg_item_neighbors_ws_bytes(C.byref(cfg), n, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s = torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
    i = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    rc = lib.ltg_item_neighbors(C.byref(cfg), table.data_ptr(), q_img.data_ptr(), gid.data_ptr(), n, lab.data_ptr() if lab is not None else None,
                                mask, k, s.data_ptr(), i.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _small_engine(I=1024, steps=0, seed=1234, **kw):
    """an Engine with the reference's initialisation, optionally moved by a few G steps (smoke()'s step on random histories)"""
    import torch
    import helpers as Hh
    from ltgan.engine import CsrRows, Engine, Pairs
    from oracle import ltg_oracle as O
    B = 16
    rng = np.random.default_rng(0)
    eng = Engine(I, h_sizes=(16, 24, 40, 32), lr=1e-3, precision="bf16", seed=seed, **kw)
    if not eng.sharded:
        eng.set_generator(Hh.gen_to_engine(O.init_generator(I, seed=1)))
    dev = eng.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for st in range(steps):
        X = Hh.random_history(rng, B, I, mean_nnz=9)
        slot, uptr, rowidx, pos, nu = Hh.csc_view(X)
        batch = CsrRows(t(X.indptr.astype(np.int32)), t(X.indices.astype(np.int32)), 0, B, slot=t(slot), uptr=t(uptr), rowidx=t(rowidx),
                        csr_pos=t(pos), n_unique=nu)
        acts = eng.new_acts(B)
        rows = np.repeat(np.arange(B, dtype=np.int32), 2)
        fake = Pairs(t(rng.integers(0, I, 2 * B).astype(np.int32)), t(rng.integers(0, I, 2 * B).astype(np.int32)), t(rows))
        cnt = torch.tensor([2 * B], dtype=torch.int32, device=dev)
        eng.g_step(batch, fake, acts, cnt, anneal=0.1, rng_step=3 + 2 * st, d_rng_step=4 + 2 * st)
    torch.cuda.synchronize()
    return eng


# ================================================================================================ worker side
def open_ranks(backend="gloo", dev=DEV):
    """the worker's process group, every rank on the one GPU (dev=None: a CPU worker) -> (rank, world, dev)"""
    import torch
    import torch.distributed as dist
    dist.init_process_group(backend)
    if dev is not None:
        torch.cuda.set_device(dev)
    return dist.get_rank(), dist.get_world_size(), dev


def close_ranks(token_line):
    """every rank got here: rank 0 prints the line that carries the worker's OK token, and the group is taken down"""
    import torch.distributed as dist
    dist.barrier()
    if dist.get_rank() == 0:
        print(token_line)
    dist.destroy_process_group()


def slabs(I, world):
    from ltgan.sharded import item_slab
    return [item_slab(I, r, world) for r in range(world)]


def slab_sizes(I, world):
    """the distinct slab widths, as the OK lines print them"""
    return sorted({hi - lo for lo, hi in slabs(I, world)})


def slab_engines(I, h_sizes, rank, world, dev=DEV, lr=1e-3, precision="bf16", seed=77, d_seed=3):
    """an engine on the whole catalogue and this rank's slab engine, from the same seeds -> (ref, eng, lo, hi)"""
    from ltgan.engine import Engine
    from ltgan.sharded import item_slab
    ref = Engine(I, h_sizes=h_sizes, lr=lr, precision=precision, seed=seed, d_seed=d_seed, device=dev)
    lo, hi = item_slab(I, rank, world)
    eng = Engine(I, h_sizes=h_sizes, lr=lr, precision=precision, seed=seed, d_seed=d_seed, device=dev, item_lo=lo, item_hi=hi)
    return ref, eng, lo, hi


def exact_sum_arrays(rng, I, H, n_ev):
    """the arrays of exact_sum_model, drawn from rng in this order: the item bias in [1, 3] (logits of a trained model's size, see
    dist_topk_worker.py), W_q0 in multiples of 1/64 in [-1, 1], 16 distinct fold-in items per user -> (bias [I], wq0 [I, H], fold CSR
    [n_ev, I] with sorted indices).  Pure numpy; the caller goes on drawing from rng."""
    import scipy.sparse as sp
    bias = rng.uniform(1.0, 3.0, I).astype(np.float32)
    wq0 = (rng.integers(-64, 65, (I, H)) / 64.0).astype(np.float32)
    cols = np.concatenate([rng.choice(I, 16, replace=False) for _ in range(n_ev)])
    fold = sp.csr_matrix((np.ones(16 * n_ev, np.float32), (np.repeat(np.arange(n_ev), 16), cols)), shape=(n_ev, I))
    fold.sort_indices()
    return bias, wq0, fold


def exact_sum_model(rng, ref, eng, n_ev, dev=DEV):
    """A model on which the sharded and the unsharded forward agree BIT FOR BIT -> (fold, ev_full, ev_sh), the fold-in rows also being
    the held-out ones.

    The sharded forward all-reduces the encoder's partial pre-activations, which in general sums in another order than the unsharded
    forward (dist_topk_worker.py: near-ties swap).  Here that sum is exact: W_q0 holds multiples of 1/64 in [-1, 1], every user has 16
    fold-in items and dropout is off (the workers run with keep_prob=1.0), so every partial sum is a multiple of 1/64 below 16 -- exact
    in fp32 in any order -- and the row scale is 1/sqrt(16) = 1/4, a power of two.  What is left of a difference between the two
    recommenders is then the claim under test and not the forward."""
    import torch
    from ltgan.dataset import EvalData
    bias, wq0, fold = exact_sum_arrays(rng, ref.I, ref.H, n_ev)
    bias, wq0 = torch.from_numpy(bias).to(dev), torch.from_numpy(wq0).to(dev)
    lo, hi = eng.item_lo, eng.item_hi
    ref.g_p[7].copy_(bias)
    eng.g_p[7].copy_(bias[lo:hi])
    ref.g_p[0].copy_(wq0)
    eng.g_p[0].copy_(wq0[lo:hi])
    return fold, EvalData(fold, fold, dev), EvalData(fold, fold, dev, item_lo=lo, item_hi=hi)


def gathered_logits(mine, lo, hi, I, world):
    """the [n, I] logits of the whole catalogue, all-gathered from every rank's [n, hi - lo] slab logits `mine` of one sharded forward"""
    import torch
    import torch.distributed as dist
    cuts = slabs(I, world)
    pad = torch.zeros(mine.shape[0], max(b - a for a, b in cuts), dtype=torch.float32, device=mine.device)
    pad[:, : hi - lo] = mine
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    return torch.cat([p[:, : b - a] for p, (a, b) in zip(parts, cuts)], dim=1).contiguous()


def same_on_every_rank(*tensors):
    """every rank holds the same tables: each device tensor equals rank 0's"""
    import torch
    import torch.distributed as dist
    for a in tensors:
        a0 = a.clone()
        dist.broadcast(a0, 0)
        assert torch.equal(a, a0)
